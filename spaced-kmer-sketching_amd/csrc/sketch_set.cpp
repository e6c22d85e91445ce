// C-ABI implementation (include/sks.h): device sketch sets — the one place
// that makes a set, the accessors, copy, export and free, and the entry points
// that move sets between a device and sketch files (format: persist.cpp).
#include <utility>

#include "sks_ctx.hpp"

using namespace sks;

int sks::make_sketch_set(int device, int elem_words, int window, const uint64_t mask[2], const sks_policy& policy,
                         std::vector<uint32_t> sizes, std::vector<uint64_t> windows, std::vector<std::string> names,
                         const uint64_t* data_words, hipStream_t st, MetaUpload up, SetPtr* out, DevBlock* abund) {
  SetPtr set(new (std::nothrow) sks_sketch_set());
  if (!set) return sks::fail(SKS_E_NOMEM, "sketch set: out of memory");
  const uint32_t n = (uint32_t)sizes.size();
  set->device = device;
  set->elem_words = elem_words;
  set->n = n;
  set->window = window;
  set->mask[0] = mask[0];
  set->mask[1] = mask[1];
  set->policy = policy;
  set->starts.resize(n);
  uint64_t total = 0;
  for (uint32_t g = 0; g < n; ++g) {
    set->starts[g] = total;
    total += sizes[g];
  }
  set->sizes = std::move(sizes);
  set->windows = std::move(windows);
  set->names = std::move(names);
  if (data_words) SKS_TRY(alloc_u64(set->data, *data_words, st));
  if (abund) set->abund = std::move(*abund);
  SKS_TRY(alloc_u64(set->dstarts, n, st));
  SKS_HIP(set->dsizes.alloc(std::max<uint32_t>(n, 1) * sizeof(uint32_t), st));
  if (n && up == MetaUpload::kStream) {
    SKS_HIP(sks::pinned_h2d(set->d_starts(), set->starts.data(), n * sizeof(uint64_t), st));
    SKS_HIP(sks::pinned_h2d(set->d_sizes(), set->sizes.data(), n * sizeof(uint32_t), st));
  } else if (n && up == MetaUpload::kBlocking) {
    SKS_HIP(hipMemcpy(set->d_starts(), set->starts.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
    SKS_HIP(hipMemcpy(set->d_sizes(), set->sizes.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  *out = std::move(set);
  return SKS_OK;
}

namespace {

uint64_t elements(const sks_sketch_set* set) {
  uint64_t total = 0;
  for (uint32_t v : set->sizes) total += v;
  return total;
}

// Uploads host sketches, or copies device ones, into a new device set; with
// host_abund or device_abund (one u32 per element) a counted one.
int make_device_set(int device, const sks::SketchFileMeta& meta, const std::vector<uint32_t>& sizes,
                    const std::vector<uint64_t>& windows, const uint64_t* host_data, const uint64_t* device_data,
                    std::vector<std::string> names, sks_sketch_set** out, const uint32_t* host_abund = nullptr,
                    const uint32_t* device_abund = nullptr) {
  uint64_t words = 0, total = 0;
  for (uint32_t v : sizes) total += v;
  words = total * meta.elem_words;
  DevBlock abund;
  if (host_abund || device_abund) SKS_HIP(abund.alloc(std::max<uint64_t>(total, 1) * sizeof(uint32_t), nullptr));
  SetPtr set;
  SKS_TRY(make_sketch_set(device, meta.elem_words, meta.window, meta.mask, meta.policy, sizes, windows,
                          std::move(names), &words, nullptr, MetaUpload::kBlocking, &set,
                          abund ? &abund : nullptr));
  if (words && host_data) SKS_HIP(hipMemcpy(set->d_data(), host_data, words * 8, hipMemcpyHostToDevice));
  if (words && device_data) SKS_HIP(hipMemcpy(set->d_data(), device_data, words * 8, hipMemcpyDeviceToDevice));
  if (total && host_abund) SKS_HIP(hipMemcpy(set->d_abund(), host_abund, total * 4, hipMemcpyHostToDevice));
  if (total && device_abund) SKS_HIP(hipMemcpy(set->d_abund(), device_abund, total * 4, hipMemcpyDeviceToDevice));
  *out = set.release();
  return SKS_OK;
}

sks::SketchFileMeta file_meta_of(const sks_sketch_set* set) {
  sks::SketchFileMeta meta;
  meta.window = set->window;
  meta.elem_words = set->elem_words;
  meta.mask[0] = set->mask[0];
  meta.mask[1] = set->mask[1];
  meta.policy = set->policy;
  return meta;
}

}  // namespace

extern "C" {

int sks_sketch_set_free(sks_sketch_set* set) {
  if (!set) return SKS_OK;
  DeviceGuard g(set->device);
  // hipFree's contract: work queued on the arrays (any stream) completes before
  // they are reused; then they go to the block cache instead of being unmapped
  if (set->data || set->dstarts || set->dsizes || set->abund) (void)hipDeviceSynchronize();
  for (DevBlock* b : {&set->data, &set->dstarts, &set->dsizes, &set->abund}) b->release();
  delete set;
  return SKS_OK;
}

int sks_sketch_set_free_on_stream(sks_sketch_set* set, void* stream) {
  if (!set) return SKS_OK;
  DeviceGuard g(set->device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (DevBlock* b : {&set->data, &set->dstarts, &set->dsizes, &set->abund}) b->release_after(st);
  delete set;
  return SKS_OK;
}

uint32_t sks_sketch_set_num(const sks_sketch_set* set) { return set ? set->n : 0; }

int sks_sketch_set_elem_words(const sks_sketch_set* set) { return set ? set->elem_words : 0; }

int sks_sketch_set_sizes(const sks_sketch_set* set, uint32_t* sizes) {
  if (!set || !sizes) return sks::fail(SKS_E_ARG, "sks_sketch_set_sizes: null argument");
  std::copy(set->sizes.begin(), set->sizes.end(), sizes);
  return SKS_OK;
}

int sks_sketch_set_windows(const sks_sketch_set* set, uint64_t* windows) {
  if (!set || !windows) return sks::fail(SKS_E_ARG, "sks_sketch_set_windows: null argument");
  std::copy(set->windows.begin(), set->windows.end(), windows);
  return SKS_OK;
}

int sks_sketch_set_starts(const sks_sketch_set* set, uint64_t* starts) {
  if (!set || !starts) return sks::fail(SKS_E_ARG, "sks_sketch_set_starts: null argument");
  std::copy(set->starts.begin(), set->starts.end(), starts);
  return SKS_OK;
}

const uint64_t* sks_sketch_set_device_data(const sks_sketch_set* set) { return set ? set->d_data() : nullptr; }
const uint64_t* sks_sketch_set_device_starts(const sks_sketch_set* set) { return set ? set->d_starts() : nullptr; }
const uint32_t* sks_sketch_set_device_sizes(const sks_sketch_set* set) { return set ? set->d_sizes() : nullptr; }

int sks_sketch_set_copy(const sks_sketch_set* set, uint32_t i, uint64_t* out) {
  if (!set) return sks::fail(SKS_E_ARG, "sks_sketch_set_copy: null set");
  if (i >= set->n) return sks::fail(SKS_E_ARG, "sks_sketch_set_copy: index out of range");
  if (!out && set->sizes[i]) return sks::fail(SKS_E_ARG, "sks_sketch_set_copy: null output");
  DeviceGuard g(set->device);
  uint64_t words = (uint64_t)set->sizes[i] * set->elem_words;
  if (words)
    SKS_HIP(hipMemcpy(out, set->d_data() + set->starts[i] * set->elem_words, words * sizeof(uint64_t),
                      hipMemcpyDeviceToHost));
  return SKS_OK;
}

int sks_sketch_set_has_abund(const sks_sketch_set* set) { return set && set->has_abund() ? 1 : 0; }

const uint32_t* sks_sketch_set_device_abund(const sks_sketch_set* set) { return set ? set->d_abund() : nullptr; }

int sks_sketch_set_abund_copy(const sks_sketch_set* set, uint32_t i, uint32_t* out) {
  if (!set) return sks::fail(SKS_E_ARG, "sks_sketch_set_abund_copy: null set");
  if (!set->has_abund()) return sks::fail(SKS_E_ARG, "sks_sketch_set_abund_copy: the set has no abundance column");
  if (i >= set->n) return sks::fail(SKS_E_ARG, "sks_sketch_set_abund_copy: index out of range");
  if (!out && set->sizes[i]) return sks::fail(SKS_E_ARG, "sks_sketch_set_abund_copy: null output");
  DeviceGuard g(set->device);
  if (set->sizes[i])
    SKS_HIP(hipMemcpy(out, set->d_abund() + set->starts[i], (size_t)set->sizes[i] * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
  return SKS_OK;
}

int sks_sketch_set_export(const sks_sketch_set* set, uint64_t* d_dst, uint64_t stride, uint32_t* d_sizes) {
  if (!set || !d_dst || !d_sizes) return sks::fail(SKS_E_ARG, "sks_sketch_set_export: null argument");
  for (uint32_t s : set->sizes)
    if (s > stride) return sks::fail(SKS_E_ARG, "sks_sketch_set_export: stride smaller than a sketch");
  DeviceGuard g(set->device);
  SKS_HIP(sks::launch_export(set->d_data(), set->d_starts(), set->d_sizes(), set->n, set->elem_words, d_dst, stride,
                             d_sizes, nullptr));
  SKS_HIP(hipStreamSynchronize(nullptr));
  return SKS_OK;
}

int sks_sketch_set_export_csr(const sks_sketch_set* set, uint64_t* d_data, uint32_t* d_sizes) {
  if (!set) return sks::fail(SKS_E_ARG, "sks_sketch_set_export_csr: null set");
  DeviceGuard g(set->device);
  const uint64_t total = elements(set);
  if ((total && !d_data) || (set->n && !d_sizes))
    return sks::fail(SKS_E_ARG, "sks_sketch_set_export_csr: null argument");
  // the set's arrays are CSR in sketch order: one copy each
  if (total)
    SKS_HIP(hipMemcpy(d_data, set->d_data() + set->starts[0] * set->elem_words,
                      total * set->elem_words * sizeof(uint64_t), hipMemcpyDeviceToDevice));
  if (set->n) SKS_HIP(hipMemcpy(d_sizes, set->d_sizes(), set->n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
  return SKS_OK;
}

int sks_sketch_set_info(const sks_sketch_set* set, sks_sketch_info* info) {
  if (!set || !info) return sks::fail(SKS_E_ARG, "sks_sketch_set_info: null argument");
  *info = info_of(*set);
  return SKS_OK;
}

const char* sks_sketch_set_name(const sks_sketch_set* set, uint32_t i) {
  if (!set || i >= set->names.size()) return nullptr;
  return set->names[i].c_str();
}

int sks_sketch_set_set_names(sks_sketch_set* set, const char* const* names) {
  if (!set) return sks::fail(SKS_E_ARG, "sks_sketch_set_set_names: null set");
  std::vector<std::string> v;
  if (names)
    for (uint32_t i = 0; i < set->n; ++i) {
      if (!names[i]) return sks::fail(SKS_E_ARG, "sks_sketch_set_set_names: null name");
      v.emplace_back(names[i]);
    }
  set->names = std::move(v);
  return SKS_OK;
}

int sks_sketch_set_save(const sks_sketch_set* set, const char* path) {
  if (!set || !path) return sks::fail(SKS_E_ARG, "sks_sketch_set_save: null argument");
  DeviceGuard g(set->device);
  std::vector<uint64_t> host(elements(set) * set->elem_words);
  if (!host.empty()) SKS_HIP(hipMemcpy(host.data(), set->d_data(), host.size() * 8, hipMemcpyDeviceToHost));
  if (!set->has_abund())
    return sks::write_sketch_file(path, file_meta_of(set), set->sizes, set->windows, host.data(), set->names);
  std::vector<uint32_t> abund(elements(set));
  if (!abund.empty()) SKS_HIP(hipMemcpy(abund.data(), set->d_abund(), abund.size() * 4, hipMemcpyDeviceToHost));
  return sks::write_sketch_file(path, file_meta_of(set), set->sizes, set->windows, host.data(), set->names, &abund);
}

int sks_sketch_set_load(sks_ctx* ctx, const char* path, sks_sketch_set** out) {
  if (!ctx || !path || !out) return sks::fail(SKS_E_ARG, "sks_sketch_set_load: null argument");
  *out = nullptr;
  sks::SketchFileMeta meta;
  std::vector<uint32_t> sizes;
  std::vector<uint64_t> windows, data;
  std::vector<std::string> names;
  std::vector<uint32_t> abund;
  bool counted = false;
  SKS_TRY(sks::read_sketch_file(path, meta, sizes, windows, data, names, &abund, &counted));
  DeviceGuard g(ctx->device);
  return make_device_set(ctx->device, meta, sizes, windows, data.data(), nullptr, std::move(names), out,
                         counted ? abund.data() : nullptr);
}

int sks_sketch_set_concat(sks_ctx* ctx, const sks_sketch_set* const* sets, uint32_t n_sets, sks_sketch_set** out) {
  if (!ctx || !out || (n_sets && !sets)) return sks::fail(SKS_E_ARG, "sks_sketch_set_concat: null argument");
  *out = nullptr;
  if (n_sets == 0) return sks::fail(SKS_E_ARG, "sks_sketch_set_concat: no sets");
  const sks_sketch_set* a = sets[0];
  bool names = true;
  uint32_t counted = 0;
  for (uint32_t i = 0; i < n_sets; ++i) {
    const sks_sketch_set* b = sets[i];
    if (!b) return sks::fail(SKS_E_ARG, "sks_sketch_set_concat: null set");
    if (set_differs_in(info_of(*a), info_of(*b), ParamRule::kAlways))
      return sks::fail(SKS_E_ARG, "sks_sketch_set_concat: sets differ in window, mask or policy");
    names = names && (b->names.size() == b->n);
    counted += b->has_abund() ? 1 : 0;
  }
  if (counted != 0 && counted != n_sets)
    return sks::fail(SKS_E_ARG, "sks_sketch_set_concat: some sets have an abundance column and some have none");
  DeviceGuard g(ctx->device);
  std::vector<uint32_t> sizes;
  std::vector<uint64_t> windows;
  std::vector<std::string> all_names;
  uint64_t total = 0;
  for (uint32_t i = 0; i < n_sets; ++i) {
    total += elements(sets[i]);
    sizes.insert(sizes.end(), sets[i]->sizes.begin(), sets[i]->sizes.end());
    windows.insert(windows.end(), sets[i]->windows.begin(), sets[i]->windows.end());
    if (names) all_names.insert(all_names.end(), sets[i]->names.begin(), sets[i]->names.end());
  }
  const int ew = a->elem_words;
  DevBlock staged;  // the sets' elements back to back (the sets may live on other devices)
  SKS_TRY(alloc_u64(staged, total * ew, nullptr));
  uint64_t at = 0;
  for (uint32_t i = 0; i < n_sets; ++i) {
    const uint64_t words = elements(sets[i]) * ew;
    if (words) SKS_HIP(hipMemcpy(staged.as<uint64_t>() + at, sets[i]->d_data(), words * 8, hipMemcpyDefault));
    at += words;
  }
  DevBlock staged_abund;  // and their abundances, when all have them
  if (counted) {
    SKS_HIP(staged_abund.alloc(std::max<uint64_t>(total, 1) * sizeof(uint32_t), nullptr));
    uint64_t el = 0;
    for (uint32_t i = 0; i < n_sets; ++i) {
      const uint64_t m = elements(sets[i]);
      if (m) SKS_HIP(hipMemcpy(staged_abund.as<uint32_t>() + el, sets[i]->d_abund(), m * 4, hipMemcpyDefault));
      el += m;
    }
  }
  // the staged blocks go back ordered after the copies, which ran on the null stream
  return make_device_set(ctx->device, file_meta_of(a), sizes, windows, nullptr, staged.as<uint64_t>(),
                         std::move(all_names), out, nullptr, counted ? staged_abund.as<uint32_t>() : nullptr);
}

}  // extern "C"
