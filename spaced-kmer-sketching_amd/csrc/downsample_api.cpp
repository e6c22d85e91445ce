// C-ABI implementation (include/sks.h): sks_sketch_set_downsample — a coarser
// copy of a device sketch set (FracMinHash 1/c -> 1/c', bottom-s -> bottom-s')
// made from the set's own elements by the filter kernels of downsample.hip.
// downsample_arrays, the work after the argument checks, also cuts the bottom-s
// sketches of sks_sketch_set_merge (merge_api.cpp); the chunk prefixes and the
// sizing tail also serve sks_sketch_set_filter (filter_api.cpp).
#include <numeric>

#include "sks_ctx.hpp"
#include "sks_hash.hpp"

using namespace sks;

int sks::reserve_chunk_counters(sks_ctx* c, uint64_t n_chunks) {
  SKS_HIP(c->flag.reserve((n_chunks + 1) * sizeof(uint32_t)));
  SKS_HIP(c->pos.reserve((n_chunks + 1) * sizeof(uint64_t)));
  return SKS_OK;
}

void sks::chunk_prefixes(const std::vector<uint32_t>& sizes, std::vector<uint64_t>* chunk_off,
                         std::vector<uint64_t>* dense_off) {
  const size_t n = sizes.size();
  chunk_off->assign(n + 1, 0);
  dense_off->assign(n + 1, 0);
  for (size_t g = 0; g < n; ++g) {
    (*chunk_off)[g + 1] = (*chunk_off)[g] + (sizes[g] + (uint64_t)kDownsampleChunk - 1) / kDownsampleChunk;
    (*dense_off)[g + 1] = (*dense_off)[g] + sizes[g];
  }
}

int sks::size_set_from_counts(sks_ctx* c, const char* who, const char* too_large, uint64_t n_chunks,
                              const uint64_t* d_chunk_off, const uint32_t* bound, sks_sketch_set* set) {
  hipStream_t st = c->stream;
  const uint32_t n = set->n;
  SKS_HIP(sks::downsample_offsets(chunk_counts(c), n_chunks, chunk_offs(c), d_chunk_off, n, set->d_starts(),
                                  set->d_sizes(), c->tmp, st));
  // the wait: the new sizes size the new set's data array exactly
  std::vector<uint32_t> sizes(n, 0);
  SKS_HIP(sks::pinned_d2h(sizes.data(), set->d_sizes(), n * sizeof(uint32_t), st));
  uint64_t total = 0;
  for (uint32_t g = 0; g < n; ++g) {
    if (sizes[g] > bound[g]) return sks::fail(SKS_E_HIP, std::string(who) + ": " + too_large);
    set->starts[g] = total;
    total += sizes[g];
  }
  SKS_TRY(alloc_u64(set->data, total * set->elem_words, st));
  set->sizes = std::move(sizes);
  return SKS_OK;
}

int sks::downsample_arrays(sks_ctx* c, const char* who, const uint64_t* d_data, const uint64_t* d_starts,
                           const uint32_t* d_sizes, const std::vector<uint32_t>& src_sizes, const sks_sketch_set& like,
                           uint64_t param, SetPtr* out) {
  const sks_policy& pol = like.policy;
  const bool bottom = pol.kind == SKS_BOTTOM_S;
  hipStream_t st = c->stream;
  const uint32_t n = (uint32_t)src_sizes.size();
  const int ew = like.elem_words;

  // chunks and elements before each sketch
  std::vector<uint64_t> chunk_off, dense_off;
  chunk_prefixes(src_sizes, &chunk_off, &dense_off);
  uint64_t max_len = 0;
  bool selects = false;  // bottom-s: a sketch holds more than `param` elements
  for (uint32_t g = 0; g < n; ++g) {
    const uint64_t sz = src_sizes[g];
    max_len = std::max(max_len, sz);
    selects = selects || sz > param;
  }
  const uint64_t n_chunks = chunk_off[n], T = dense_off[n];
  const int mode = !bottom ? (param == pol.param ? kDownsampleAll : kDownsampleFrac)
                           : (selects ? kDownsampleFlag : kDownsampleAll);

  // the device writes d_starts and d_sizes; the host sizes follow the read-back below
  sks_policy coarser = pol;
  coarser.param = param;
  SetPtr set;
  SKS_TRY(make_sketch_set(c->device, ew, like.window, like.mask, coarser, std::vector<uint32_t>(n, 0), like.windows,
                          like.names, nullptr, st, MetaUpload::kNone, &set));

  MetaArena arena(c);
  const size_t o_chunk = arena.add(chunk_off), o_dense = arena.add(dense_off);
  SKS_TRY(arena.upload());
  SKS_TRY(reserve_chunk_counters(c, n_chunks));

  DownsampleArgs a{};
  a.data = d_data;
  a.starts = d_starts;
  a.sizes = d_sizes;
  a.chunk_off = arena.ptr(o_chunk);
  a.dense_off = arena.ptr(o_dense);
  a.kconst = sks::fmh_const(like.mask[0], like.mask[1], like.window, pol.nonce, pol.flavour);
  if (mode == kDownsampleFrac) {
    const sks::DivTest dt = sks::make_div_test(param);
    a.low_mask = dt.low_mask;
    a.high_mask = dt.rot > 32 ? (uint32_t)((1ull << (dt.rot - 32)) - 1) : 0u;
    a.dinv = dt.dinv;
    a.dlim = dt.lim;
  }
  if (mode == kDownsampleFlag) {
    // (fmh, index) sorted by fmh within each sketch: the sort is stable and the
    // elements ascend by k-mer, so a sketch's first `param` entries are its
    // smallest by (fmh, k-mer), ties at the last fmh taken in k-mer order
    SKS_TRY(reserve_cols(c, {0, 1, 2, 3, 4}, T + 1));
    uint32_t* d_keep = reinterpret_cast<uint32_t*>(col(c, 2));
    SKS_HIP(sks::downsample_fmh(a, ew, pol.flavour, n, max_len, col(c, 0), col(c, 1), st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 0), col(c, 3), col(c, 1), col(c, 4), T, dense_off, a.dense_off, 64, c->tmp,
                                st));
    SKS_HIP(hipMemsetAsync(d_keep, 0, T * sizeof(uint32_t), st));
    SKS_HIP(sks::downsample_mark(a, n, param, max_len, col(c, 4), d_keep, st));
    a.keep_flag = d_keep;
  }

  SKS_HIP(sks::downsample_count(a, ew, pol.flavour, mode, n, max_len, chunk_counts(c), st));
  // the call's one wait
  SKS_TRY(size_set_from_counts(c, who, "a filtered sketch is larger than its source", n_chunks, a.chunk_off,
                               src_sizes.data(), set.get()));
  SKS_HIP(sks::downsample_scatter(a, ew, pol.flavour, mode, n, max_len, chunk_offs(c), set->d_data(), st));
  *out = std::move(set);
  return SKS_OK;
}

extern "C" int sks_sketch_set_downsample(sks_ctx* c, const sks_sketch_set* src, uint64_t param,
                                         sks_sketch_set** out) {
  if (out) *out = nullptr;
  if (!c || !src || !out) return sks::fail(SKS_E_ARG, "sks_sketch_set_downsample: null argument");
  if (param == 0) return sks::fail(SKS_E_ARG, "sks_sketch_set_downsample: policy param must be > 0");
  if (src->device != c->device)
    return sks::fail(SKS_E_ARG, "sks_sketch_set_downsample: the set is on device " + std::to_string(src->device) +
                                    ", the context on device " + std::to_string(c->device));
  const sks_policy& pol = src->policy;
  const bool bottom = pol.kind == SKS_BOTTOM_S;
  if (!bottom && pol.kind != SKS_FRAC_MOD)
    return sks::fail(SKS_E_ARG, "sks_sketch_set_downsample: unknown policy kind");
  if (pol.flavour != 0 && pol.flavour != 1)
    return sks::fail(SKS_E_ARG, "sks_sketch_set_downsample: unknown hash flavour");
  if (src->elem_words != 1 && src->elem_words != 2)
    return sks::fail(SKS_E_ARG, "sks_sketch_set_downsample: elements of 1 or 2 words only");
  if (!bottom && (pol.param == 0 || param % pol.param != 0))
    return sks::fail(SKS_E_ARG, "sks_sketch_set_downsample: policy param " + std::to_string(param) +
                                    " is not a multiple of the set's " + std::to_string(pol.param) +
                                    " (a FracMinHash sketch can only be made coarser)");
  if (bottom && param > pol.param)
    return sks::fail(SKS_E_ARG, "sks_sketch_set_downsample: policy param " + std::to_string(param) +
                                    " is larger than the set's " + std::to_string(pol.param) +
                                    " (a bottom-s sketch can only be made smaller)");

  DeviceGuard guard(c->device);
  SetPtr set;
  SKS_TRY(downsample_arrays(c, "sks_sketch_set_downsample", src->d_data(), src->d_starts(), src->d_sizes(), src->sizes,
                            *src, param, &set));
  *out = set.release();
  return SKS_OK;
}
