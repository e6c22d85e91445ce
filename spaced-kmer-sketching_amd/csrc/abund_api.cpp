// C-ABI implementation (include/sks.h): what is done with a counted sketch set
// (one made by sks_sketch_build_counted, build.cpp) — its totals, the trim by
// abundance and the weighted overlap of sketch pairs.  The host decides every
// refusal; abund.hip does the work; downsample's tail sizes a trimmed set.
#include "sks_ctx.hpp"

using namespace sks;

namespace {

int refuse(const char* who, const std::string& what) { return sks::fail(SKS_E_ARG, std::string(who) + ": " + what); }

const char* const kNoAbund = "the set has no abundance column (sks_sketch_build_counted makes one)";

std::string other_device(int set_device, int ctx_device) {
  return "a set is on device " + std::to_string(set_device) + ", the context on device " + std::to_string(ctx_device);
}

}  // namespace

extern "C" {

int sks_sketch_set_abund_totals(const sks_sketch_set* set, uint64_t* totals) {
  const char* const who = "sks_sketch_set_abund_totals";
  if (!set || (!totals && set->n)) return refuse(who, "null argument");
  if (!set->has_abund()) return refuse(who, kNoAbund);
  const uint32_t n = set->n;
  if (n == 0) return SKS_OK;
  DeviceGuard guard(set->device);
  DevBlock d;
  SKS_TRY(alloc_u64(d, n, nullptr));
  SKS_HIP(sks::abund_totals(set->d_abund(), set->d_starts(), set->d_sizes(), n, d.as<unsigned long long>(), nullptr));
  SKS_HIP(hipMemcpy(totals, d.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost));  // the wait
  d.release();
  return SKS_OK;
}

int sks_sketch_set_abund_trim(sks_ctx* c, const sks_sketch_set* src, uint32_t min_abund, uint32_t max_abund,
                              sks_sketch_set** out) {
  const char* const who = "sks_sketch_set_abund_trim";
  if (out) *out = nullptr;
  if (!c || !src || !out) return refuse(who, "null argument");
  if (!src->has_abund()) return refuse(who, kNoAbund);
  const int ew = src->elem_words;
  if (ew != 1 && ew != 2) return refuse(who, "elements of 1 or 2 words only");
  if (src->device != c->device) return refuse(who, other_device(src->device, c->device));
  const uint32_t n = src->n;

  DeviceGuard guard(c->device);
  hipStream_t st = c->stream;
  // the device writes d_starts and d_sizes; the host sizes follow the read-back below
  SetPtr set;
  const uint64_t none = 0;
  SKS_TRY(make_sketch_set(c->device, ew, src->window, src->mask, src->policy, std::vector<uint32_t>(n, 0),
                          src->windows, src->names, n ? nullptr : &none, st, MetaUpload::kNone, &set));
  if (n == 0) {
    SKS_HIP(set->abund.alloc(sizeof(uint32_t), st));
    *out = set.release();
    return SKS_OK;
  }
  std::vector<uint64_t> chunk_off, dense_off;
  chunk_prefixes(src->sizes, &chunk_off, &dense_off);
  const uint64_t n_chunks = chunk_off[n];
  MetaArena arena(c);
  const size_t o_chunk = arena.add(chunk_off);
  SKS_TRY(arena.upload());
  SKS_TRY(reserve_chunk_counters(c, n_chunks));
  SKS_TRY(reserve_cols(c, {0}, filter_bitmap_words(n_chunks)));  // one bit per source element

  const AbundTrimArgs a{src->d_data(), src->d_abund(), src->d_starts(), src->d_sizes(), arena.ptr(o_chunk),
                        n,             min_abund,      max_abund};
  SKS_HIP(sks::abund_trim_mark(a, n_chunks, col(c, 0), chunk_counts(c), st));
  // the call's one wait
  SKS_TRY(size_set_from_counts(c, who, "a trimmed sketch is larger than its source", n_chunks, a.chunk_off,
                               src->sizes.data(), set.get()));
  uint64_t total = 0;
  for (uint32_t v : set->sizes) total += v;
  SKS_HIP(set->abund.alloc(std::max<uint64_t>(total, 1) * sizeof(uint32_t), st));
  SKS_HIP(sks::abund_trim_scatter(a, ew, n_chunks, col(c, 0), chunk_offs(c), set->d_data(), set->d_abund(), st));
  *out = set.release();
  return SKS_OK;
}

int sks_abund_pairs(sks_ctx* c, const sks_sketch_set* samples, const sks_sketch_set* refs, const int32_t* d_a,
                    const int32_t* d_b, uint64_t n_pairs, int32_t* d_shared, uint64_t* d_weight) {
  const char* const who = "sks_abund_pairs";
  if (!c) return refuse(who, "null ctx");
  if (!samples || !refs) return refuse(who, "null argument");
  if (n_pairs && (!d_a || !d_b || !d_shared || !d_weight)) return refuse(who, "null argument");
  if (!samples->has_abund()) return refuse(who, std::string("samples: ") + kNoAbund);
  sks_sketch_info info{};
  int k = 0;
  SKS_TRY(search_sets_compatible(c, who, samples, refs, &info, &k,
                                 "the sets' policy kind must be SKS_FRAC_MOD (a bottom-s sketch samples a hash range "
                                 "of its own)"));
  if (info.elem_words != 1 && info.elem_words != 2) return refuse(who, "elements of 1 or 2 words only");
  if (n_pairs == 0) return SKS_OK;
  DeviceGuard guard(c->device);
  AbundPairsArgs a{};
  a.s_data = samples->d_data();
  a.s_starts = samples->d_starts();
  a.s_sizes = samples->d_sizes();
  a.s_abund = samples->d_abund();
  a.s_n = samples->n;
  a.r_data = refs->d_data();
  a.r_starts = refs->d_starts();
  a.r_sizes = refs->d_sizes();
  a.r_n = refs->n;
  a.d_a = d_a;
  a.d_b = d_b;
  a.n_pairs = n_pairs;
  a.shared = d_shared;
  a.weight = reinterpret_cast<unsigned long long*>(d_weight);
  SKS_HIP(sks::abund_pairs(a, info.elem_words, c->stream));
  return SKS_OK;
}

}  // extern "C"
