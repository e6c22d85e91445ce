// C-ABI implementation (include/sks.h): sks_sketch_set_filter — every sketch of
// a device sketch set without (SUBTRACT) or within (INTERSECT) a sketch of a
// second set.  An element is a masked canonical k-mer kept on its own hash, so
// at one FracMinHash scale the difference and the intersection of two sketches
// are the sketches of the difference and the intersection.  The host decides
// every refusal and uploads the chunk prefixes and each sketch's filter range
// once; filter.hip marks and scatters, downsample's tail sizes the new set.
#include <cstdlib>

#include "sks_ctx.hpp"

using namespace sks;

static_assert(SKS_FILTER_SUBTRACT == kFilterSubtract && SKS_FILTER_INTERSECT == kFilterIntersect,
              "filter_plan.hpp restates sks_filter_kind");

namespace {

const char* const kWho = "sks_sketch_set_filter";

int refuse(const std::string& what) { return sks::fail(SKS_E_ARG, std::string(kWho) + ": " + what); }

}  // namespace

extern "C" int sks_sketch_set_filter(sks_ctx* c, const sks_sketch_set* src, const sks_sketch_set* filters,
                                     const uint32_t* filter_of, int kind, sks_sketch_set** out) {
  if (out) *out = nullptr;
  if (!c || !src || !filters || !out) return refuse("null argument");
  if (kind != SKS_FILTER_SUBTRACT && kind != SKS_FILTER_INTERSECT)
    return refuse("unknown filter kind " + std::to_string(kind));
  if (const char* f = set_differs_in(info_of(*src), info_of(*filters), ParamRule::kAlways))
    return refuse(std::string("the set and the filters differ in ") + f);
  if (src->policy.kind != SKS_FRAC_MOD)
    return refuse("policy kind: FracMinHash sets only (a bottom-s sketch of a difference or an intersection "
                  "is not a part of the bottom-s sketches)");
  const int ew = src->elem_words;
  if (ew != 1 && ew != 2) return refuse("elements of 1 or 2 words only");
  if (src->device != c->device || filters->device != c->device)
    return refuse("a set is on device " + std::to_string(src->device != c->device ? src->device : filters->device) +
                  ", the context on device " + std::to_string(c->device));
  if (!filter_of && filters->n != 1)
    return refuse("a null filter_of needs filters of exactly one sketch (it holds " + std::to_string(filters->n) +
                  ")");
  const uint32_t n = src->n;
  for (uint32_t i = 0; filter_of && i < n; ++i)
    if (filter_of[i] != UINT32_MAX && filter_of[i] >= filters->n)
      return refuse("filter_of[" + std::to_string(i) + "] = " + std::to_string(filter_of[i]) +
                    " is neither UINT32_MAX nor below the filters' " + std::to_string(filters->n) + " sketches");
  const bool no_stage = getenv("SKS_FILTER_NO_STAGE") != nullptr;

  DeviceGuard guard(c->device);
  hipStream_t st = c->stream;
  // the device writes d_starts and d_sizes; the host sizes follow the read-back below
  SetPtr set;
  const uint64_t none = 0;
  SKS_TRY(make_sketch_set(c->device, ew, src->window, src->mask, src->policy, std::vector<uint32_t>(n, 0),
                          src->windows, src->names, n ? nullptr : &none, st, MetaUpload::kNone, &set));
  if (n == 0) {
    *out = set.release();
    return SKS_OK;
  }

  std::vector<uint64_t> chunk_off, dense_off, frange(2 * (size_t)n, 0);
  chunk_prefixes(src->sizes, &chunk_off, &dense_off);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t f = filter_of ? filter_of[i] : 0u;
    frange[2 * (size_t)i] = f == UINT32_MAX ? 0 : filters->starts[f];
    frange[2 * (size_t)i + 1] = f == UINT32_MAX ? kFilterNone : filters->sizes[f];
  }
  const uint64_t n_chunks = chunk_off[n];
  MetaArena arena(c);
  const size_t o_chunk = arena.add(chunk_off), o_dense = arena.add(dense_off), o_range = arena.add(frange);
  SKS_TRY(arena.upload());
  SKS_TRY(reserve_chunk_counters(c, n_chunks));
  SKS_TRY(reserve_cols(c, {0}, filter_bitmap_words(n_chunks)));  // one bit per source element

  FilterArgs a{};
  a.data = src->d_data();
  a.starts = src->d_starts();
  a.chunk_off = arena.ptr(o_chunk);
  a.dense_off = arena.ptr(o_dense);
  a.fdata = filters->d_data();
  a.frange = arena.ptr(o_range);
  a.n = n;
  a.kind = kind;
  a.no_stage = no_stage ? 1 : 0;
  SKS_HIP(sks::filter_mark(a, ew, n_chunks, col(c, 0), chunk_counts(c), st));
  // the call's one wait
  SKS_TRY(size_set_from_counts(c, kWho, "a filtered sketch is larger than its source", n_chunks, a.chunk_off,
                               src->sizes.data(), set.get()));
  SKS_HIP(sks::filter_scatter(a, ew, n_chunks, col(c, 0), chunk_offs(c), set->d_data(), st));
  *out = set.release();
  return SKS_OK;
}
