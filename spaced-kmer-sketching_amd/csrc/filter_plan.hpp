// The arithmetic of sks_sketch_set_filter (no HIP: tests/cpp/filter_plan_test.cpp
// runs it on any machine, and filter.hip runs the same functions on the device):
// the keep rule, the range of an ascending filter sketch that a chunk of an
// ascending source sketch can meet (its bracket), the 64-ary narrowing that
// finds the bracket's two ends with a wavefront, the bitmap of kept elements and
// the choice between the staged and the direct search.
#pragma once
#include <cstddef>
#include <cstdint>

#include "gather_plan.hpp"  // SKS_PLAN_HD, gather_less, gather_lower_bound, gather_equal

// The bytes of LDS that hold a chunk's bracket on the staged path (DESIGN.md
// "Filtering a sketch set" has the measurement; a -D overrides it for A/B builds).
#ifndef SKS_FILTER_STAGE_BYTES
#define SKS_FILTER_STAGE_BYTES 16384
#endif

namespace sks {

constexpr uint32_t kFilterChunk = 1024;  // consecutive elements of one source sketch per workgroup
constexpr uint32_t kFilterStageBytes = SKS_FILTER_STAGE_BYTES;
constexpr uint64_t kFilterNone = ~0ull;  // the filter size of a sketch that is copied unchanged

// ---- the keep rule -----------------------------------------------------------------------
// sks_filter_kind (sks.h; filter_api.cpp checks the values): SUBTRACT keeps x
// iff x is not in the filter sketch, INTERSECT iff it is.
constexpr int kFilterSubtract = 0, kFilterIntersect = 1;
SKS_PLAN_HD inline bool filter_keeps(bool found, int kind) { return found != (kind == kFilterSubtract); }

// ---- the bitmap of kept elements ---------------------------------------------------------
// Chunk c owns kFilterChunkWords words from word c * kFilterChunkWords; element
// e of the chunk (e < kFilterChunk) is bit e % 64 of its word e / 64.  A
// workgroup of 256 threads reads element s * 256 + thread in its stride s, so
// the ballot of wavefront v in stride s is exactly word 4 s + v.
constexpr uint32_t kFilterChunkWords = kFilterChunk / 64;
SKS_PLAN_HD inline uint32_t filter_word_of(uint32_t e) { return e >> 6; }
SKS_PLAN_HD inline uint32_t filter_bit_of(uint32_t e) { return e & 63u; }
SKS_PLAN_HD inline uint32_t filter_ballot_word(uint32_t stride, uint32_t wave) { return 4u * stride + wave; }
SKS_PLAN_HD inline uint64_t filter_bitmap_words(uint64_t n_chunks) { return n_chunks * kFilterChunkWords; }

// ---- staged or direct --------------------------------------------------------------------
// A bracket of at most filter_stage_elems(ew) elements is copied into LDS and
// searched there; a longer one is searched where it lies.
SKS_PLAN_HD inline uint32_t filter_stage_elems(int elem_words) {
  return kFilterStageBytes / (8u * (uint32_t)elem_words);
}
SKS_PLAN_HD inline bool filter_staged(uint32_t range_len, int elem_words, bool no_stage) {
  return !no_stage && range_len <= filter_stage_elems(elem_words);
}

// ---- the 64-ary narrowing ----------------------------------------------------------------
// Finds the first index in [lo, hi] of an ascending array at which a monotone
// predicate (true, ..., true, false, ..., false) turns false; hi if it never
// does.  A step probes 64 indices, one per lane, and the number of lanes whose
// probe is true gives the next, at least 65 times shorter, range.  While more
// than 64 indices are left the probes are spread evenly (all distinct, all
// inside the range); the last step probes lo, lo + 1, ... and ends the search.
struct FilterRange {
  uint32_t lo, hi;
};
// the index lane `lane` probes, or `hi` (nothing to probe: the lane reports false)
SKS_PLAN_HD inline uint32_t filter_probe(FilterRange r, uint32_t lane) {
  const uint32_t len = r.hi - r.lo;
  if (len <= 64u) return lane < len ? r.lo + lane : r.hi;
  return r.lo + (uint32_t)(((uint64_t)len * (lane + 1u)) / 65u);
}
// the range after a step in which the probes of the first `n_true` lanes were
// true; *done: lo is the answer
SKS_PLAN_HD inline FilterRange filter_narrow(FilterRange r, uint32_t n_true, bool* done) {
  const uint32_t len = r.hi - r.lo;
  if (len <= 64u) {
    *done = true;
    return {r.lo + n_true, r.lo + n_true};
  }
  *done = false;
  const uint32_t lo = n_true ? filter_probe(r, n_true - 1u) + 1u : r.lo;
  const uint32_t hi = n_true < 64u ? filter_probe(r, n_true) : r.hi;
  return {lo, hi};
}

// ---- the bracket -------------------------------------------------------------------------
// Elements are EW words each, (lo) or (lo, hi), ordered by the 128-bit value.
template <int EW>
SKS_PLAN_HD inline bool filter_below(const uint64_t* a, uint64_t v_lo, uint64_t v_hi) {  // a < v
  return gather_less<EW>(a, v_lo, v_hi);
}
template <int EW>
SKS_PLAN_HD inline bool filter_not_above(const uint64_t* a, uint64_t v_lo, uint64_t v_hi) {  // a <= v
  if (EW == 2 && a[1] != v_hi) return a[1] < v_hi;
  return a[0] <= v_lo;
}
// The filter elements a chunk whose first element is (first) and whose last is
// (last) can meet: [lower_bound(first), upper_bound(last)) of the ascending
// f[0 .. n).  Empty (lo == hi) for an empty filter and when every filter element
// lies below the chunk, above it, or in a gap of it.  One lane's search; the
// kernel finds the same two ends with filter_probe / filter_narrow.
template <int EW>
SKS_PLAN_HD inline FilterRange filter_bracket(const uint64_t* f, uint32_t n, uint64_t first_lo, uint64_t first_hi,
                                              uint64_t last_lo, uint64_t last_hi) {
  const uint32_t b = gather_lower_bound<EW>(f, 0, n, first_lo, first_hi);
  uint32_t lo = b, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (filter_not_above<EW>(f + (size_t)mid * EW, last_lo, last_hi)) lo = mid + 1;
    else hi = mid;
  }
  return {b, lo};
}

// Whether (v) is one of q[lo .. hi) (ascending): the search of both paths.
template <int EW>
SKS_PLAN_HD inline bool filter_member(const uint64_t* q, uint32_t lo, uint32_t hi, uint64_t v_lo, uint64_t v_hi) {
  const uint32_t i = gather_lower_bound<EW>(q, lo, hi, v_lo, v_hi);
  return i < hi && gather_equal<EW>(q + (size_t)i * EW, v_lo, v_hi);
}

}  // namespace sks
