// The arithmetic of sks_gather (no HIP: tests/cpp/gather_plan_test.cpp runs it on
// any machine, and gather.hip runs the same functions on the device): the
// round's best key, the bitmap of unexplained query elements, the bounded
// search of the membership pass, how candidates' lists map to scoring workgroups
// and how rounds are queued between host waits.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SKS_PLAN_HD __host__ __device__
#else
#define SKS_PLAN_HD
#endif

namespace sks {

// ---- the round's key ---------------------------------------------------------------------
// (count << 32) | (0xffffffff - ref): the largest key is the largest count and,
// among equal counts, the smallest reference index.  0 is "no candidate posted"
// (a posted count is at least 1).  count is in [0, 2^31), ref in [0, 2^32 - 1).
SKS_PLAN_HD inline unsigned long long gather_key(int32_t count, uint32_t ref) {
  return ((unsigned long long)(uint32_t)count << 32) | (unsigned long long)(0xffffffffu - ref);
}
SKS_PLAN_HD inline int32_t gather_key_count(unsigned long long key) { return (int32_t)(uint32_t)(key >> 32); }
SKS_PLAN_HD inline uint32_t gather_key_ref(unsigned long long key) { return 0xffffffffu - (uint32_t)key; }

// thr of the rule: a round must explain at least max(min_shared, 1) elements
SKS_PLAN_HD inline int32_t gather_threshold(int32_t min_shared) { return min_shared < 1 ? 1 : min_shared; }

// ---- the bitmap of unexplained query elements -----------------------------------------------
// Bit p of the bitmap (word p / 32, bit p % 32) is set while query element p is
// unexplained.  The last word's bits at and above q_size stay clear.
SKS_PLAN_HD inline uint32_t gather_bitmap_words(uint32_t q_size) { return (q_size + 31u) / 32u; }
SKS_PLAN_HD inline uint32_t gather_word_of(uint32_t p) { return p >> 5; }
SKS_PLAN_HD inline uint32_t gather_bit_of(uint32_t p) { return 1u << (p & 31u); }
// the initial value of word w (w < gather_bitmap_words(q_size))
SKS_PLAN_HD inline uint32_t gather_word_init(uint32_t w, uint32_t q_size) {
  const uint32_t left = q_size - w * 32u;  // elements from this word on (>= 1)
  return left >= 32u ? 0xffffffffu : (1u << left) - 1u;
}

// ---- the bounded search ------------------------------------------------------------------
// Elements are EW words each, (lo) or (lo, hi), ordered by the 128-bit value:
// hi first.
template <int EW>
SKS_PLAN_HD inline bool gather_less(const uint64_t* a, uint64_t b_lo, uint64_t b_hi) {
  if (EW == 2 && a[1] != b_hi) return a[1] < b_hi;
  return a[0] < b_lo;
}
// The first index i in [lo, hi) with q[i] >= (v_lo, v_hi), or hi: lower_bound of
// the ascending q restricted to the range.
template <int EW>
SKS_PLAN_HD inline uint32_t gather_lower_bound(const uint64_t* q, uint32_t lo, uint32_t hi, uint64_t v_lo,
                                               uint64_t v_hi) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (gather_less<EW>(q + (size_t)mid * EW, v_lo, v_hi)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
template <int EW>
SKS_PLAN_HD inline bool gather_equal(const uint64_t* a, uint64_t b_lo, uint64_t b_hi) {
  return a[0] == b_lo && (EW == 1 || a[1] == b_hi);
}

// ---- candidates, wavefronts and workgroups -----------------------------------------------
// A candidate's position list is scored in chunks of kGatherChunk positions, a
// workgroup (kGatherScoreWaves wavefronts, each counting its share and reducing
// it) per chunk: every candidate gets `per` workgroups, workgroup
// c * per + j taking the chunks j, j + per, ... of candidate c.  `per` is what the
// longest list needs, capped so that the grid stays below 2^30 workgroups.
// The workgroups of a candidate add their counts into one 64-bit word,
// (1 << 32 | count) each: the one that finds gather_blocks_of(len, per) - 1
// arrivals before it holds the candidate's whole count.
constexpr uint32_t kGatherScoreWaves = 4;
constexpr uint32_t kGatherChunk = 2048;
SKS_PLAN_HD inline uint32_t gather_chunks_of(uint32_t len) { return (len + kGatherChunk - 1) / kGatherChunk; }
SKS_PLAN_HD inline uint32_t gather_blocks_per_candidate(uint32_t max_len, uint32_t n_cand) {
  const uint32_t want = gather_chunks_of(max_len), cap = n_cand ? (1u << 30) / n_cand : 1u;
  const uint32_t per = want < cap ? want : cap;
  return per ? per : 1u;
}
SKS_PLAN_HD inline uint32_t gather_candidate_of(uint32_t block, uint32_t per) { return block / per; }
SKS_PLAN_HD inline uint32_t gather_first_chunk_of(uint32_t block, uint32_t per) { return block % per; }
// the workgroups of a candidate that have a chunk to score
SKS_PLAN_HD inline uint32_t gather_blocks_of(uint32_t len, uint32_t per) {
  const uint32_t chunks = gather_chunks_of(len);
  return chunks < per ? chunks : per;
}
SKS_PLAN_HD inline unsigned long long gather_arrival(uint32_t count) { return (1ull << 32) | count; }

// ---- round groups ------------------------------------------------------------------------
// Rounds are queued in groups; the host reads {done, hits} after each.  Every
// round that does not raise `done` reports a candidate that no later round can
// report again, so min(n_cand, max_rounds or n_cand) + 1 rounds always suffice:
// the last of them finds nothing left (or max_rounds reached) and raises done.
constexpr uint32_t kGatherDefaultRounds = 64;  // rounds per host wait: the fastest measured (DESIGN.md "Gather")
inline uint64_t gather_round_limit(uint32_t n_cand, uint32_t max_rounds) {
  const uint64_t most = max_rounds && max_rounds < n_cand ? max_rounds : n_cand;
  return most + 1;
}
// the rounds of the next group, `queued` of `limit` being queued already
inline uint32_t gather_group_rounds(uint32_t rounds_per_wait, uint64_t queued, uint64_t limit) {
  const uint64_t g = rounds_per_wait ? rounds_per_wait : kGatherDefaultRounds;
  const uint64_t left = limit > queued ? limit - queued : 0;
  return (uint32_t)(left < g ? left : g);
}

}  // namespace sks
