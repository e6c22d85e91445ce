// The arithmetic of sks_search_topk (no HIP: tests/cpp/topk_plan_test.cpp runs it
// on any machine, and topk.hip runs the same functions on the device): a list
// slot and its "empty" value, the strict total order of candidates, the score's
// denominator per rank kind, eligibility, and the update of a sorted list by one
// candidate, lane by lane as the kernel does it and as a scalar model.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SKS_PLAN_HD __host__ __device__
#else
#define SKS_PLAN_HD
#endif

namespace sks {

constexpr uint32_t kTopkMax = 64;  // SKS_TOPK_MAX: one lane of a wavefront per slot

// the values of sks_rank_kind (include/sks.h)
constexpr int kRankQuery = 0, kRankRef = 1, kRankMax = 2;

// ---- a slot ----------------------------------------------------------------------------
// 16 bytes of state per (query, slot).  An empty slot has ref 0xffffffff (no
// reference has that index: a set holds fewer than 2^32 - 1 sketches) and a
// score below every candidate's, so the order below puts it after all of them.
struct alignas(16) TopkSlot {
  double score;
  int32_t shared;
  uint32_t ref;
};
static_assert(sizeof(TopkSlot) == 16, "a slot is one 16-byte word");

constexpr uint32_t kTopkNoRef = 0xffffffffu;
SKS_PLAN_HD inline TopkSlot topk_empty() { return TopkSlot{-1.0, 0, kTopkNoRef}; }
SKS_PLAN_HD inline bool topk_is_empty(const TopkSlot& s) { return s.ref == kTopkNoRef; }

// ---- the order -------------------------------------------------------------------------
// a before b: the larger score, then the larger shared, then the smaller ref.
// Strict and total over slots of distinct refs; two equal slots are neither
// before the other.
SKS_PLAN_HD inline bool topk_better(const TopkSlot& a, const TopkSlot& b) {
  if (a.score != b.score) return a.score > b.score;
  if (a.shared != b.shared) return a.shared > b.shared;
  return a.ref < b.ref;
}

// ---- the score -------------------------------------------------------------------------
// |Q_q|, |R_r| or the smaller of them
SKS_PLAN_HD inline int32_t topk_denominator(int rank_kind, int32_t q_size, int32_t r_size) {
  if (rank_kind == kRankQuery) return q_size;
  if (rank_kind == kRankRef) return r_size;
  return q_size < r_size ? q_size : r_size;
}
// the expression of containment_of (sks_ani.hpp): one double division
SKS_PLAN_HD inline double topk_score(int32_t shared, int32_t denominator) {
  return shared == 0 ? 0.0 : (double)shared / (double)denominator;
}
// thr of the rule: a listed pair shares at least max(min_shared, 1) elements
SKS_PLAN_HD inline int32_t topk_threshold(int32_t min_shared) { return min_shared < 1 ? 1 : min_shared; }
SKS_PLAN_HD inline bool topk_eligible(const TopkSlot& c, uint32_t query, int32_t thr, double min_score,
                                      bool skip_same_index) {
  return c.shared >= thr && c.score >= min_score && !(skip_same_index && c.ref == query);
}

// ---- the list update -------------------------------------------------------------------
// A query's list is kept sorted, slot 0 the best, empty slots last.  A candidate
// c enters iff it is before the last slot, list[k - 1]; it then takes position
//   p = the number of slots s < k with !topk_better(c, list[s])
// (those form a prefix of a sorted list, and p < k), slots p .. k - 2 move one
// down and the old list[k - 1] leaves.  Slot `lane` of the new list, from its
// own old value and the old value of the slot before it:
SKS_PLAN_HD inline TopkSlot topk_lane_after(const TopkSlot& mine, const TopkSlot& before, const TopkSlot& c,
                                            uint32_t lane, uint32_t p) {
  return lane < p ? mine : lane == p ? c : before;
}

// The scalar model of the kernel's update: list[0 .. k) sorted, one candidate.
inline void topk_list_update(TopkSlot* list, uint32_t k, const TopkSlot& c) {
  if (!topk_better(c, list[k - 1])) return;
  uint32_t p = 0;
  for (uint32_t s = 0; s < k; ++s) p += topk_better(c, list[s]) ? 0u : 1u;
  for (uint32_t lane = k; lane-- > 0;)  // from the end, so list[lane - 1] is still the old value
    list[lane] = topk_lane_after(list[lane], lane ? list[lane - 1] : list[lane], c, lane, p);
}

}  // namespace sks
