// The k best references per query: selection from count tiles (topk.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "topk_plan.hpp"

struct sks_top_hit;  // include/sks.h

namespace sks {

// What a call's launches share.  state: [nq][k] slots (topk_plan.hpp), each
// query's list sorted, slot 0 the best.
struct TopkArgs {
  TopkSlot* state;
  uint32_t nq, k;
  int rank_kind;         // sks_rank_kind
  double min_score;
  int32_t min_shared;    // as the caller gave it
  bool skip_same_index;
  const uint32_t* q_sizes;
  const uint32_t* r_sizes;  // of the whole reference set (indexed by the global reference)
};

// every slot of every query empty
hipError_t launch_topk_init(TopkSlot* state, uint32_t nq, uint32_t k, hipStream_t s);
// One reference batch: `packed` holds its count tiles [b_blocks][q_blocks][64][64]
// as launch_search_hits reads them (tile bj * q_blocks + qi, rows = queries).
// Cell (q, r) with q < nq and r < n_batch is a candidate {score, count, ref0 + r}
// when it is eligible (topk_eligible); each query's list takes the candidates
// that are before its last slot.  A wavefront per query row, no LDS, no atomics.
// stat_q / stat_b: the two layouts' status words; a non-zero word 1 (invalid
// layout) makes the launch a no-op.
hipError_t launch_topk_update(const TopkArgs& a, const int32_t* packed, uint32_t q_blocks, uint32_t b_blocks,
                              uint32_t ref0, uint32_t n_batch, const uint32_t* stat_q, const uint32_t* stat_b,
                              hipStream_t s);
// hits[q * k + j] from slot j of query q (an empty slot: {q, UINT32_MAX, rank j,
// the rest 0}), counts[q] (or null) the filled slots.
hipError_t launch_topk_finish(const TopkArgs& a, int kmer_num_ones, sks_top_hit* hits, uint32_t* counts,
                              hipStream_t s);

}  // namespace sks
