// The k best references per query: from a reference batch's count tiles to a
// sorted list of k slots per query, on the device.
//
// sks_search_topk joins the query layout with one reference batch's layout
// into packed 64 x 64 count tiles exactly as sks_search does (rows = queries).
// k_topk_update reads the tiles once.  A wavefront owns one query row for the
// whole launch and keeps that query's list in registers, lane l holding slot
// l, sorted, slot 0 the best: the list's last slot is then one readlane away
// (held in scalar registers between inserts), and a candidate enters with one
// ballot (its position) and one wave-wide move up by a lane of the 16-byte
// slot (four DPP moves).  Nearly all cells are zero: a row of a tile whose 64
// counts are all below the threshold costs its load and one ballot.  The
// order (topk_plan.hpp) is strict and total, so the k best are the same set
// whatever the order in which cells arrive; between batches the lists live in
// scratch, 16 bytes a slot, and k_topk_finish expands them into sks_top_hit
// records (pow runs once per slot, not per cell).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "code_objects.hpp"
#include "sks.h"
#include "sks_ani.hpp"
#include "topk.hpp"
#include "wave_prims.hpp"

namespace sks {

namespace {

constexpr int kTB = 256;           // threads per workgroup: 4 wavefronts, a query row each
constexpr int kTWaves = kTB / 64;
constexpr int kTile = 64;
constexpr int kAhead = 4;          // tile rows loaded before the first of them is looked at

static_assert(sizeof(sks_top_hit) == 40, "sks_top_hit is 40 bytes");
static_assert(SKS_TOPK_MAX == kTopkMax && kTopkMax == 64, "a lane per slot");
static_assert(SKS_RANK_QUERY == kRankQuery && SKS_RANK_REF == kRankRef && SKS_RANK_MAX == kRankMax, "rank kinds");

// slot `l` (wave-uniform) of the lanes' slots, in every lane
__device__ __forceinline__ TopkSlot slot_of_lane(const TopkSlot& s, uint32_t l) {
  TopkSlot r;
  r.score = __longlong_as_double((long long)readlane64((uint64_t)__double_as_longlong(s.score), l));
  r.shared = __builtin_amdgcn_readlane(s.shared, (int)l);
  r.ref = (uint32_t)__builtin_amdgcn_readlane((int)s.ref, (int)l);
  return r;
}

// lane l receives lane l - 1's slot (lane 0 its own)
__device__ __forceinline__ TopkSlot slot_before(const TopkSlot& s) {
  TopkSlot r;
  r.score = __longlong_as_double((long long)wave_shr1_64((uint64_t)__double_as_longlong(s.score)));
  r.shared = (int32_t)wave_shr1((uint32_t)s.shared);
  r.ref = wave_shr1(s.ref);
  return r;
}

__global__ __launch_bounds__(kTB) void k_topk_init(TopkSlot* __restrict__ state, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x;
  if (i < n) state[i] = topk_empty();
}

__global__ __launch_bounds__(kTB) void k_topk_update(TopkArgs a, const int32_t* __restrict__ packed,
                                                     uint32_t q_blocks, uint32_t b_blocks, uint32_t ref0,
                                                     uint32_t n_batch, const uint32_t* __restrict__ stat_q,
                                                     const uint32_t* __restrict__ stat_b) {
  if (stat_q[1] | stat_b[1]) return;  // an invalid layout's counts are not counts
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x * kTWaves + wave;  // uniform over the wavefront
  if (q >= a.nq) return;                           // a padding row
  const int32_t q_size = (int32_t)a.q_sizes[q];
  if (q_size == 0) return;  // an empty sketch shares nothing
  const int32_t thr = topk_threshold(a.min_shared);
  const uint32_t k = a.k;
  TopkSlot* list = a.state + (uint64_t)q * k;
  TopkSlot mine = lane < k ? list[lane] : topk_empty();
  TopkSlot worst = slot_of_lane(mine, k - 1);
  bool changed = false;
  // row q % 64 of tile bj * q_blocks + q / 64, this lane's column
  const int32_t* cell = packed + ((uint64_t)(q / kTile) * (kTile * kTile) + (q % kTile) * kTile + lane);
  const uint64_t step = (uint64_t)q_blocks * (kTile * kTile);
  for (uint32_t b0 = 0; b0 < b_blocks; b0 += kAhead) {
    int32_t cnt[kAhead];
#pragma unroll
    for (int i = 0; i < kAhead; ++i) cnt[i] = b0 + i < b_blocks ? cell[(uint64_t)(b0 + i) * step] : 0;
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      const uint32_t col = (b0 + i) * kTile + lane;
      const bool live = cnt[i] >= thr && col < n_batch;  // thr >= 1: no padding column, no block past the batch
      if (!__ballot(live)) continue;
      TopkSlot c = topk_empty();
      bool enters = false;
      if (live) {
        c.ref = ref0 + col;
        c.shared = cnt[i];
        const int32_t r_size = a.rank_kind == kRankQuery ? 0 : (int32_t)a.r_sizes[c.ref];
        c.score = topk_score(cnt[i], topk_denominator(a.rank_kind, q_size, r_size));
        enters = topk_eligible(c, q, thr, a.min_score, a.skip_same_index) && topk_better(c, worst);
      }
      // one by one; a later one may no longer beat the list's last slot
      for (unsigned long long todo = __ballot(enters); todo; todo &= todo - 1) {
        const TopkSlot in = slot_of_lane(c, (uint32_t)__builtin_ctzll(todo));
        if (!topk_better(in, worst)) continue;
        const uint32_t p = (uint32_t)__popcll(__ballot(lane < k && !topk_better(in, mine)));
        mine = topk_lane_after(mine, slot_before(mine), in, lane, p);
        worst = slot_of_lane(mine, k - 1);
        changed = true;
      }
    }
  }
  if (changed && lane < k) list[lane] = mine;
}

__global__ __launch_bounds__(kTB) void k_topk_finish(TopkArgs a, double inv_k, sks_top_hit* __restrict__ hits,
                                                     uint32_t* __restrict__ counts) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x * kTWaves + wave;
  if (q >= a.nq) return;
  const bool slot = lane < a.k;
  const TopkSlot s = slot ? a.state[(uint64_t)q * a.k + lane] : topk_empty();
  const bool filled = slot && !topk_is_empty(s);
  const unsigned long long all = __ballot(filled);
  if (slot) {
    sks_top_hit h{};
    h.query = q;
    h.ref = UINT32_MAX;
    h.rank = lane;
    if (filled) {
      h.ref = s.ref;
      h.shared = s.shared;
      h.query_size = (int32_t)a.q_sizes[q];
      h.ref_size = (int32_t)a.r_sizes[s.ref];
      // the hit filter's function (search.hip): with SKS_RANK_QUERY the same doubles
      h.ani = ani_of(s.shared, topk_denominator(a.rank_kind, h.query_size, h.ref_size), inv_k, &h.score);
    }
    hits[(uint64_t)q * a.k + lane] = h;
  }
  if (counts && lane == 0) counts[q] = (uint32_t)__popcll(all);
}

}  // namespace

hipError_t launch_topk_init(TopkSlot* state, uint32_t nq, uint32_t k, hipStream_t s) {
  const uint64_t n = (uint64_t)nq * k;
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_topk_init, dim3((unsigned)((n + kTB - 1) / kTB)), dim3(kTB), 0, s, state, n);
  return hipGetLastError();
}

hipError_t launch_topk_update(const TopkArgs& a, const int32_t* packed, uint32_t q_blocks, uint32_t b_blocks,
                              uint32_t ref0, uint32_t n_batch, const uint32_t* stat_q, const uint32_t* stat_b,
                              hipStream_t s) {
  if (!a.nq || !b_blocks) return hipSuccess;
  if (a.k == 0 || a.k > kTopkMax || (uint64_t)q_blocks * kTile < a.nq) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_topk_update, dim3((a.nq + kTWaves - 1) / kTWaves), dim3(kTB), 0, s, a, packed, q_blocks,
                     b_blocks, ref0, n_batch, stat_q, stat_b);
  return hipGetLastError();
}

hipError_t launch_topk_finish(const TopkArgs& a, int kmer_num_ones, sks_top_hit* hits, uint32_t* counts,
                              hipStream_t s) {
  if (!a.nq) return hipSuccess;
  if (a.k == 0 || a.k > kTopkMax || kmer_num_ones <= 0) return hipErrorInvalidValue;
  const double inv_k = ((double)1.0) / ((double)kmer_num_ones);
  hipLaunchKernelGGL(k_topk_finish, dim3((a.nq + kTWaves - 1) / kTWaves), dim3(kTB), 0, s, a, inv_k, hits, counts);
  return hipGetLastError();
}

SKS_CODE_OBJECT_HOOK(topk)

}  // namespace sks
