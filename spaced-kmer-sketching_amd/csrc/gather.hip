// Greedy min-set cover of one query sketch Q by reference sketches, on the
// device (sks_gather).  Neither phase uses the join layout: there is one large
// query and many references, not 64 x 64 blocks of sketches.
//
// Membership, once per call.  Q and every reference are ascending, so a
// wavefront that takes 64 consecutive elements of one reference first bounds
// the range of Q they can fall in (lower bounds of its first and last element,
// searched from where the wavefront's previous 64 ended) and every other lane
// searches inside that range only (gather_plan.hpp).  A workgroup per
// reference walks it in tiles of 256 elements and compacts the positions found
// in tile order, so each reference's list of positions in Q comes out
// ascending with no sort, at off[r] = the sizes before r: O(r_total) words.
//
// Rounds.  A bitmap of |Q| bits holds what is still unexplained.  k_gather_score
// counts each live candidate's positions whose bit is set, a workgroup per chunk
// of 2048 positions (one wavefront per candidate walked a 25 000-position list in
// 390 dependent steps and made a round cost 170 us); the candidate's last
// workgroup posts (count << 32 | ~ref) with one 64-bit atomicMax;
// k_gather_take, one workgroup, reads the key, appends the hit and clears the
// winner's bits with atomicAnd (lanes share words).  Counts never grow, so a
// candidate that fell below the threshold is skipped from then on.  Every
// kernel returns at once when the done flag is up, which lets the host queue
// rounds in groups and wait once per group.  The two kernels of a round are
// separate launches on one stream: what one wrote (plain stores and atomics) is
// visible to the next at the kernel boundary.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "code_objects.hpp"
#include "gather.hpp"
#include "gather_plan.hpp"
#include "sks.h"
#include "sks_ani.hpp"
#include "wave_prims.hpp"

namespace sks {

namespace {

constexpr int kGB = 256;    // threads per workgroup of the membership and scoring kernels: 4 wavefronts
constexpr int kWide = 1024;  // threads of the single-workgroup kernels (scans, the take)
static_assert(kGatherScoreWaves == (uint32_t)(kGB / 64) && kGatherChunk % kGB == 0, "a scoring workgroup walks whole chunks");
static_assert(sizeof(sks_gather_hit) == 32, "sks_gather_hit is two 16-byte words per record");

// off[r] = the sizes before r, by one workgroup walking the sizes in chunks
// (64-bit sums: a wrong size cannot wrap the check against r_total)
__global__ __launch_bounds__(kWide) void k_gather_offsets(const uint32_t* __restrict__ r_sizes, uint32_t r_n,
                                                          uint64_t r_total, uint32_t* __restrict__ off,
                                                          uint32_t* __restrict__ state) {
  __shared__ uint64_t wsum[kWide / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry = 0;  // the sizes before this chunk (uniform)
  for (uint32_t base = 0; base < r_n; base += kWide) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = i < r_n ? r_sizes[i] : 0;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWide / 64; ++w) {
      const uint64_t t = wsum[w];
      before += w < wave ? t : 0ull;
      all += t;
    }
    const uint64_t at = carry + before + inc - v;
    if (i < r_n) off[i] = at > 0xffffffffull ? 0xffffffffu : (uint32_t)at;
    carry += all;
    __syncthreads();  // wsum is written again
  }
  if (threadIdx.x == 0 && carry > r_total) state[kGatherBadTotal] = 1;
}

template <int EW>
__global__ __launch_bounds__(kGB) void k_gather_member(const uint64_t* __restrict__ q, uint32_t q_size,
                                                       const uint64_t* __restrict__ r_data,
                                                       const uint64_t* __restrict__ r_starts,
                                                       const uint32_t* __restrict__ r_sizes,
                                                       const uint32_t* __restrict__ off, uint32_t* __restrict__ list,
                                                       int32_t* __restrict__ shared,
                                                       const uint32_t* __restrict__ state) {
  __shared__ uint32_t wsum[kGB / 64];
  if (state[kGatherBadTotal]) return;  // off[] does not fit the list: write nothing
  const uint32_t r = blockIdx.x, size = r_sizes[r];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t* e = r_data + r_starts[r] * EW;
  uint32_t* out = list + off[r];  // off[r] + size <= r_total (k_gather_offsets)
  uint32_t found_before = 0;      // positions written so far (uniform over the workgroup)
  uint32_t floor = 0;             // lower bound in Q of this wavefront's next elements
  for (uint32_t tile = 0; tile < size; tile += kGB) {
    const uint32_t first = tile + wave * 64;                           // this wavefront's 64 elements
    const uint32_t in_wave = first < size ? (size - first < 64 ? size - first : 64) : 0;
    const bool valid = (uint32_t)lane < in_wave;
    uint64_t v_lo = 0, v_hi = 0;
    if (valid) {
      v_lo = e[(uint64_t)(first + lane) * EW];
      if (EW == 2) v_hi = e[(uint64_t)(first + lane) * EW + 1];
    }
    uint32_t pos = q_size;
    bool found = false;
    if (in_wave) {  // uniform over the wavefront
      const int last_lane = (int)in_wave - 1;
      const bool edge = lane == 0 || lane == last_lane;
      uint32_t b = 0;
      if (edge) b = gather_lower_bound<EW>(q, floor, q_size, v_lo, v_hi);
      const uint32_t lo = (uint32_t)__shfl((int)b, 0, 64), hi = (uint32_t)__shfl((int)b, last_lane, 64);
      if (valid) {
        // an inner element lies strictly between the edges, so its lower bound is in [lo, hi]
        pos = edge ? b : gather_lower_bound<EW>(q, lo, hi, v_lo, v_hi);
        found = pos < q_size && gather_equal<EW>(q + (uint64_t)pos * EW, v_lo, v_hi);
      }
      floor = hi;
    }
    uint32_t total;
    const uint32_t rank = block_rank<kGB / 64>(found, wsum, &total);
    if (found) out[found_before + rank] = pos;
    found_before += total;
    __syncthreads();  // wsum is written again
  }
  if (threadIdx.x == 0) shared[r] = (int32_t)found_before;
}

// the candidates in index order, and the scalar round state
__global__ __launch_bounds__(kWide) void k_gather_cands(const int32_t* __restrict__ shared, uint32_t r_n, int32_t thr,
                                                        uint32_t q_size, uint32_t* __restrict__ cand,
                                                        int32_t* __restrict__ last,
                                                        unsigned long long* __restrict__ best,
                                                        uint32_t* __restrict__ state) {
  __shared__ uint32_t wsum[kWide / 64];
  __shared__ uint32_t longest;
  if (threadIdx.x == 0) longest = 0;
  __syncthreads();
  uint32_t n_cand = 0, mine = 0;  // candidates so far (uniform); this thread's share of the list total
  uint32_t my_longest = 0;
  if (!state[kGatherBadTotal])
    for (uint32_t base = 0; base < r_n; base += kWide) {
      const uint32_t i = base + threadIdx.x;
      const int32_t sh = i < r_n ? shared[i] : 0;
      const bool is = i < r_n && sh >= thr;
      uint32_t total;
      const uint32_t rank = block_rank<kWide / 64>(is, wsum, &total);
      if (is) {
        cand[n_cand + rank] = i;
        last[n_cand + rank] = sh;
        mine += (uint32_t)sh;
        my_longest = my_longest > (uint32_t)sh ? my_longest : (uint32_t)sh;
      }
      n_cand += total;
      __syncthreads();  // wsum is written again
    }
  if (my_longest) atomicMax(&longest, my_longest);
  uint32_t list_total;
  (void)block_excl_scan<kWide / 64>(mine, wsum, &list_total);  // its barrier also orders `longest`
  if (threadIdx.x == 0) {
    state[kGatherDone] = 0;
    state[kGatherHits] = 0;
    state[kGatherRemaining] = q_size;
    state[kGatherCands] = n_cand;
    state[kGatherListTotal] = list_total;
    state[kGatherLongest] = longest;
    best[0] = 0;
    best[1] = 0;
  }
}

__global__ __launch_bounds__(kGB) void k_gather_bitmap(uint32_t* __restrict__ bitmap, uint32_t words,
                                                       uint32_t q_size) {
  const uint32_t w = blockIdx.x * kGB + threadIdx.x;
  if (w < words) bitmap[w] = gather_word_init(w, q_size);
}

// A workgroup per (candidate, chunk of its list): kGatherChunk / kGB positions a
// thread, the list loads and the bitmap loads of a chunk issued together.  The
// workgroups of a candidate meet in arrive[c] (gather_plan.hpp); the last one
// holds the whole count, stores it and posts the key.  last[c] is read by every
// workgroup of c before it arrives and written only after all have, so the
// test below sees the previous round's count in all of them.
__global__ __launch_bounds__(kGB) void k_gather_score(const uint32_t* __restrict__ cand, uint32_t per,
                                                      const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ list,
                                                      const int32_t* __restrict__ shared, int32_t* last,
                                                      const uint32_t* __restrict__ bitmap,
                                                      unsigned long long* arrive, unsigned long long* best,
                                                      const uint32_t* __restrict__ state, int32_t thr) {
  __shared__ uint32_t wsum[kGB / 64];
  if (state[kGatherDone]) return;
  const uint32_t c = gather_candidate_of(blockIdx.x, per);
  if (last[c] < thr) return;  // counts never grow: dead for good
  const uint32_t r = cand[c], len = (uint32_t)shared[r];
  const uint32_t blocks = gather_blocks_of(len, per), first = gather_first_chunk_of(blockIdx.x, per);
  if (first >= blocks) return;  // a shorter list than the longest: no chunk for this workgroup
  const uint32_t* p = list + off[r];
  constexpr int kPer = kGatherChunk / kGB;
  uint32_t mine = 0;
  for (uint64_t chunk = first; chunk * kGatherChunk < len; chunk += per) {
    const uint64_t base = chunk * kGatherChunk + threadIdx.x;
    uint32_t at[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) at[k] = base + (uint64_t)k * kGB < len ? p[base + (uint64_t)k * kGB] : 0xffffffffu;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (at[k] != 0xffffffffu) mine += (bitmap[gather_word_of(at[k])] & gather_bit_of(at[k])) != 0;
  }
  const uint32_t inc = wave_scan(mine);
  if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t count = 0;
#pragma unroll
    for (int w = 0; w < kGB / 64; ++w) count += wsum[w];
    const unsigned long long before = atomicAdd(&arrive[c], gather_arrival(count));
    if ((uint32_t)(before >> 32) == blocks - 1) {  // the last to arrive
      const int32_t total = (int32_t)((uint32_t)before + count);
      arrive[c] = 0;  // for the next round (no workgroup of c is left in this launch)
      last[c] = total;
      if (total >= thr) atomicMax(best, gather_key(total, r));
    }
  }
}

__global__ __launch_bounds__(kWide) void k_gather_take(const uint32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ list,
                                                       const int32_t* __restrict__ shared,
                                                       const uint32_t* __restrict__ r_sizes,
                                                       uint32_t* __restrict__ bitmap,
                                                       unsigned long long* best_now, unsigned long long* best_next,
                                                       uint32_t* state, uint32_t q_size, int32_t thr,
                                                       uint32_t max_rounds, double inv_k,
                                                       sks_gather_hit* __restrict__ hits, uint64_t cap) {
  const uint32_t done = state[kGatherDone], n_hits = state[kGatherHits], remaining = state[kGatherRemaining];
  const unsigned long long key = *best_now;
  __syncthreads();  // every thread has read the state before thread 0 changes it
  if (done) return;
  const int32_t count = gather_key_count(key);
  if (count < thr || (max_rounds && n_hits >= max_rounds)) {
    if (threadIdx.x == 0) state[kGatherDone] = 1;
    return;
  }
  const uint32_t r = gather_key_ref(key), len = (uint32_t)shared[r];
  const uint32_t* p = list + off[r];
  constexpr int kPer = 8;  // list loads in flight per thread, ahead of their atomics
  for (uint64_t base = threadIdx.x; base < len; base += (uint64_t)kWide * kPer) {
    uint32_t at[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) at[k] = base + (uint64_t)k * kWide < len ? p[base + (uint64_t)k * kWide] : 0xffffffffu;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (at[k] != 0xffffffffu) atomicAnd(&bitmap[gather_word_of(at[k])], ~gather_bit_of(at[k]));
  }
  if (threadIdx.x == 0) {
    if (hits && n_hits < cap) {  // past the capacity: counted, not stored
      sks_gather_hit h;
      h.ref = r;
      h.shared = (int32_t)len;
      h.shared_new = count;
      h.ref_size = (int32_t)r_sizes[r];
      h.f_query_new = containment_of(count, (int32_t)q_size);
      h.ani = ani_of(h.shared, h.ref_size, inv_k, nullptr);
      hits[n_hits] = h;
    }
    state[kGatherHits] = n_hits + 1;
    state[kGatherRemaining] = remaining - (uint32_t)count;
    *best_next = 0;
  }
}

}  // namespace

hipError_t launch_gather_offsets(const uint32_t* r_sizes, uint32_t r_n, uint64_t r_total, uint32_t* off,
                                 uint32_t* state, hipStream_t s) {
  hipLaunchKernelGGL(k_gather_offsets, dim3(1), dim3(kWide), 0, s, r_sizes, r_n, r_total, off, state);
  return hipGetLastError();
}

hipError_t launch_gather_member(const uint64_t* q, uint32_t q_size, const uint64_t* r_data,
                                const uint64_t* r_starts, const uint32_t* r_sizes, uint32_t r_n, int elem_words,
                                const uint32_t* off, uint32_t* list, int32_t* shared, const uint32_t* state,
                                hipStream_t s) {
  if (!r_n) return hipSuccess;
  if (r_n > 0x7fffffffu || (elem_words != 1 && elem_words != 2)) return hipErrorInvalidValue;
  if (elem_words == 1)
    hipLaunchKernelGGL(k_gather_member<1>, dim3(r_n), dim3(kGB), 0, s, q, q_size, r_data, r_starts, r_sizes, off,
                       list, shared, state);
  else
    hipLaunchKernelGGL(k_gather_member<2>, dim3(r_n), dim3(kGB), 0, s, q, q_size, r_data, r_starts, r_sizes, off,
                       list, shared, state);
  return hipGetLastError();
}

hipError_t launch_gather_begin(const int32_t* shared, uint32_t r_n, int32_t thr, uint32_t q_size, uint32_t* cand,
                               int32_t* last, uint32_t* bitmap, unsigned long long* best, uint32_t* state,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_gather_cands, dim3(1), dim3(kWide), 0, s, shared, r_n, thr, q_size, cand, last, best, state);
  const uint32_t words = gather_bitmap_words(q_size);
  if (words)
    hipLaunchKernelGGL(k_gather_bitmap, dim3((words + kGB - 1) / kGB), dim3(kGB), 0, s, bitmap, words, q_size);
  return hipGetLastError();
}

hipError_t launch_gather_round(const GatherRound& g, uint32_t round, hipStream_t s) {
  if (!g.n_cand) return hipSuccess;
  if (!g.per || (uint64_t)g.n_cand * g.per > (1ull << 30)) return hipErrorInvalidValue;
  unsigned long long* now = g.best + (round & 1u);
  unsigned long long* next = g.best + ((round & 1u) ^ 1u);
  hipLaunchKernelGGL(k_gather_score, dim3(g.n_cand * g.per), dim3(kGB), 0, s, g.cand, g.per, g.off, g.list, g.shared,
                     g.last, g.bitmap, g.arrive, now, g.state, g.thr);
  hipLaunchKernelGGL(k_gather_take, dim3(1), dim3(kWide), 0, s, g.off, g.list, g.shared, g.r_sizes, g.bitmap, now,
                     next, g.state, g.q_size, g.thr, g.max_rounds, g.inv_k, g.hits, g.hits ? g.cap : 0);
  return hipGetLastError();
}

SKS_CODE_OBJECT_HOOK(gather)

}  // namespace sks
