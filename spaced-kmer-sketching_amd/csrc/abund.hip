// K-mer abundances on the device (arithmetic: abund_plan.hpp).
//
// Run lengths.  seg_unique_scan leaves, per sorted record, a "first of its run"
// flag and the exclusive scan of the flags, so a run's rank among all distinct
// values is its first record's position.  k_ab_run_starts stores each first
// record's index at that rank; k_ab_run_lengths gives every rank the distance to
// the next run's first record, or to the segment's end for a segment's last run.
// Both are O(1) per record or distinct value: a homopolymer's run of millions of
// equal keys costs one subtraction.
//
// Trim.  The count -> scan -> scatter shape of downsample.hip and filter.hip:
// every workgroup owns one chunk of kDownsampleChunk consecutive elements of one
// sketch, four per thread striped by the workgroup.  k_ab_mark writes the
// ballots of the keep rule to a bitmap in element order and the chunk's count;
// the scan and the new starts and sizes are downsample_offsets; k_ab_scatter
// stores each kept element and its abundance at its chunk's offset plus its
// rank.  No atomics: the output order is the input order.
//
// Weighted pairs.  One workgroup per pair on a grid-strided loop.  The smaller
// sketch is walked in chunks; each chunk's bracket in the larger sketch is found
// by two wavefronts with the 64-ary narrowing of filter_plan.hpp, and every
// thread searches its elements inside the bracket.  The abundance is the
// sample's: at the walked position when the sample is walked, at the found one
// when the reference is.  Counts and weights are summed per wavefront, then over
// the workgroup's four wavefronts through LDS, and one thread stores the pair's
// result: no atomics, so the same input gives the same bits.
#include <hip/hip_runtime.h>

#include "abund.hpp"
#include "code_objects.hpp"
#include "downsample.hpp"
#include "filter_plan.hpp"
#include "merge_plan.hpp"
#include "wave_prims.hpp"

namespace sks {

SKS_CODE_OBJECT_HOOK(abund)

namespace {

constexpr int kAbB = 256;
constexpr int kAbWaves = kAbB / 64;
constexpr int kAbItems = (int)kDownsampleChunk / kAbB;  // elements per thread, striped by kAbB
static_assert(kAbItems * kAbB == (int)kDownsampleChunk, "chunk is a whole number of block strides");
static_assert(kFilterChunk == kDownsampleChunk, "the bitmap layout is the filter's");
static_assert(kAbItems * kAbWaves == (int)kFilterChunkWords, "one ballot per bitmap word");
constexpr uint64_t kAbMaxGrid = 0x7fffffffull;
constexpr uint32_t kAbLoopGrid = 16384;  // workgroups of the grid-strided kernels

uint32_t grid_for(uint64_t n) {
  const uint64_t g = (n + kAbB - 1) / kAbB;
  return (uint32_t)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}

// ---- run lengths ---------------------------------------------------------------------------
__global__ __launch_bounds__(kAbB) void k_ab_run_starts(const uint32_t* __restrict__ flag,
                                                        const uint64_t* __restrict__ pos,
                                                        const uint64_t* __restrict__ off,
                                                        uint64_t* __restrict__ run_start) {
  const uint32_t g = blockIdx.y;
  const uint64_t b = off[g], e = off[g + 1];
  for (uint64_t i = b + (uint64_t)blockIdx.x * kAbB + threadIdx.x; i < e; i += (uint64_t)gridDim.x * kAbB)
    if (flag[i]) run_start[pos[i]] = i;
}

__global__ __launch_bounds__(kAbB) void k_ab_run_lengths(const uint64_t* __restrict__ pos,
                                                         const uint64_t* __restrict__ off,
                                                         const uint64_t* __restrict__ run_start,
                                                         uint32_t* __restrict__ abund, uint64_t* __restrict__ starts,
                                                         uint32_t* __restrict__ sizes) {
  const uint32_t g = blockIdx.y;
  const uint64_t seg_end = off[g + 1];
  const uint64_t rb = pos[off[g]], re = pos[seg_end];
  for (uint64_t r = rb + (uint64_t)blockIdx.x * kAbB + threadIdx.x; r < re; r += (uint64_t)gridDim.x * kAbB)
    abund[r] = abund_run_length(run_start, r, re, seg_end);
  if (starts && blockIdx.x == 0 && threadIdx.x == 0) {
    starts[g] = rb;
    sizes[g] = (uint32_t)(re - rb);
  }
}

// ---- trim ----------------------------------------------------------------------------------
// The chunk of this workgroup: sketch g, the chunk's `len` elements from `base`
// of the sketch's `first` (len 0 past the sketch's device size).
struct TrimChunk {
  uint64_t first, base;
  uint32_t g, len;
  __device__ __forceinline__ void open(const AbundTrimArgs& a) {
    g = tile_owner(a.chunk_off, a.n, blockIdx.x);
    const uint64_t size = a.sizes[g];
    base = (blockIdx.x - a.chunk_off[g]) * kDownsampleChunk;
    len = base >= size ? 0u : (size - base < kDownsampleChunk ? (uint32_t)(size - base) : kDownsampleChunk);
    first = a.starts[g];
  }
};

__global__ __launch_bounds__(kAbB) void k_ab_mark(const AbundTrimArgs a, uint64_t* __restrict__ bitmap,
                                                  uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kAbWaves];
  TrimChunk ch;
  ch.open(a);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t* __restrict__ ab = a.abund + ch.first + ch.base;
  uint64_t* words = bitmap + (uint64_t)blockIdx.x * kFilterChunkWords;
  uint32_t cnt = 0;  // of this wave
#pragma unroll
  for (int j = 0; j < kAbItems; ++j) {
    const uint32_t e = (uint32_t)j * kAbB + threadIdx.x;
    const bool keep = e < ch.len && abund_keeps(ab[e], a.min_abund, a.max_abund);
    const uint64_t bal = __ballot(keep);
    if (lane == 0) words[filter_ballot_word((uint32_t)j, wave)] = bal;
    cnt += (uint32_t)__popcll(bal);
  }
  if (lane == 0) wsum[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t all = 0;
#pragma unroll
    for (int w = 0; w < kAbWaves; ++w) all += wsum[w];
    counts[blockIdx.x] = all;
  }
}

template <int EW>
struct AbElem;
template <>
struct AbElem<1> {
  using type = uint64_t;
};
template <>
struct AbElem<2> {
  using type = ulong2;  // a 16-byte (lo, hi) pair, moved whole
};

// The rank of a kept element is the kept elements of the bitmap words before
// its own plus those of the lanes below it (filter.hip k_sf_scatter's scheme).
template <int EW>
__global__ __launch_bounds__(kAbB) void k_ab_scatter(const AbundTrimArgs a, const uint64_t* __restrict__ bitmap,
                                                     const uint64_t* __restrict__ offs,
                                                     uint64_t* __restrict__ out_words,
                                                     uint32_t* __restrict__ out_abund) {
  using T = typename AbElem<EW>::type;
  TrimChunk ch;
  ch.open(a);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t* words = bitmap + (uint64_t)blockIdx.x * kFilterChunkWords;
  const T* __restrict__ src = reinterpret_cast<const T*>(a.data) + ch.first + ch.base;
  const uint32_t* __restrict__ ab = a.abund + ch.first + ch.base;
  T* out = reinterpret_cast<T*>(out_words) + offs[blockIdx.x];
  uint32_t* oab = out_abund + offs[blockIdx.x];
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < kAbItems; ++j) {
    uint32_t before = 0;
    uint64_t mine = 0;
#pragma unroll
    for (int w = 0; w < kAbWaves; ++w) {
      const uint64_t bits = words[filter_ballot_word((uint32_t)j, (uint32_t)w)];
      if ((uint32_t)w == wave) {
        before = run;
        mine = bits;
      }
      run += (uint32_t)__popcll(bits);
    }
    if ((mine >> lane) & 1ull) {
      const uint32_t e = (uint32_t)j * kAbB + threadIdx.x;  // < ch.len: the tail's bits are zero
      const uint32_t at = before + (uint32_t)__popcll(mine & ((1ull << lane) - 1));
      out[at] = src[e];
      oab[at] = ab[e];
    }
  }
}

// ---- sums over a workgroup -----------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The workgroup's sums of (count, weight) in thread 0 (the others' values are
// unspecified).  Two barriers: the second frees the LDS words for the next call.
__device__ __forceinline__ void block_sums(uint32_t count, unsigned long long weight, uint32_t* wcnt,
                                           unsigned long long* wwgt, uint32_t* count_out,
                                           unsigned long long* weight_out) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t c = wave_scan(count);  // lane 63: the wave's count
  const unsigned long long w = wave_sum64(weight);
  if (lane == 63) {
    wcnt[wave] = c;
    wwgt[wave] = w;
  }
  __syncthreads();
  uint32_t call = 0;
  unsigned long long wall = 0;
#pragma unroll
  for (int i = 0; i < kAbWaves; ++i) {
    call += wcnt[i];
    wall += wwgt[i];
  }
  *count_out = call;
  *weight_out = wall;
  __syncthreads();
}

// ---- weighted pairs ------------------------------------------------------------------------
// One end of the bracket by this wavefront (filter.hip wave_bound): the first
// index of f[0 .. n) whose element is not below (UPPER: is above) the value.
template <int EW, bool UPPER>
__device__ __forceinline__ uint32_t ab_wave_bound(const uint64_t* __restrict__ f, uint32_t n, uint64_t v_lo,
                                                  uint64_t v_hi) {
  const uint32_t lane = threadIdx.x & 63;
  FilterRange r{0u, n};
  for (;;) {
    const uint32_t i = filter_probe(r, lane);
    bool t = false;
    if (i < r.hi) {
      const uint64_t* e = f + (size_t)i * EW;
      t = UPPER ? filter_not_above<EW>(e, v_lo, v_hi) : filter_below<EW>(e, v_lo, v_hi);
    }
    bool done;
    r = filter_narrow(r, (uint32_t)__popcll(__ballot(t)), &done);  // wave-uniform
    if (done) return r.lo;
  }
}

template <int EW>
__global__ __launch_bounds__(kAbB) void k_ab_pairs(const AbundPairsArgs a) {
  __shared__ uint32_t range[2];
  __shared__ uint32_t wcnt[kAbWaves];
  __shared__ unsigned long long wwgt[kAbWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t p = blockIdx.x; p < a.n_pairs; p += gridDim.x) {
    const int32_t ia = a.d_a[p], ib = a.d_b[p];  // workgroup-uniform, like everything about the pair
    if (ia < 0 || (uint32_t)ia >= a.s_n || ib < 0 || (uint32_t)ib >= a.r_n) {
      if (threadIdx.x == 0) {
        a.shared[p] = -1;
        a.weight[p] = 0;
      }
      continue;
    }
    const uint32_t na = a.s_sizes[ia], nb = a.r_sizes[ib];
    const uint64_t* __restrict__ A = a.s_data + a.s_starts[ia] * EW;
    const uint64_t* __restrict__ B = a.r_data + a.r_starts[ib] * EW;
    const uint32_t* __restrict__ ab = a.s_abund + a.s_starts[ia];
    const bool walk_sample = na <= nb;
    const uint64_t* __restrict__ S = walk_sample ? A : B;  // walked in chunks
    const uint64_t* __restrict__ L = walk_sample ? B : A;  // searched
    const uint32_t ns = walk_sample ? na : nb, nl = walk_sample ? nb : na;
    uint32_t count = 0;
    unsigned long long weight = 0;
    for (uint32_t base = 0; base < ns; base += kDownsampleChunk) {  // ns <= nl, so L is not empty
      const uint32_t len = ns - base < kDownsampleChunk ? ns - base : kDownsampleChunk;
      if (wave < 2) {
        const uint64_t* edge = S + (size_t)(base + (wave == 0 ? 0u : len - 1u)) * EW;
        const uint64_t e_lo = edge[0], e_hi = EW == 2 ? edge[EW - 1] : 0;
        const uint32_t end = wave == 0 ? ab_wave_bound<EW, false>(L, nl, e_lo, e_hi)
                                       : ab_wave_bound<EW, true>(L, nl, e_lo, e_hi);
        if (lane == 0) range[wave] = end;
      }
      __syncthreads();
      const uint32_t lb = range[0], ub = range[1];
      if (ub > lb) {
#pragma unroll
        for (int j = 0; j < kAbItems; ++j) {
          const uint32_t e = (uint32_t)j * kAbB + threadIdx.x;
          if (e < len) {
            const uint64_t* v = S + (size_t)(base + e) * EW;
            const uint64_t v_lo = v[0], v_hi = EW == 2 ? v[EW - 1] : 0;
            const uint32_t i = gather_lower_bound<EW>(L, lb, ub, v_lo, v_hi);
            if (i < ub && gather_equal<EW>(L + (size_t)i * EW, v_lo, v_hi)) {
              ++count;
              weight += ab[walk_sample ? base + e : i];
            }
          }
        }
      }
      __syncthreads();  // range is written again
    }
    uint32_t call;
    unsigned long long wall;
    block_sums(count, weight, wcnt, wwgt, &call, &wall);
    if (threadIdx.x == 0) {
      a.shared[p] = (int32_t)call;
      a.weight[p] = wall;
    }
  }
}

// ---- totals --------------------------------------------------------------------------------
__global__ __launch_bounds__(kAbB) void k_ab_totals(const uint32_t* __restrict__ abund,
                                                    const uint64_t* __restrict__ starts,
                                                    const uint32_t* __restrict__ sizes, uint32_t n,
                                                    unsigned long long* __restrict__ totals) {
  __shared__ uint32_t wcnt[kAbWaves];
  __shared__ unsigned long long wwgt[kAbWaves];
  for (uint32_t g = blockIdx.x; g < n; g += gridDim.x) {
    const uint32_t* __restrict__ ab = abund + starts[g];
    const uint32_t size = sizes[g];
    unsigned long long sum = 0;
    for (uint32_t i = threadIdx.x; i < size; i += kAbB) sum += ab[i];
    uint32_t call;
    unsigned long long all;
    block_sums(0u, sum, wcnt, wwgt, &call, &all);
    if (threadIdx.x == 0) totals[g] = all;
  }
}

}  // namespace

hipError_t abund_run_lengths(const uint32_t* d_flag, const uint64_t* d_pos, const uint64_t* d_off, uint32_t n_seg,
                             uint64_t max_len, uint64_t* run_start, uint32_t* abund, uint64_t* starts,
                             uint32_t* sizes, hipStream_t s) {
  if (n_seg == 0) return hipSuccess;
  const dim3 grid(grid_for(max_len < (1ull << 24) ? max_len : (1ull << 24)), n_seg);
  hipLaunchKernelGGL(k_ab_run_starts, grid, dim3(kAbB), 0, s, d_flag, d_pos, d_off, run_start);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ab_run_lengths, grid, dim3(kAbB), 0, s, d_pos, d_off, run_start, abund, starts, sizes);
  return hipGetLastError();
}

hipError_t abund_trim_mark(const AbundTrimArgs& args, uint64_t n_chunks, uint64_t* bitmap, uint32_t* counts,
                           hipStream_t s) {
  if (args.n == 0 || n_chunks == 0) return hipSuccess;
  if (n_chunks > kAbMaxGrid) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ab_mark, dim3((unsigned)n_chunks), dim3(kAbB), 0, s, args, bitmap, counts);
  return hipGetLastError();
}

hipError_t abund_trim_scatter(const AbundTrimArgs& args, int ew, uint64_t n_chunks, const uint64_t* bitmap,
                              const uint64_t* offs, uint64_t* out, uint32_t* out_abund, hipStream_t s) {
  if (args.n == 0 || n_chunks == 0) return hipSuccess;
  if (n_chunks > kAbMaxGrid) return hipErrorInvalidValue;
  if (ew == 1)
    hipLaunchKernelGGL(k_ab_scatter<1>, dim3((unsigned)n_chunks), dim3(kAbB), 0, s, args, bitmap, offs, out,
                       out_abund);
  else
    hipLaunchKernelGGL(k_ab_scatter<2>, dim3((unsigned)n_chunks), dim3(kAbB), 0, s, args, bitmap, offs, out,
                       out_abund);
  return hipGetLastError();
}

hipError_t abund_pairs(const AbundPairsArgs& args, int ew, hipStream_t s) {
  if (args.n_pairs == 0) return hipSuccess;
  const unsigned grid = (unsigned)(args.n_pairs < kAbLoopGrid ? args.n_pairs : kAbLoopGrid);
  if (ew == 1)
    hipLaunchKernelGGL(k_ab_pairs<1>, dim3(grid), dim3(kAbB), 0, s, args);
  else
    hipLaunchKernelGGL(k_ab_pairs<2>, dim3(grid), dim3(kAbB), 0, s, args);
  return hipGetLastError();
}

hipError_t abund_totals(const uint32_t* abund, const uint64_t* starts, const uint32_t* sizes, uint32_t n,
                        unsigned long long* totals, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const unsigned grid = n < kAbLoopGrid ? n : kAbLoopGrid;
  hipLaunchKernelGGL(k_ab_totals, dim3(grid), dim3(kAbB), 0, s, abund, starts, sizes, n, totals);
  return hipGetLastError();
}

}  // namespace sks
