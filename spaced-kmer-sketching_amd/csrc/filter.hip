// Subtracting or intersecting sketches (sks_sketch_set_filter): an
// order-preserving membership filter of sorted elements against a sorted filter
// sketch, in the count -> scan -> scatter shape of downsample.hip.
//
// Every workgroup owns one chunk of kFilterChunk consecutive elements of one
// source sketch on a dense grid (tile_owner over the host's chunk prefix), four
// elements per thread striped by the workgroup, so every load and store of a
// wavefront is contiguous.  Source chunk and filter sketch both ascend, so only
// the filter elements in [lower_bound(first of chunk), upper_bound(last of
// chunk)) can match: that bracket is found once per chunk, its two ends by one
// wavefront each with the 64-ary narrowing of filter_plan.hpp (the code the CPU
// test runs).  An empty bracket decides the chunk without a search; one of at
// most filter_stage_elems elements is copied into LDS and every thread searches
// its elements there; a longer one is searched in global memory.
//
// Pass 1 (k_sf_mark) writes the ballots of the keep predicate to a bitmap, in
// element order, and the chunk's count; the scan and the new starts and sizes
// are downsample_offsets; pass 2 (k_sf_scatter) reads the elements and the
// bitmap, not the filter, and stores each kept element at its chunk's offset
// plus its rank.  No atomics: the output order is the input order.
#include <hip/hip_runtime.h>

#include "code_objects.hpp"
#include "downsample.hpp"
#include "filter.hpp"
#include "merge_plan.hpp"

namespace sks {

SKS_CODE_OBJECT_HOOK(filter)

namespace {

constexpr int kSfB = 256;
constexpr int kSfWaves = kSfB / 64;
constexpr int kSfItems = (int)kFilterChunk / kSfB;  // elements per thread, striped by kSfB
static_assert(kSfItems * kSfB == (int)kFilterChunk, "chunk is a whole number of block strides");
static_assert(kFilterChunk == kDownsampleChunk, "the chunks are counted by downsample_offsets");
static_assert(kSfItems * kSfWaves == (int)kFilterChunkWords, "one ballot per bitmap word");
static_assert(kFilterStageBytes % 16 == 0 && kFilterStageBytes >= 16, "the stage holds whole wide elements");
constexpr uint64_t kSfMaxGrid = 0x7fffffffull;

// One element: a u64 (narrow) or a 16-byte (lo, hi) pair (wide), moved whole.
template <int EW>
struct FElem;
template <>
struct FElem<1> {
  using type = uint64_t;
  static __device__ __forceinline__ uint64_t lo(type v) { return v; }
  static __device__ __forceinline__ uint64_t hi(type) { return 0; }
};
template <>
struct FElem<2> {
  using type = ulong2;
  static __device__ __forceinline__ uint64_t lo(type v) { return v.x; }
  static __device__ __forceinline__ uint64_t hi(type v) { return v.y; }
};

// The chunk of this workgroup: source sketch g, its elements src[0 .. size), the
// chunk's `len` elements from `base`.
template <int EW>
struct SrcChunk {
  const typename FElem<EW>::type* src;
  uint64_t size, base;
  uint32_t g, len;
  __device__ __forceinline__ void open(const FilterArgs& a) {
    g = tile_owner(a.chunk_off, a.n, blockIdx.x);
    size = a.dense_off[g + 1] - a.dense_off[g];
    base = (blockIdx.x - a.chunk_off[g]) * kFilterChunk;
    len = size - base < kFilterChunk ? (uint32_t)(size - base) : kFilterChunk;
    src = reinterpret_cast<const typename FElem<EW>::type*>(a.data) + a.starts[g];
  }
};

// One end of the bracket by this wavefront: the first index of f[0 .. n) whose
// element is not below (UPPER: is above) the value.
template <int EW, bool UPPER>
__device__ __forceinline__ uint32_t wave_bound(const uint64_t* __restrict__ f, uint32_t n, uint64_t v_lo,
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
__global__ __launch_bounds__(kSfB) void k_sf_mark(const FilterArgs a, uint64_t* __restrict__ bitmap,
                                                  uint32_t* __restrict__ counts) {
  using T = typename FElem<EW>::type;
  __shared__ __attribute__((aligned(16))) uint64_t stage[kFilterStageBytes / 8];
  __shared__ uint32_t range[2];
  __shared__ uint32_t wsum[kSfWaves];
  SrcChunk<EW> ch;
  ch.open(a);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T v[kSfItems];
  bool valid[kSfItems];
#pragma unroll
  for (int j = 0; j < kSfItems; ++j) {
    const uint32_t e = (uint32_t)j * kSfB + threadIdx.x;
    valid[j] = e < ch.len;
    v[j] = T{};
    if (valid[j]) v[j] = ch.src[ch.base + e];
  }
  const uint64_t fsize = a.frange[2 * (uint64_t)ch.g + 1];
  const bool copies = fsize == kFilterNone;  // workgroup-uniform, like everything about the bracket
  const uint64_t* __restrict__ f = a.fdata + a.frange[2 * (uint64_t)ch.g] * EW;
  if (wave < 2) {
    uint32_t end = 0;
    if (!copies && fsize != 0) {
      const T edge = ch.src[ch.base + (wave == 0 ? 0u : ch.len - 1u)];
      end = wave == 0 ? wave_bound<EW, false>(f, (uint32_t)fsize, FElem<EW>::lo(edge), FElem<EW>::hi(edge))
                      : wave_bound<EW, true>(f, (uint32_t)fsize, FElem<EW>::lo(edge), FElem<EW>::hi(edge));
    }
    if (lane == 0) range[wave] = end;
  }
  __syncthreads();
  const uint32_t lb = range[0], ub = range[1], rlen = ub - lb;
  bool found[kSfItems] = {};
  if (rlen != 0) {
    if (filter_staged(rlen, EW, a.no_stage != 0)) {
      const T* from = reinterpret_cast<const T*>(f) + lb;
      T* to = reinterpret_cast<T*>(stage);
      for (uint32_t i = threadIdx.x; i < rlen; i += kSfB) to[i] = from[i];
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kSfItems; ++j)
        if (valid[j]) found[j] = filter_member<EW>(stage, 0u, rlen, FElem<EW>::lo(v[j]), FElem<EW>::hi(v[j]));
    } else {
#pragma unroll
      for (int j = 0; j < kSfItems; ++j)
        if (valid[j]) found[j] = filter_member<EW>(f, lb, ub, FElem<EW>::lo(v[j]), FElem<EW>::hi(v[j]));
    }
  }
  uint64_t* words = bitmap + (uint64_t)blockIdx.x * kFilterChunkWords;
  uint32_t cnt = 0;  // of this wave
#pragma unroll
  for (int j = 0; j < kSfItems; ++j) {
    const bool keep = valid[j] && (copies || filter_keeps(found[j], a.kind));
    const uint64_t bal = __ballot(keep);
    if (lane == 0) words[filter_ballot_word((uint32_t)j, wave)] = bal;
    cnt += (uint32_t)__popcll(bal);
  }
  if (lane == 0) wsum[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t all = 0;
#pragma unroll
    for (int w = 0; w < kSfWaves; ++w) all += wsum[w];
    counts[blockIdx.x] = all;
  }
}

// The rank of a kept element is the kept elements of the bitmap words before
// its own plus those of the lanes below it: block_rank's scheme, the per-wave
// counts read from the bitmap instead of LDS.
template <int EW>
__global__ __launch_bounds__(kSfB) void k_sf_scatter(const FilterArgs a, const uint64_t* __restrict__ bitmap,
                                                     const uint64_t* __restrict__ offs,
                                                     uint64_t* __restrict__ out_words) {
  using T = typename FElem<EW>::type;
  SrcChunk<EW> ch;
  ch.open(a);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t* words = bitmap + (uint64_t)blockIdx.x * kFilterChunkWords;
  T* out = reinterpret_cast<T*>(out_words) + offs[blockIdx.x];
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < kSfItems; ++j) {
    uint32_t before = 0;
    uint64_t mine = 0;
#pragma unroll
    for (int w = 0; w < kSfWaves; ++w) {
      const uint64_t bits = words[filter_ballot_word((uint32_t)j, (uint32_t)w)];
      if ((uint32_t)w == wave) {
        before = run;
        mine = bits;
      }
      run += (uint32_t)__popcll(bits);
    }
    if ((mine >> lane) & 1ull) {
      const uint32_t e = (uint32_t)j * kSfB + threadIdx.x;  // < ch.len: the tail's bits are zero
      out[before + (uint32_t)__popcll(mine & ((1ull << lane) - 1))] = ch.src[ch.base + e];
    }
  }
}

}  // namespace

hipError_t filter_mark(const FilterArgs& args, int ew, uint64_t n_chunks, uint64_t* bitmap, uint32_t* counts,
                       hipStream_t s) {
  if (args.n == 0 || n_chunks == 0) return hipSuccess;
  if (n_chunks > kSfMaxGrid) return hipErrorInvalidValue;
  if (ew == 1)
    hipLaunchKernelGGL(k_sf_mark<1>, dim3((unsigned)n_chunks), dim3(kSfB), 0, s, args, bitmap, counts);
  else
    hipLaunchKernelGGL(k_sf_mark<2>, dim3((unsigned)n_chunks), dim3(kSfB), 0, s, args, bitmap, counts);
  return hipGetLastError();
}

hipError_t filter_scatter(const FilterArgs& args, int ew, uint64_t n_chunks, const uint64_t* bitmap,
                          const uint64_t* offs, uint64_t* out, hipStream_t s) {
  if (args.n == 0 || n_chunks == 0) return hipSuccess;
  if (n_chunks > kSfMaxGrid) return hipErrorInvalidValue;
  if (ew == 1)
    hipLaunchKernelGGL(k_sf_scatter<1>, dim3((unsigned)n_chunks), dim3(kSfB), 0, s, args, bitmap, offs, out);
  else
    hipLaunchKernelGGL(k_sf_scatter<2>, dim3((unsigned)n_chunks), dim3(kSfB), 0, s, args, bitmap, offs, out);
  return hipGetLastError();
}

}  // namespace sks
