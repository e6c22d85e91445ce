// Device-only pieces the last passes over fully merged groups share (merge.hip's
// duplicate filter, tally.hip's threshold filter): the element types, the chunk
// a workgroup owns, and the order-preserving count and scatter of a chunk's kept
// elements by wave ballots.  Included by .hip units only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "merge_plan.hpp"

namespace sks {

constexpr int kMgB = 256;
constexpr int kMgWaves = kMgB / 64;
constexpr int kMgItems = (int)kMergeTile / kMgB;
static_assert(kMgItems * kMgB == (int)kMergeTile, "a tile is a whole number of block strides");

// One element: a u64 (narrow) or a 16-byte (lo, hi) pair ordered hi word major (wide).
template <int EW>
struct MElem;
template <>
struct MElem<1> {
  using type = uint64_t;
  static __device__ __forceinline__ bool less(type x, type y) { return x < y; }
  static __device__ __forceinline__ bool same(type x, type y) { return x == y; }
};
template <>
struct MElem<2> {
  using type = ulong2;
  static __device__ __forceinline__ bool less(type x, type y) { return x.y < y.y || (x.y == y.y && x.x < y.x); }
  static __device__ __forceinline__ bool same(type x, type y) { return x.x == y.x && x.y == y.y; }
};

// The chunk of this workgroup: group g's elements src[0 .. size), the chunk from `base`.
template <int EW>
struct GroupChunk {
  const typename MElem<EW>::type* src;
  uint64_t size, base;
  uint32_t g;
  __device__ __forceinline__ void open(const uint64_t* runs, const uint64_t* chunk_off, uint32_t n_groups) {
    g = tile_owner(chunk_off, n_groups, blockIdx.x);
    src = reinterpret_cast<const typename MElem<EW>::type*>(runs[2 * (uint64_t)g]);
    size = runs[2 * (uint64_t)g + 1];
    base = (blockIdx.x - chunk_off[g]) * kMergeTile;
  }
  // element i and whether it is the first of its value
  __device__ __forceinline__ bool first_of_value(uint64_t i, typename MElem<EW>::type& v) const {
    if (i >= size) return false;
    v = src[i];
    return i == 0 || !MElem<EW>::same(v, src[i - 1]);
  }
};

// keep(i, v) -> does element i of the group stay (v: the element, read by keep).
// Thread t looks at the chunk's elements base + j * kMgB + t, j < kMgItems.

// counts[blockIdx.x] = the chunk's kept elements.  wsum: kMgWaves words of LDS.
template <int EW, class Keep>
__device__ __forceinline__ void chunk_count(uint64_t base, const Keep& keep, uint32_t* wsum,
                                            uint32_t* __restrict__ counts) {
  using T = typename MElem<EW>::type;
  uint32_t cnt = 0;  // of this wave
#pragma unroll
  for (int j = 0; j < kMgItems; ++j) {
    T v{};
    const bool p = keep(base + (uint64_t)j * kMgB + threadIdx.x, v);
    cnt += (uint32_t)__popcll(__ballot(p));
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t all = 0;
#pragma unroll
    for (int w = 0; w < kMgWaves; ++w) all += wsum[w];
    counts[blockIdx.x] = all;
  }
}

// put(rank, i, v) for every kept element i, rank its place among the chunk's
// kept ones in element order.  wsum: kMgItems * kMgWaves words of LDS, kept per
// (stride j, wave).
template <int EW, class Keep, class Put>
__device__ __forceinline__ void chunk_scatter(uint64_t base, const Keep& keep, uint32_t* wsum, const Put& put) {
  using T = typename MElem<EW>::type;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T v[kMgItems];
  bool p[kMgItems];
  uint32_t in_wave[kMgItems];
#pragma unroll
  for (int j = 0; j < kMgItems; ++j) {
    v[j] = T{};
    p[j] = keep(base + (uint64_t)j * kMgB + threadIdx.x, v[j]);
    const uint64_t bal = __ballot(p[j]);
    in_wave[j] = (uint32_t)__popcll(bal & ((1ull << lane) - 1));
    if (lane == 0) wsum[j * kMgWaves + wave] = (uint32_t)__popcll(bal);
  }
  __syncthreads();
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < kMgItems; ++j) {
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < kMgWaves; ++w) {
      if (w == wave) before = run;
      run += wsum[j * kMgWaves + w];
    }
    if (p[j]) put(before + in_wave[j], base + (uint64_t)j * kMgB + threadIdx.x, v[j]);
  }
}

constexpr uint64_t kMgMaxGrid = 0x7fffffffull;

}  // namespace sks
