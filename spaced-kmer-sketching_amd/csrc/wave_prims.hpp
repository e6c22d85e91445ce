// Device-only wave and workgroup primitives shared by the kernels (wave64).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sks {

// inclusive prefix sum over the 64 lanes of a wave (DPP; no LDS)
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return v;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t x, uint32_t l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, (int)l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), (int)l);
  return ((uint64_t)hi << 32) | lo;
}

// The wave moved up by one lane: lane l receives lane l - 1's v, lane 0 keeps its
// own (DPP wave_shr:1, one VALU move across all four rows; no LDS)
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false);  // wave_shr:1
}
__device__ __forceinline__ uint64_t wave_shr1_64(uint64_t x) {
  return ((uint64_t)wave_shr1((uint32_t)(x >> 32)) << 32) | wave_shr1((uint32_t)x);
}

// Exclusive prefix sum of one count per thread over a workgroup of WAVES
// waves (wsum: WAVES words of LDS); *total (optional) = the sum.  One barrier;
// none after the reads of wsum, so a caller that writes wsum again (another
// scan) or relies on the scan to order its own LDS traffic adds its own.
template <int WAVES>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t* total = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const uint32_t t = wsum[w];
    before += w < wave ? t : 0u;
    all += t;
  }
  if (total) *total = all;
  return before + inc - v;
}

// The same of a predicate (a ballot per wave): this thread's rank among the
// threads with p set, *total = their count.  One barrier, as above.
template <int WAVES>
__device__ __forceinline__ uint32_t block_rank(bool p, uint32_t* wsum, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t bal = __ballot(p);
  const uint32_t in_wave = (uint32_t)__popcll(bal & ((1ull << lane) - 1));
  if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const uint32_t c = wsum[w];
    before += w < wave ? c : 0u;
    all += c;
  }
  *total = all;
  return before + in_wave;
}

}  // namespace sks
