// Query-vs-reference search: from a reference batch's count tiles to a compact
// hit list, on the device.
//
// sks_search joins the query layout with one reference batch's layout into
// packed 64 x 64 count tiles (join.hip, rows = queries).  Nearly all of those
// cells are zero or below the caller's thresholds, and a caller asking which
// of 100 000 stored genomes contain its queries keeps a few hundred of them.
// k_search_hits reads the tiles once, applies the thresholds and appends one
// 32-byte record per surviving pair to a hit buffer, so neither the tiles nor a
// dense matrix ever leave the device.  Batches append in any order; after the
// last one the records are put in (query, ref) order by a radix sort of
// query << ref_bits | ref carrying the record index (post.hip's rocPRIM sort)
// and one gather.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "code_objects.hpp"
#include "search_kernels.hpp"
#include "sks.h"
#include "sks_ani.hpp"

namespace sks {

namespace {

constexpr int kSB = 256;                  // threads per workgroup: 4 wavefronts
constexpr int kTile = 64;
constexpr int kRows = kTile / (kSB / 64);  // tile rows per wavefront

static_assert(sizeof(sks_hit) == 32, "sks_hit is two 16-byte words per record");

// A workgroup per tile, a wavefront per 16 rows, lanes along the row (each load
// is one contiguous 256-byte row of the tile).  A wavefront first tests all its
// cells, keeping the counts in registers and one 64-bit ballot per row, then
// takes its slots with ONE atomicAdd of the ballots' population; a lane's slot
// within a row is its rank in the ballot (mbcnt).
__global__ __launch_bounds__(kSB) void k_search_hits(const int32_t* __restrict__ packed, uint32_t q_blocks,
                                                     uint32_t nq, uint32_t ref0, uint32_t n_batch,
                                                     const uint32_t* __restrict__ q_sizes, double min_containment,
                                                     int32_t min_shared, double inv_k,
                                                     const double* __restrict__ root, uint32_t root_size,
                                                     const uint32_t* __restrict__ stat_q,
                                                     const uint32_t* __restrict__ stat_b, sks_hit* __restrict__ hits,
                                                     uint64_t cap, unsigned long long* __restrict__ counter) {
  if (stat_q[1] | stat_b[1]) return;  // an invalid layout's counts are not counts
  const uint32_t t = blockIdx.x, qi = t % q_blocks, bj = t / q_blocks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t col = bj * kTile + lane;
  const bool col_ok = col < n_batch;
  const int32_t* tile = packed + (uint64_t)t * (kTile * kTile);
  int32_t cnt[kRows], size[kRows];
  unsigned long long ballot[kRows];
  uint32_t total = 0;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const uint32_t r = wave * kRows + i, q = qi * kTile + r;
    const bool row_ok = q < nq;  // uniform over the wavefront
    size[i] = row_ok ? (int32_t)q_sizes[q] : 0;
    cnt[i] = row_ok ? tile[r * kTile + lane] : 0;
    const bool hit = row_ok && col_ok && cnt[i] >= min_shared &&
                     containment_of(cnt[i], size[i]) >= min_containment;
    ballot[i] = __ballot(hit);
    total += (uint32_t)__popcll(ballot[i]);
  }
  if (!total) return;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(counter, (unsigned long long)total);
  base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const unsigned long long b = ballot[i];
    if ((b >> lane) & 1) {
      const uint32_t rank =
          __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
      const unsigned long long slot = base + rank;
      if (slot < cap) {  // past the capacity: counted, not stored
        sks_hit h;
        h.query = qi * kTile + wave * kRows + i;
        h.ref = ref0 + col;
        h.shared = cnt[i];
        h.query_size = size[i];
        const double a = ani_of(cnt[i], size[i], inv_k, &h.containment);
        h.ani = (root && (uint32_t)size[i] == root_size && (uint32_t)cnt[i] <= root_size) ? root[cnt[i]] : a;
        hits[slot] = h;
      }
    }
    base += (unsigned long long)__popcll(b);
  }
}

__global__ __launch_bounds__(kSB) void k_search_keys(const sks_hit* __restrict__ hits, uint64_t n, int ref_bits,
                                                     uint64_t* __restrict__ keys, uint64_t* __restrict__ idx) {
  const uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x;
  if (i >= n) return;
  keys[i] = ((uint64_t)hits[i].query << ref_bits) | hits[i].ref;
  idx[i] = i;
}

__global__ __launch_bounds__(kSB) void k_search_gather(const sks_hit* __restrict__ src,
                                                       const uint64_t* __restrict__ idx, uint64_t n,
                                                       sks_hit* __restrict__ dst) {
  const uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x;
  if (i >= n) return;
  const uint64_t j = idx[i];
  if (j < n) dst[i] = src[j];
}

}  // namespace

hipError_t launch_search_hits(const int32_t* packed, uint32_t q_blocks, uint32_t b_blocks, uint32_t nq,
                              uint32_t ref0, uint32_t n_batch, const uint32_t* q_sizes, double min_containment,
                              int32_t min_shared, int kmer_num_ones, const double* root, uint32_t root_size,
                              const uint32_t* stat_q, const uint32_t* stat_b, sks_hit* hits, uint64_t cap,
                              unsigned long long* counter, hipStream_t s) {
  const uint64_t tiles = (uint64_t)q_blocks * b_blocks;
  if (!tiles) return hipSuccess;
  if (tiles > 0x7fffffffull || kmer_num_ones <= 0) return hipErrorInvalidValue;
  const double inv_k = ((double)1.0) / ((double)kmer_num_ones);
  hipLaunchKernelGGL(k_search_hits, dim3((unsigned)tiles), dim3(kSB), 0, s, packed, q_blocks, nq, ref0, n_batch,
                     q_sizes, min_containment, min_shared < 1 ? 1 : min_shared, inv_k, root, root_size, stat_q,
                     stat_b, hits, hits ? cap : 0, counter);
  return hipGetLastError();
}

hipError_t launch_search_keys(const sks_hit* hits, uint64_t n, int ref_bits, uint64_t* keys, uint64_t* idx,
                              hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_search_keys, dim3((unsigned)((n + kSB - 1) / kSB)), dim3(kSB), 0, s, hits, n, ref_bits, keys,
                     idx);
  return hipGetLastError();
}

hipError_t launch_search_gather(const sks_hit* src, const uint64_t* idx, uint64_t n, sks_hit* dst, hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_search_gather, dim3((unsigned)((n + kSB - 1) / kSB)), dim3(kSB), 0, s, src, idx, n, dst);
  return hipGetLastError();
}

SKS_CODE_OBJECT_HOOK(search)

}  // namespace sks
