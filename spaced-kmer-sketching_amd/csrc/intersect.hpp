// Sketch intersection counts: pair lists, the global kernel and the tiled
// all-pairs driver (intersect.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_mem.hpp"

namespace sks {

hipError_t launch_intersect_pairs(const uint64_t* data, const uint64_t* starts,
                                  const uint32_t* sizes, int elem_words, const int32_t* a,
                                  const int32_t* b, uint64_t n_pairs, int32_t* out, hipStream_t s);
hipError_t launch_intersect_all_global(const uint64_t* data, const uint64_t* starts,
                                       const uint32_t* sizes, int elem_words, uint32_t n,
                                       uint32_t row_begin, uint32_t row_end, int32_t* out,
                                       hipStream_t s);
// Tiled all-pairs (intersect.hip + join.hip): ew = 1 (u64) or 2 (128-bit)
// k-mers.  sym: upper-triangle tiles [tile_begin, tile_end) written to both
// halves of an n x n matrix; otherwise rows [row_begin, row_end) x n.  Zeroes
// `out` first.  *used_tiles = false means no tiled kernel could take the set
// (extreme value skew, or 128-bit k-mers without a join layout): use the
// global kernel.  check: the invariant-checking kernel builds.
hipError_t launch_intersect_tiled(const uint64_t* data, const uint64_t* starts, const uint32_t* sizes,
                                  uint32_t n, bool sym, uint32_t row_begin, uint32_t row_end,
                                  uint64_t tile_begin, uint64_t tile_end, int32_t* out,
                                  Scratch& work, hipStream_t s, bool* used_tiles, int algo, int ew,
                                  bool check);
// intersection kernel choice (sks_ctx_set_intersect_kernel)
constexpr int kIntersectAuto = 0;    // join when the bucket sizes allow, else merge tiles
constexpr int kIntersectMerge = 1;   // k_tiles (pairwise LDS merges)
constexpr int kIntersectJoin = 2;    // k_join (LDS hash join), merge tiles if infeasible
constexpr int kIntersectGlobal = 3;  // one wavefront per pair from global memory
uint64_t intersect_sym_tiles(uint32_t n);
// Common value-range bucket bounds[0..B] (quantiles averaged over up to 64
// sample sketches; any non-decreasing bounds give exact counts) and
// pos[i][b] = first element of sketch i that is >= bounds[b] (pos[i][B] = size).
hipError_t launch_value_bounds(const uint64_t* data, const uint64_t* starts, const uint32_t* sizes,
                               uint32_t n, uint32_t B, uint64_t* bounds, hipStream_t s);
hipError_t launch_bucket_pos(const uint64_t* data, const uint64_t* starts, const uint32_t* sizes,
                             uint32_t n, uint32_t B, const uint64_t* bounds, uint32_t* pos,
                             hipStream_t s);

}  // namespace sks
