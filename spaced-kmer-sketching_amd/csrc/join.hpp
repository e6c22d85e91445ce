// The all-pairs join and its layout build (join.hip, layout.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace sks {

// Join layout (layout.hip builds it, join.hip's k_join reads it; format in
// join_common.hpp): per 64-sketch block, each distinct value once with the mask
// of the block's sketches holding it, in value groups x hash buckets, regions
// of groups at their raw offsets.
struct JoinLayout {
  const uint64_t* vals;    // [T * ew] entry values
  const uint64_t* masks;   // [T] sketch masks
  const uint32_t* boff;    // [nb * (B + NR)] bucket starts, then region ends (block-relative)
  const uint64_t* bstart;  // [nb + 1] raw block starts
};
uint32_t join_cap();                       // entries per join chunk (table capacity)
uint32_t join_log_b(uint32_t max_size);    // bucket count for a largest sketch of max_size
// how this process cuts a join call of `tiles` tiles over a layout of 2^log_b
// buckets (join_plan.hpp, with SKS_JOIN_WGS applied): workgroups per tile and
// whole tiles per launch
void join_launch_plan(uint64_t tiles, uint32_t log_b, uint32_t* n_groups, uint64_t* tiles_per_launch);
// G = 2^log_b / 8 value groups (>= 1); bounds: (G + 1) values of ew words.
// join_layout_bounds computes the group bounds of a set (the median over up
// to 64 sample sketches of their quantiles).  join_layout_build: the layout of sketches (data,
// starts, sizes)[0, count) with the caller's bounds, or (d_bounds null)
// bounds computed from these sketches; temp: join_layout_temp_bytes;
// d_stat[0] is raised to the largest block-bucket population (entries),
// d_stat[1] counts groups the build could not place (layout invalid).  Three
// launches, no host synchronisation.  `zero`: up to three word spans the build's
// second launch clears before the placement runs (the caller's status words,
// count tiles, tile counters: no memset launches of their own).
uint32_t join_layout_groups(uint32_t log_b);
// log2 of the value groups per region a build of n_blk blocks uses (1..3)
uint32_t join_layout_region_log(uint32_t n_blk, uint32_t log_b);
uint32_t join_layout_boff_words(uint32_t log_b);  // B + NR: one block's boff row
hipError_t join_layout_bounds(const uint64_t* data, const uint64_t* starts, const uint32_t* sizes,
                              uint32_t count, uint32_t log_b, int ew, uint64_t* bounds, hipStream_t s);
size_t join_layout_temp_bytes(uint32_t count, uint32_t log_b, int ew);
struct ZeroSpans {
  uint32_t* p[3];     // 4-byte aligned, null: unused
  uint64_t words[3];
};
hipError_t join_layout_build(const uint64_t* data, const uint64_t* starts, const uint32_t* sizes,
                             uint32_t count, uint32_t log_b, int ew, const uint64_t* d_bounds, void* temp,
                             uint64_t* out_vals, uint64_t* out_masks, uint32_t* out_boff,
                             uint64_t* out_bstart, uint32_t* d_stat, bool check, hipStream_t s,
                             const ZeroSpans* zero = nullptr, uint32_t blocks_hint = 0);
// Tiles of the n x n (sym: upper-triangle range [tile_begin, tile_end), or
// with d_tiles the (I, J) list entries [tile_begin, tile_end), both halves
// written) or rows x n matrix; tile (I, J) reads row block r_blk0 + I of
// `rows` and column block c_blk0 + J of `cols` (uint32 arithmetic: 0 - blk0
// maps global block indices onto a layout whose block 0 is blk0).  packed:
// out = [tile - tile_begin][64][64].  Counts are added to `out`.
// Fused containment / ANI (sym / tile-list launches only): the last workgroup
// of each tile reads the tile's finished counts back and writes
// ani[i * n + j] = binomial_estimator(containment(count, sizes[i]), k) for both
// orientations of the tile, so the conversion (and, when `ani` is pinned host
// memory, its PCIe transfer) runs under the join instead of after it.
struct JoinAni {
  double* ani;            // n x n row-major: HBM, or host memory mapped for the device
  const int32_t* sizes;   // [n] |S_i| by global genome index
  int kmer_num_ones;      // k of binomial_estimator
  uint32_t* tile_done;    // [tile_end - tile_begin] workgroups finished per tile, zeroed
  const double* root = nullptr;  // optional: root[i] = ANI of i shared elements for a set of root_size
  uint32_t root_size = 0;
};
hipError_t join_launch(const JoinLayout& rows, uint32_t r_blk0, const JoinLayout& cols, uint32_t c_blk0,
                       uint32_t n, uint32_t log_b, int ew, bool sym, uint32_t row_begin, uint32_t row_end,
                       uint64_t tile_begin, uint64_t tile_end, const uint32_t* d_tiles, bool packed,
                       int32_t* out, bool check, hipStream_t s, const JoinAni* ani = nullptr,
                       int layout_rg = -1);
// (layout_rg >= 0: rows and cols are ONE layout built with that region log, so a
// tile list needs no cross-region windows when its regions hold 64 buckets)
// SKS check builds: invariant violations counted since the last call (and reset)
unsigned long long join_check_take();
unsigned long long layout_check_take();

}  // namespace sks
