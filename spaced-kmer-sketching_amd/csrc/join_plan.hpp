// The host arithmetic of the join (no HIP: tests/cpp/join_plan_test.cpp runs it
// on any machine, and join.hip's join_launch / launch_join_slices call the same
// functions): how a join call is cut into bucket groups per tile and into
// launches of whole tiles, when the diagonal tiles are dispatched last, which of
// the two kernels (contiguous chunks or chunks mapped piecewise across regions)
// a call takes, and the bucket count of a layout.  The environment knobs
// (SKS_JOIN_WGS, SKS_JOIN_CAP, SKS_JOIN_TILE_ORDER, SKS_LAYOUT_RG) are read
// where they always were, once per process; their values are passed in.
#pragma once
#include <algorithm>
#include <cstdint>

namespace sks {

// workgroups per launch at most (HIP caps a grid at 2^32 - 1 work-items; a join
// workgroup has 512): larger grids are cut into launches of whole tiles
constexpr uint64_t kJoinMaxGrid = 1ull << 22;
// buckets per window of k_join (join.hip kJWinLog): regions of this many buckets
// need no cross-region windows
constexpr uint32_t kJoinWinLog = 6;
// the layout's geometry limits (join_common.hpp kGLog, kMaxLogB restate these;
// join.hip asserts that they agree)
constexpr uint32_t kJoinGroupLog = 3;
constexpr uint32_t kJoinMaxLogB = 14;

// Bucket groups per tile: ~128 buckets per workgroup (a workgroup's start-up —
// clearing its table and count planes — and its count flush, up to 4096 global
// atomics on a tile of related genomes, are then small beside its chunks), at
// least ~1024 workgroups in all, at least 16 buckets each (round 3 sweep,
// config 4: 4352 workgroups 0.681 ms against 2176: 0.705, 8704: 0.742).  The
// ~128-buckets floor only applies while the grid is small (<= 64K workgroups);
// with very many tiles a tile gets fewer, larger groups (down to one).
// wgs_override (SKS_JOIN_WGS, diagnostics; 0: none) sets the total number of
// workgroups of the call instead.  Every group holds at least one bucket and
// the groups cover [0, B): (n_groups - 1) * buckets_per_group < B <= n_groups *
// buckets_per_group.
struct JoinGroups {
  uint32_t groups;             // the number asked for, within [1, B]
  uint32_t buckets_per_group;  // ceil(B / groups)
  uint32_t n_groups;           // the groups that hold a bucket: ceil(B / buckets_per_group)
};
inline JoinGroups join_plan_groups(uint32_t B, uint64_t tiles, uint64_t wgs_override) {
  if (tiles == 0) tiles = 1;
  // (x - 1) / tiles + 1, not (x + tiles - 1) / tiles: an override near 2^64 must not wrap
  const auto per_tile = [tiles](uint64_t x) { return x ? (x - 1) / tiles + 1 : 0; };
  uint64_t want = wgs_override ? per_tile(wgs_override)
                               : std::max<uint64_t>(std::min<uint64_t>((B + 127) / 128, per_tile(65536)),
                                                    per_tile(1024));
  if (!wgs_override) want = std::min<uint64_t>(want, std::max<uint32_t>(1, B / 16));
  JoinGroups g;
  g.groups = (uint32_t)std::min<uint64_t>(B, std::max<uint64_t>(1, want));
  g.buckets_per_group = (B + g.groups - 1) / g.groups;
  g.n_groups = (B + g.buckets_per_group - 1) / g.buckets_per_group;
  return g;
}

// Whole tiles per launch: tiles_per_launch * n_groups workgroups <= kJoinMaxGrid.
inline uint64_t join_plan_tiles_per_launch(uint32_t n_groups) {
  return std::max<uint64_t>(1, kJoinMaxGrid / std::max<uint32_t>(1, n_groups));
}

// The launches of tiles [tile_begin, tile_end): launch s takes tiles
// [join_plan_slice_begin(s), + join_plan_slice_tiles(s)); its packed output and
// its fused-ANI tile counters start (slice begin - tile_begin) tiles into the
// call's.
inline uint64_t join_plan_slices(uint64_t tile_begin, uint64_t tile_end, uint64_t tiles_per_launch) {
  return tile_end > tile_begin ? (tile_end - tile_begin + tiles_per_launch - 1) / tiles_per_launch : 0;
}
inline uint64_t join_plan_slice_begin(uint64_t tile_begin, uint64_t s, uint64_t tiles_per_launch) {
  return tile_begin + s * tiles_per_launch;
}
inline uint64_t join_plan_slice_tiles(uint64_t tile_begin, uint64_t tile_end, uint64_t s, uint64_t tiles_per_launch) {
  return std::min(tiles_per_launch, tile_end - join_plan_slice_begin(tile_begin, s, tiles_per_launch));
}
inline uint64_t join_plan_slice_offset(uint64_t tile_begin, uint64_t s, uint64_t tiles_per_launch) {
  return join_plan_slice_begin(tile_begin, s, tiles_per_launch) - tile_begin;
}

// Diagonal tiles last: a symmetric launch of every tile (no tile list) that
// fits one launch, unless the plain tile order is asked for (SKS_JOIN_TILE_ORDER).
inline bool join_plan_diag_last(bool sym, bool tile_list, uint64_t tile_begin, uint64_t tile_end,
                                uint32_t n_col_blocks, uint64_t tiles_per_launch, bool plain_order) {
  const uint64_t all_sym = (uint64_t)n_col_blocks * (n_col_blocks + 1) / 2;
  return sym && !tile_list && tile_begin == 0 && tile_end == all_sym && tile_end <= tiles_per_launch && !plain_order;
}

// log2 of the buckets of one region of 2^rg value groups (join_common.hpp lay_rb_log)
inline uint32_t join_plan_region_bucket_log(uint32_t log_b, uint32_t rg) {
  return log_b < kJoinGroupLog + rg ? log_b : kJoinGroupLog + rg;
}

// Windows across regions (the PIECES kernel: false here) unless both layouts
// have 64-bucket regions.  That is known only for one layout: either it covers
// all the call's sketches from block 0 with no tile list, so its build picked
// the region log `natural_rg` from the call's own block count
// (join_layout_region_log), or the caller names the region log the layout was
// built with (layout_rg >= 0).  A tile list otherwise joins per-rank layouts,
// small ones.
inline bool join_plan_contiguous(uint32_t log_b, uint32_t natural_rg, int layout_rg, bool one_layout, bool tile_list,
                                 uint32_t r_blk0, uint32_t c_blk0) {
  return (!tile_list && r_blk0 == 0 && c_blk0 == 0 && one_layout &&
          join_plan_region_bucket_log(log_b, natural_rg) >= kJoinWinLog) ||
         (layout_rg >= 0 && one_layout && join_plan_region_bucket_log(log_b, (uint32_t)layout_rg) >= kJoinWinLog);
}

// Bucket count for the join: mean raw block-bucket population ~ cap / 6, so a
// chunk holds several whole buckets (fewer after deduplication).  cap: column
// entries per chunk (join_cap(): 1024, or SKS_JOIN_CAP clamped to [64, 1024]).
inline uint32_t join_plan_log_b(uint32_t max_size, uint32_t cap) {
  uint32_t log_b = 0;
  while ((1ull << log_b) * (cap / 6) < 64ull * max_size && log_b < kJoinMaxLogB) ++log_b;
  return log_b;
}

}  // namespace sks
