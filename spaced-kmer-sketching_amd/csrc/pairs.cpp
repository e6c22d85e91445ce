// C-ABI implementation (include/sks.h): intersections, join layouts, the
// all-pairs and tile-list ANI calls and the count -> ANI conversions.
#include "sks_ani.hpp"
#include "sks_ctx.hpp"

using namespace sks;

namespace {

// Builds the join layout of sketches [0, n) in context scratch, as the all-pairs
// and tile-list ANI calls use it.  c->lay holds the layout's arrays, two status
// words (the caller's d_status is used instead when given), `tiles` packed
// count tiles (*counts comes in null and goes out pointing at them; a caller's
// own tiles are used as they are) and the build's temporary storage.  The
// build's second launch clears the status words, the count tiles and, for the
// fused ANI, the tiles' finisher counters in c->tdone: no memsets.
int layout_in_scratch(sks_ctx* c, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes, int ew,
                      uint32_t n, uint64_t total, uint32_t log_b, const uint64_t* d_bounds, uint32_t blocks_hint,
                      uint64_t tiles, bool ani, uint32_t* d_status, int32_t** counts, JoinLayout* L) {
  Carver cv;
  const LayoutRegions lay = carve_layout(cv, total, (n + 63) / 64, sks::join_layout_boff_words(log_b), ew);
  const Region<uint32_t> r_stat = cv.take<uint32_t>(4);
  const Region<int32_t> r_cnt = cv.take<int32_t>(*counts ? 0 : (size_t)tiles * 4096);
  const Region<char> r_tmp = cv.take<char>(sks::join_layout_temp_bytes(n, log_b, ew) + 256);
  SKS_HIP(c->lay.reserve(cv.need()));
  SKS_HIP(c->tdone.reserve(tiles * sizeof(uint32_t)));
  void* w = c->lay.ptr;
  const LayoutArrays a = lay.in(w);
  uint32_t* stat = d_status ? d_status : r_stat.in(w);
  if (!*counts) *counts = r_cnt.in(w);
  const ZeroSpans zs{{stat, reinterpret_cast<uint32_t*>(*counts), ani ? static_cast<uint32_t*>(c->tdone.ptr) : nullptr},
                     {2, tiles * 4096, ani ? tiles : 0}};
  SKS_HIP(sks::join_layout_build(d_data, d_starts, d_sizes, n, log_b, ew, d_bounds, r_tmp.in(w), a.vals, a.masks,
                                 a.boff, a.bstart, stat, c->join_check, c->stream, &zs, blocks_hint));
  *L = view_of(a);
  return SKS_OK;
}

}  // namespace

extern "C" {

int sks_intersect_pairs(sks_ctx* c, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                        int elem_words, const int32_t* d_a, const int32_t* d_b, uint64_t n_pairs, int32_t* d_out) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_intersect_pairs: null ctx");
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (n_pairs && (!d_starts || !d_sizes || !d_a || !d_b || !d_out))
    return sks::fail(SKS_E_ARG, "sks_intersect_pairs: null argument");
  DeviceGuard g(c->device);
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  SKS_HIP(sks::launch_intersect_pairs(d_data, d_starts, d_sizes, elem_words, d_a, d_b, n_pairs, d_out, c->stream));
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

int sks_intersect_all(sks_ctx* c, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                      int elem_words, uint32_t n, uint32_t row_begin, uint32_t row_end, int32_t* d_out) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_intersect_all: null ctx");
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (row_begin > row_end || row_end > n) return sks::fail(SKS_E_ARG, "sks_intersect_all: bad row range");
  if (row_end > row_begin && (!d_starts || !d_sizes || !d_out))
    return sks::fail(SKS_E_ARG, "sks_intersect_all: null argument");
  DeviceGuard g(c->device);
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  bool done = false;
  if (c->intersect_algo != sks::kIntersectGlobal)
    SKS_HIP(sks::launch_intersect_tiled(d_data, d_starts, d_sizes, n, false, row_begin, row_end, 0, 0, d_out, c->iwork,
                                        c->stream, &done, c->intersect_algo, elem_words, c->join_check));
  if (!done)
    SKS_HIP(sks::launch_intersect_all_global(d_data, d_starts, d_sizes, elem_words, n, row_begin,
                                             row_end, d_out, c->stream));
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

uint64_t sks_intersect_sym_tiles(uint32_t n) { return sks::intersect_sym_tiles(n); }

int sks_intersect_sym(sks_ctx* c, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                      int elem_words, uint32_t n, uint64_t tile_begin, uint64_t tile_end, int32_t* d_out) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_intersect_sym: null ctx");
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (tile_begin > tile_end) return sks::fail(SKS_E_ARG, "sks_intersect_sym: bad tile range");
  if (n && (!d_starts || !d_sizes || !d_out)) return sks::fail(SKS_E_ARG, "sks_intersect_sym: null argument");
  DeviceGuard g(c->device);
  const uint64_t all = sks::intersect_sym_tiles(n);
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  bool done = false;
  if (c->intersect_algo != sks::kIntersectGlobal)
    SKS_HIP(sks::launch_intersect_tiled(d_data, d_starts, d_sizes, n, true, 0, n, tile_begin, tile_end, d_out, c->iwork,
                                        c->stream, &done, c->intersect_algo, elem_words, c->join_check));
  if (!done) {
    if (tile_begin != 0 || tile_end < all)
      return sks::fail(SKS_E_UNSUPPORTED,
                       "sks_intersect_sym: partial tile ranges need sketches without extreme "
                       "value skew; use sks_intersect_all row blocks");
    SKS_HIP(sks::launch_intersect_all_global(d_data, d_starts, d_sizes, elem_words, n, 0, n, d_out, c->stream));
  }
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

uint32_t sks_join_layout_log_b(uint32_t max_sketch_size) { return sks::join_log_b(max_sketch_size); }
uint32_t sks_join_layout_capacity(void) { return sks::join_cap(); }
uint32_t sks_join_layout_region_log(uint32_t n_blocks, uint32_t log_b) {
  return log_b > 14 ? 0u : sks::join_layout_region_log(n_blocks, log_b);
}
int sks_join_launch_plan(uint64_t tiles, uint32_t log_b, uint32_t* n_groups, uint64_t* tiles_per_launch) {
  if (log_b > 14) return sks::fail(SKS_E_ARG, "sks_join_launch_plan: log_b too large");
  sks::join_launch_plan(tiles, log_b, n_groups, tiles_per_launch);
  return SKS_OK;
}
uint32_t sks_join_layout_groups(uint32_t log_b) { return sks::join_layout_groups(log_b); }
uint32_t sks_join_layout_boff_words(uint32_t log_b) { return log_b > 14 ? 0u : sks::join_layout_boff_words(log_b); }

int sks_join_layout_bounds(sks_ctx* c, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                           int elem_words, uint32_t n, uint32_t log_b, uint64_t* d_bounds) {
  SKS_TRY(check_layout_args("sks_join_layout_bounds", c, log_b, elem_words));
  if (!d_bounds || (n && (!d_starts || !d_sizes))) return sks::fail(SKS_E_ARG, "sks_join_layout_bounds: null argument");
  DeviceGuard g(c->device);
  SKS_HIP(sks::join_layout_bounds(d_data, d_starts, d_sizes, n, log_b, elem_words, d_bounds, c->stream));
  return SKS_OK;
}

int sks_join_layout_build(sks_ctx* c, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                          int elem_words, uint32_t n, uint64_t total_hint, uint32_t log_b, const uint64_t* d_bounds,
                          uint64_t* d_out_vals, uint64_t* d_out_masks, uint32_t* d_out_boff, uint64_t* d_out_bstart,
                          uint32_t* max_block_bucket) {
  SKS_TRY(check_layout_args("sks_join_layout_build", c, log_b, elem_words));
  if (!d_out_bstart || (n && (!d_starts || !d_sizes || !d_out_boff)))
    return sks::fail(SKS_E_ARG, "sks_join_layout_build: null argument");
  DeviceGuard g(c->device);
  uint64_t total = total_hint;
  if (n && total == UINT64_MAX) {  // unknown: read the sizes back (waits for the stream)
    std::vector<uint32_t> h_sizes(n);
    SKS_HIP(sks::pinned_d2h(h_sizes.data(), d_sizes, n * sizeof(uint32_t), c->stream));
    total = 0;
    for (uint32_t v : h_sizes) total += v;
  }
  if (!n) total = 0;
  // bucket starts are u32: the layout must hold < 2^32 elements
  if (total >= (1ull << 32))
    return sks::fail(SKS_E_UNSUPPORTED, "sks_join_layout_build: >= 2^32 elements in one layout");
  const size_t o_stat = (sks::join_layout_temp_bytes(n, log_b, elem_words) + 15) & ~(size_t)15;
  SKS_HIP(c->iwork.reserve(o_stat + 16));
  char* w = static_cast<char*>(c->iwork.ptr);
  uint32_t* stat = reinterpret_cast<uint32_t*>(w + o_stat);
  SKS_HIP(hipMemsetAsync(stat, 0, 8, c->stream));
  c->layout_stat = stat;
  if (n == 0) {
    SKS_HIP(hipMemsetAsync(d_out_bstart, 0, 8, c->stream));
  } else {
    SKS_HIP(sks::join_layout_build(d_data, d_starts, d_sizes, n, log_b, elem_words, d_bounds, w, d_out_vals,
                                   d_out_masks, d_out_boff, d_out_bstart, stat, c->join_check, c->stream, nullptr,
                                   c->layout_blocks_hint));
  }
  if (max_block_bucket) {  // NULL: no read-back, the call does not wait for the build
    uint32_t h[2] = {0, 0};
    SKS_HIP(sks::pinned_d2h(h, stat, 8, c->stream));
    *max_block_bucket = h[1] ? UINT32_MAX : h[0];
  }
  return SKS_OK;
}

int sks_join_layout_stat_copy(sks_ctx* c, uint32_t* d_dst) {
  if (!c || !d_dst) return sks::fail(SKS_E_ARG, "sks_join_layout_stat_copy: null argument");
  if (!c->layout_stat) return sks::fail(SKS_E_ARG, "sks_join_layout_stat_copy: no layout built on this context");
  DeviceGuard g(c->device);
  SKS_HIP(hipMemcpyAsync(d_dst, c->layout_stat, 8, hipMemcpyDeviceToDevice, c->stream));
  return SKS_OK;
}

int sks_intersect_sym_layout(sks_ctx* c, uint32_t n, uint32_t log_b, int elem_words, const uint64_t* d_vals,
                             const uint64_t* d_masks, const uint32_t* d_boff, const uint64_t* d_bstart,
                             uint64_t tile_begin, uint64_t tile_end, int32_t* d_out) {
  SKS_TRY(check_layout_args("sks_intersect_sym_layout", c, log_b, elem_words));
  if (tile_begin > tile_end) return sks::fail(SKS_E_ARG, "sks_intersect_sym_layout: bad tile range");
  if (n && (!d_boff || !d_bstart || !d_out))
    return sks::fail(SKS_E_ARG, "sks_intersect_sym_layout: null argument");
  DeviceGuard g(c->device);
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  SKS_HIP(hipMemsetAsync(d_out, 0, (uint64_t)n * n * sizeof(int32_t), c->stream));
  if (n) {
    const sks::JoinLayout L{d_vals, d_masks, d_boff, d_bstart};
    SKS_HIP(sks::join_launch(L, 0, L, 0, n, log_b, elem_words, true, 0, n, tile_begin, tile_end, nullptr, false,
                             d_out, c->join_check, c->stream));
  }
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

int sks_intersect_layout_tiles(sks_ctx* c, uint32_t n, uint32_t log_b, int elem_words, const uint64_t* d_vals,
                               const uint64_t* d_masks, const uint32_t* d_boff, const uint64_t* d_bstart,
                               uint32_t blk0, const uint32_t* d_tiles, uint64_t tile_begin,
                               uint64_t tile_end, int packed, int32_t* d_out) {
  SKS_TRY(check_layout_args("sks_intersect_layout_tiles", c, log_b, elem_words));
  if (tile_begin > tile_end) return sks::fail(SKS_E_ARG, "sks_intersect_layout_tiles: bad tile range");
  if (!d_tiles && tile_end > sks::intersect_sym_tiles(n))
    return sks::fail(SKS_E_ARG, "sks_intersect_layout_tiles: tile range beyond the upper triangle");
  // the upper-triangle range starts at global block 0: a layout whose block 0
  // is another block holds only part of it (a tile list names its blocks)
  if (!d_tiles && blk0 != 0 && tile_end > tile_begin)
    return sks::fail(SKS_E_ARG, "sks_intersect_layout_tiles: a tile range needs blk0 = 0 (pass a tile list)");
  if (tile_end > tile_begin && (!d_boff || !d_bstart || !d_out))
    return sks::fail(SKS_E_ARG, "sks_intersect_layout_tiles: null argument");
  DeviceGuard g(c->device);
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  if (n && tile_end > tile_begin) {
    const sks::JoinLayout L{d_vals, d_masks, d_boff, d_bstart};
    SKS_HIP(sks::join_launch(L, 0u - blk0, L, 0u - blk0, n, log_b, elem_words, true, 0, n, tile_begin, tile_end,
                             d_tiles, packed != 0, d_out, c->join_check, c->stream));
  }
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

int sks_intersect_layout_pair_tiles(sks_ctx* c, uint32_t n, uint32_t log_b, int elem_words,
                                    const uint64_t* d_rvals, const uint64_t* d_rmasks, const uint32_t* d_rboff,
                                    const uint64_t* d_rbstart, uint32_t r_blk0, const uint64_t* d_cvals,
                                    const uint64_t* d_cmasks, const uint32_t* d_cboff, const uint64_t* d_cbstart,
                                    uint32_t c_blk0, const uint32_t* d_tiles, uint64_t tile_begin,
                                    uint64_t tile_end, int packed, int32_t* d_out) {
  SKS_TRY(check_layout_args("sks_intersect_layout_pair_tiles", c, log_b, elem_words));
  if (tile_begin > tile_end) return sks::fail(SKS_E_ARG, "sks_intersect_layout_pair_tiles: bad tile range");
  if (tile_end > tile_begin && (!d_tiles || !d_rboff || !d_rbstart || !d_cboff || !d_cbstart || !d_out))
    return sks::fail(SKS_E_ARG, "sks_intersect_layout_pair_tiles: null argument (a tile list is required)");
  DeviceGuard g(c->device);
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  if (n && tile_end > tile_begin) {
    const sks::JoinLayout R{d_rvals, d_rmasks, d_rboff, d_rbstart}, C{d_cvals, d_cmasks, d_cboff, d_cbstart};
    SKS_HIP(sks::join_launch(R, 0u - r_blk0, C, 0u - c_blk0, n, log_b, elem_words, true, 0, n, tile_begin,
                             tile_end, d_tiles, packed != 0, d_out, c->join_check, c->stream));
  }
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

int sks_intersect_layout_ani(sks_ctx* c, uint32_t n, uint32_t log_b, int elem_words, const uint64_t* d_rvals,
                             const uint64_t* d_rmasks, const uint32_t* d_rboff, const uint64_t* d_rbstart,
                             uint32_t r_blk0, const uint64_t* d_cvals, const uint64_t* d_cmasks,
                             const uint32_t* d_cboff, const uint64_t* d_cbstart, uint32_t c_blk0,
                             const uint32_t* d_tiles, uint64_t tile_begin, uint64_t tile_end, int packed,
                             int32_t* d_out, const int32_t* d_sizes, int kmer_num_ones, double* ani) {
  SKS_TRY(check_layout_args("sks_intersect_layout_ani", c, log_b, elem_words));
  if (kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_intersect_layout_ani: kmer_num_ones must be positive");
  if (tile_begin > tile_end) return sks::fail(SKS_E_ARG, "sks_intersect_layout_ani: bad tile range");
  if (!d_tiles && tile_end > sks::intersect_sym_tiles(n))
    return sks::fail(SKS_E_ARG, "sks_intersect_layout_ani: tile range beyond the upper triangle");
  if (!d_tiles && tile_end > tile_begin && (r_blk0 != 0 || c_blk0 != 0 || d_rvals != d_cvals))
    return sks::fail(SKS_E_ARG, "sks_intersect_layout_ani: a tile range needs one layout with blk0 = 0 "
                                "(pass a tile list)");
  if (tile_end > tile_begin &&
      (!d_rboff || !d_rbstart || !d_cboff || !d_cbstart || !d_out || !d_sizes || !ani))
    return sks::fail(SKS_E_ARG, "sks_intersect_layout_ani: null argument");
  DeviceGuard g(c->device);
  // the ANI matrix may be host memory: the kernel needs its device-side address
  double* d_ani = ani;
  if (tile_end > tile_begin) SKS_TRY(device_view_of_ani(ani, &d_ani, "sks_intersect_layout_ani"));
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  if (n && tile_end > tile_begin) {
    const uint64_t nt = tile_end - tile_begin;
    SKS_HIP(c->tdone.reserve(nt * sizeof(uint32_t)));
    SKS_HIP(hipMemsetAsync(c->tdone.ptr, 0, nt * sizeof(uint32_t), c->stream));
    const sks::JoinLayout R{d_rvals, d_rmasks, d_rboff, d_rbstart}, C{d_cvals, d_cmasks, d_cboff, d_cbstart};
    sks::JoinAni A{d_ani, d_sizes, kmer_num_ones, static_cast<uint32_t*>(c->tdone.ptr)};
    attach_ani_root(c, kmer_num_ones, A);
    SKS_HIP(sks::join_launch(R, 0u - r_blk0, C, 0u - c_blk0, n, log_b, elem_words, true, 0, n, tile_begin,
                             tile_end, d_tiles, packed != 0, d_out, c->join_check, c->stream, &A));
  }
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

int sks_all_pairs_ani(sks_ctx* c, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                      int elem_words, uint32_t n, uint32_t max_size, uint64_t total, int kmer_num_ones,
                      double* ani, int32_t* d_counts, uint32_t* d_status) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_all_pairs_ani: null ctx");
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (ani && kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_all_pairs_ani: kmer_num_ones must be positive");
  if (n && (!d_starts || !d_sizes)) return sks::fail(SKS_E_ARG, "sks_all_pairs_ani: null argument");
  if (total >= (1ull << 32)) return sks::fail(SKS_E_UNSUPPORTED, "sks_all_pairs_ani: >= 2^32 elements");
  DeviceGuard g(c->device);
  double* d_ani = ani;
  if (ani && n) SKS_TRY(device_view_of_ani(ani, &d_ani, "sks_all_pairs_ani"));
  if (n == 0) {
    if (d_status) SKS_HIP(hipMemsetAsync(d_status, 0, 8, c->stream));
    SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
    SKS_HIP(hipEventRecord(c->ev_end, c->stream));
    return SKS_OK;
  }
  // one layout of all n sketches (context scratch), then every upper-triangle
  // tile in one join launch: packed counts and, when asked, the fused ANI
  const uint32_t log_b = sks::join_log_b(std::max<uint32_t>(max_size, 1));
  const uint64_t T = sks::intersect_sym_tiles(n);
  sks::JoinLayout L;
  int32_t* cnt = d_counts;
  SKS_TRY(layout_in_scratch(c, d_data, d_starts, d_sizes, elem_words, n, total, log_b, nullptr, 0, T, ani != nullptr,
                            d_status, &cnt, &L));
  sks::JoinAni A{d_ani, reinterpret_cast<const int32_t*>(d_sizes), kmer_num_ones,
                 static_cast<uint32_t*>(c->tdone.ptr)};
  if (ani) {  // bottom-s sets all hold max_size elements: their ANI comes from the table
    SKS_TRY(sks_ctx_ani_table(c, max_size, kmer_num_ones));
    attach_ani_root(c, kmer_num_ones, A);
  }
  // sks_ctx_last_intersect_ms: the join launch alone (the layout build before it
  // is the call's fixed part)
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  SKS_HIP(sks::join_launch(L, 0, L, 0, n, log_b, elem_words, true, 0, n, 0, T, nullptr, true, cnt, c->join_check,
                           c->stream, ani ? &A : nullptr));
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

int sks_layout_tiles_ani(sks_ctx* c, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                         int elem_words, uint32_t n, uint64_t total, uint32_t log_b, const uint64_t* d_bounds,
                         uint32_t blocks_hint, uint32_t blk0, const uint32_t* d_tiles, uint64_t n_tiles,
                         uint32_t n_global, const int32_t* d_sizes_global, int kmer_num_ones, double* ani,
                         int32_t* d_counts, uint32_t* d_status) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_layout_tiles_ani: null ctx");
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (ani && kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_layout_tiles_ani: kmer_num_ones must be positive");
  if (log_b > sks_join_layout_log_b(~0u)) return sks::fail(SKS_E_ARG, "sks_layout_tiles_ani: log_b too large");
  if (n_tiles && (!d_tiles || !d_counts || (ani && !d_sizes_global)))
    return sks::fail(SKS_E_ARG, "sks_layout_tiles_ani: null argument");
  if (n && (!d_starts || !d_sizes)) return sks::fail(SKS_E_ARG, "sks_layout_tiles_ani: null argument");
  if (total >= (1ull << 32)) return sks::fail(SKS_E_UNSUPPORTED, "sks_layout_tiles_ani: >= 2^32 elements");
  DeviceGuard g(c->device);
  double* d_ani = ani;
  if (ani && n_tiles) SKS_TRY(device_view_of_ani(ani, &d_ani, "sks_layout_tiles_ani"));
  if (n == 0 || n_tiles == 0) {
    if (d_status) SKS_HIP(hipMemsetAsync(d_status, 0, 8, c->stream));
    if (n_tiles) SKS_HIP(hipMemsetAsync(d_counts, 0, n_tiles * 4096 * 4, c->stream));
    SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
    SKS_HIP(hipEventRecord(c->ev_end, c->stream));
    return SKS_OK;
  }
  // the layout in context scratch, as sks_all_pairs_ani: the whole call is four
  // launches and no memset
  const uint32_t nb = (n + 63) / 64;
  sks::JoinLayout L;
  SKS_TRY(layout_in_scratch(c, d_data, d_starts, d_sizes, elem_words, n, total, log_b, d_bounds, blocks_hint, n_tiles,
                            ani != nullptr, d_status, &d_counts, &L));
  sks::JoinAni A{d_ani, d_sizes_global, kmer_num_ones, static_cast<uint32_t*>(c->tdone.ptr)};
  if (ani) attach_ani_root(c, kmer_num_ones, A);
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  // the layout's region log, as join_layout_build picks it: a tile list over
  // this one layout joins without cross-region windows when regions hold 64 buckets
  const int rg = (int)sks::join_layout_region_log(blocks_hint ? std::min(blocks_hint, nb) : nb, log_b);
  SKS_HIP(sks::join_launch(L, 0u - blk0, L, 0u - blk0, n_global, log_b, elem_words, true, 0, n_global, 0, n_tiles,
                           d_tiles, true, d_counts, c->join_check, c->stream, ani ? &A : nullptr, rg));
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

// ---- counts -> containment / ANI (ani.hip) ----------------------------------------------------

int sks_ani_matrix(sks_ctx* c, const int32_t* d_counts, uint32_t n, int kmer_num_ones, double* d_cont, double* d_ani) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ani_matrix: null ctx");
  if (kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_ani_matrix: kmer_num_ones must be positive");
  if (n && (!d_counts || !d_ani)) return sks::fail(SKS_E_ARG, "sks_ani_matrix: null argument");
  DeviceGuard g(c->device);
  SKS_HIP(sks::launch_ani_matrix(d_counts, n, kmer_num_ones, d_cont, d_ani, c->stream));
  return SKS_OK;
}

int sks_ani_rows(sks_ctx* c, const int32_t* d_counts, uint32_t n, uint32_t row_begin, uint32_t row_end,
                 int kmer_num_ones, double* d_cont, double* d_ani) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ani_rows: null ctx");
  if (kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_ani_rows: kmer_num_ones must be positive");
  if (row_begin > row_end || row_end > n) return sks::fail(SKS_E_ARG, "sks_ani_rows: bad row range");
  if (row_end > row_begin && (!d_counts || !d_ani)) return sks::fail(SKS_E_ARG, "sks_ani_rows: null argument");
  DeviceGuard g(c->device);
  SKS_HIP(sks::launch_ani_rows(d_counts, n, row_begin, row_end, kmer_num_ones, d_cont, d_ani, c->stream));
  return SKS_OK;
}

int sks_ani_tiles(sks_ctx* c, const int32_t* d_packed, const uint32_t* d_tiles, uint64_t n_tiles, uint32_t n,
                  const int32_t* d_sizes, int kmer_num_ones, double* d_ani) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ani_tiles: null ctx");
  if (kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_ani_tiles: kmer_num_ones must be positive");
  if (n_tiles && (!d_packed || !d_tiles || !d_sizes || !d_ani))
    return sks::fail(SKS_E_ARG, "sks_ani_tiles: null argument");
  DeviceGuard g(c->device);
  SKS_HIP(sks::launch_ani_tiles(d_packed, d_tiles, n_tiles, n, d_sizes, kmer_num_ones, d_ani, c->stream));
  return SKS_OK;
}

}  // extern "C"
