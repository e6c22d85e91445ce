// C-ABI implementation (include/sks.h): single-linkage clusters of a sketch set
// (kernels in cluster.hip, arithmetic in cluster_plan.hpp, layout and join as
// the search and the all-pairs calls).
#include "cluster_plan.hpp"
#include "sks_ctx.hpp"

using namespace sks;

namespace {

// packed count tiles of one batch of column blocks (16 KB a tile), as the search's
constexpr uint64_t kClusterTileBudget = 256ull << 20;

// h_bounds, invalid_layout: as the core of with_mask_bounds_retry (null: sampled from the set).
//
// The set is joined with itself and the link rule is symmetric, so ONE layout
// serves rows and columns and only the tiles (I, J), I <= J, are joined.  The
// tiles are listed column by column (cluster_plan.hpp) and uploaded once; a
// batch is a range of whole columns of that list, joined into the one tile
// buffer and linked before the next batch clears it.  Batches bound the count
// tiles, never the layout: the layout of the whole set is needed for the rows
// of every batch anyway, so no batch builds one of its own.
int cluster_core(sks_ctx* c, const char* who, const SketchSpan& S, int ew, double min_containment,
                 int32_t min_shared, const std::vector<uint64_t>* h_bounds, uint32_t* d_cluster, uint32_t* d_rep,
                 uint32_t* n_clusters, bool* invalid_layout = nullptr) {
  const std::string me(who);
  *n_clusters = 0;
  if (S.n == 0) return SKS_OK;
  DeviceGuard g(c->device);
  const uint32_t log_b = sks::join_log_b(std::max<uint32_t>(S.max_size, 1));
  const uint32_t nb = (S.n + 63) / 64;
  const uint64_t tiles_all = cluster_tiles_before(nb);
  if (tiles_all > 0x7fffffffull) return sks::fail(SKS_E_UNSUPPORTED, me + ": too many 64-sketch blocks");
  // column blocks per batch: the caller's, else what the tile budget holds (a
  // column has at most nb tiles)
  uint64_t bb64 = c->search_batch ? c->search_batch : std::max<uint64_t>(1, kClusterTileBudget / ((uint64_t)nb * 16384));
  const uint32_t bb = (uint32_t)std::min<uint64_t>(bb64, nb);
  const uint32_t n_batches = cluster_batches(nb, bb);
  uint64_t tiles_max = 0;
  for (uint32_t b = 0; b < n_batches; ++b) {
    const ClusterRange r = cluster_batch_range(nb, bb, b);
    tiles_max = std::max(tiles_max, r.end - r.begin);
  }
  const size_t BW = sks::join_layout_boff_words(log_b);
  const uint32_t chunks = (S.n + kClusterChunk - 1) / kClusterChunk;
  // c->lay: the group bounds, the layout, [status 0, status 1, clusters, -], the
  // tile list, one batch's packed counts, parent / root / id (n words each), the
  // representative keys, the roots per chunk and the layout build's temporary storage
  Carver cv;
  const Region<uint64_t> r_bounds = cv.take<uint64_t>((size_t)(sks::join_layout_groups(log_b) + 1) * ew);
  const LayoutRegions r_lay = carve_layout(cv, S.total, nb, BW, ew);
  const Region<uint32_t> r_stat = cv.take<uint32_t>(4);
  const Region<uint32_t> r_tiles = cv.take<uint32_t>(tiles_all * 2);
  const Region<int32_t> r_cnt = cv.take<int32_t>(tiles_max * 4096);
  const Region<uint32_t> r_parent = cv.take<uint32_t>(S.n), r_root = cv.take<uint32_t>(S.n), r_id = cv.take<uint32_t>(S.n);
  const Region<unsigned long long> r_key = cv.take<unsigned long long>(S.n);
  const Region<uint32_t> r_chunk = cv.take<uint32_t>(chunks);
  const Region<char> r_tmp = cv.take<char>(sks::join_layout_temp_bytes(S.n, log_b, ew) + 256);
  SKS_HIP(c->lay.reserve(cv.need()));
  void* w = c->lay.ptr;
  uint64_t* bounds = r_bounds.in(w);
  const LayoutArrays A = r_lay.in(w);
  const sks::JoinLayout L = view_of(A);
  uint32_t* stat = r_stat.in(w);
  uint32_t* tiles = r_tiles.in(w);
  int32_t* cnt = r_cnt.in(w);
  uint32_t* parent = r_parent.in(w);

  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  {
    const std::vector<uint32_t> h_tiles = cluster_tile_list(nb);
    SKS_HIP(sks::pinned_h2d(tiles, h_tiles.data(), h_tiles.size() * 4, c->stream));
  }
  SKS_TRY(queue_group_bounds(c, S, log_b, ew, h_bounds, bounds));
  // the layout, once; its second launch clears the status words, the cluster
  // count and the first batch's tiles
  const ClusterRange first = cluster_batch_range(nb, bb, 0);
  const sks::ZeroSpans zs{{stat, reinterpret_cast<uint32_t*>(cnt), nullptr}, {4, (first.end - first.begin) * 4096, 0}};
  SKS_HIP(sks::join_layout_build(S.data, S.starts, S.sizes, S.n, log_b, ew, bounds, r_tmp.in(w), A.vals, A.masks,
                                 A.boff, A.bstart, stat, c->join_check, c->stream, &zs));
  SKS_HIP(sks::launch_cluster_init(parent, r_key.in(w), S.n, c->stream));
  // the layout's region log, as the build picks it: a tile list over this one
  // layout joins without cross-region windows when regions hold 64 buckets
  const int rg = (int)sks::join_layout_region_log(nb, log_b);
  for (uint32_t b = 0; b < n_batches; ++b) {
    const ClusterRange r = cluster_batch_range(nb, bb, b);
    const uint64_t nt = r.end - r.begin;
    if (b) SKS_HIP(hipMemsetAsync(cnt, 0, nt * 4096 * sizeof(int32_t), c->stream));
    SKS_HIP(sks::join_launch(L, 0, L, 0, S.n, log_b, ew, true, 0, S.n, r.begin, r.end, tiles, true, cnt,
                             c->join_check, c->stream, nullptr, rg));
    SKS_HIP(sks::launch_cluster_link(cnt, tiles + 2 * r.begin, nt, S.n, S.sizes, min_containment, min_shared, stat,
                                     parent, c->stream));
  }
  SKS_HIP(sks::launch_cluster_number(parent, S.sizes, S.n, r_root.in(w), r_key.in(w), r_id.in(w), r_chunk.in(w),
                                     stat + 2, d_cluster, d_rep, c->stream));
  // the layout's status and the number of clusters (one wait)
  uint32_t h_stat[4] = {0, 0, 0, 0};
  SKS_HIP(sks::pinned_d2h(h_stat, stat, sizeof h_stat, c->stream));
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  if (h_stat[1]) return fail_invalid_layout(me, "the set", "nothing is linked", invalid_layout);
  *n_clusters = h_stat[2];
  return SKS_OK;
}

}  // namespace

extern "C" {

int sks_cluster(sks_ctx* c, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes, uint32_t n,
                uint32_t max_size, uint64_t total, int elem_words, int kmer_num_ones, double min_containment,
                int32_t min_shared, uint32_t* d_cluster, uint32_t* d_rep, uint32_t* n_clusters) {
  if (n_clusters) *n_clusters = 0;
  if (!c) return sks::fail(SKS_E_ARG, "sks_cluster: null ctx");
  if (!n_clusters) return sks::fail(SKS_E_ARG, "sks_cluster: null n_clusters");
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_cluster: kmer_num_ones must be positive");
  if (!(min_containment == min_containment)) return sks::fail(SKS_E_ARG, "sks_cluster: min_containment is NaN");
  if (n && (!d_starts || !d_sizes)) return sks::fail(SKS_E_ARG, "sks_cluster: null argument");
  SKS_TRY(check_span_totals("sks_cluster", "in the set", total));
  const SketchSpan S{d_data, d_starts, d_sizes, n, max_size, total, nullptr};
  return cluster_core(c, "sks_cluster", S, elem_words, min_containment, min_shared, nullptr, d_cluster, d_rep,
                      n_clusters);
}

int sks_cluster_set(sks_ctx* c, const sks_sketch_set* set, double min_containment, int32_t min_shared,
                    uint32_t* d_cluster, uint32_t* d_rep, uint32_t* n_clusters) {
  if (n_clusters) *n_clusters = 0;
  if (!c) return sks::fail(SKS_E_ARG, "sks_cluster_set: null ctx");
  if (!set || !n_clusters) return sks::fail(SKS_E_ARG, "sks_cluster_set: null argument");
  if (!(min_containment == min_containment)) return sks::fail(SKS_E_ARG, "sks_cluster_set: min_containment is NaN");
  if (set->device != c->device)
    return sks::fail(SKS_E_ARG, "sks_cluster_set: the set lives on another device than the context");
  const SketchSpan S = span_of(set);
  SKS_TRY(check_span_totals("sks_cluster_set", "in the set", S.total));
  if (S.n == 0) return SKS_OK;
  // the mask's group bounds; sampled from the set if they cannot place the layout
  std::vector<uint64_t> mask_bounds;
  SKS_TRY(mask_group_bounds(set->mask, set->elem_words, S.max_size, &mask_bounds));
  return with_mask_bounds_retry(mask_bounds, [&](const std::vector<uint64_t>* h_bounds, bool* invalid) {
    return cluster_core(c, "sks_cluster_set", S, set->elem_words, min_containment, min_shared, h_bounds, d_cluster,
                        d_rep, n_clusters, invalid);
  });
}

}  // extern "C"
