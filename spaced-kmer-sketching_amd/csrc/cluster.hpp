// Single-linkage clusters from count tiles (cluster.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sks {

constexpr uint32_t kClusterChunk = 256;  // sketches per workgroup of the numbering kernels

// parent[i] = i, key[i] = 0 for i < n.
hipError_t launch_cluster_init(uint32_t* parent, unsigned long long* key, uint32_t n, hipStream_t s);
// Links of n_tiles packed count tiles: tile t is `packed`[t][64][64] for the
// blocks (I, J) = tiles[2 t], tiles[2 t + 1], I <= J, rows = block I.  Cell
// (i, j) with i < j < n whose count and the two sizes satisfy cluster_linked
// (cluster_plan.hpp) unites i and j in `parent`; a diagonal tile's lower
// triangle and its cells (i, i) are skipped.  stat: the layout's status words;
// a non-zero word 1 (invalid layout) makes the launch a no-op.
hipError_t launch_cluster_link(const int32_t* packed, const uint32_t* tiles, uint64_t n_tiles, uint32_t n,
                               const uint32_t* sizes, double min_containment, int32_t min_shared,
                               const uint32_t* stat, uint32_t* parent, hipStream_t s);
// After every link launch: root[i] = the root of i, key[root] = the largest
// (sizes[i] << 32 | ~i) of its members, chunk_roots[w] = the roots among the
// sketches [w * kClusterChunk, ...); then ids in root order (the exclusive scan
// of the root marks, chunk sums first), *n_clusters (device) = their number,
// d_cluster[i] = id[root[i]] and d_rep[id] = ~(uint32_t)key[root] (either may be
// null).  Three launches; scratch arrays of n words (key: n u64) and
// ceil(n / kClusterChunk) chunk words.
hipError_t launch_cluster_number(const uint32_t* parent, const uint32_t* sizes, uint32_t n, uint32_t* root,
                                 unsigned long long* key, uint32_t* id, uint32_t* chunk_roots,
                                 uint32_t* n_clusters, uint32_t* d_cluster, uint32_t* d_rep, hipStream_t s);

}  // namespace sks
