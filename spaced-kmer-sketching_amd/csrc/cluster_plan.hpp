// The arithmetic of sks_cluster (no HIP: tests/cpp/cluster_plan_test.cpp runs it
// on any machine, and cluster.hip runs the same functions on the device): the
// link rule, the triangle tiles and their batch ranges, and the lock-free
// union by index the link kernel forms its components with.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SKS_PLAN_HD __host__ __device__
#else
#define SKS_PLAN_HD
#endif

namespace sks {

// ---- the link rule -----------------------------------------------------------------------
// containment_of (sks_ani.hpp), restated without HIP: the same double division
SKS_PLAN_HD inline double cluster_containment(int32_t shared, int32_t size_first) {
  return shared == 0 ? 0.0 : (double)shared / (double)size_first;
}

// Sketches of size_i and size_j elements sharing `shared` of them are linked iff
// shared >= max(min_shared, 1) and the larger of the two containments reaches
// min_containment: what sks_search_sets(set, set) reports as (i, j) or (j, i).
SKS_PLAN_HD inline bool cluster_linked(int32_t shared, uint32_t size_i, uint32_t size_j, double min_containment,
                                       int32_t min_shared) {
  if (shared < (min_shared < 1 ? 1 : min_shared)) return false;
  const double ci = cluster_containment(shared, (int32_t)size_i), cj = cluster_containment(shared, (int32_t)size_j);
  return (ci > cj ? ci : cj) >= min_containment;
}

// ---- triangle tiles ----------------------------------------------------------------------
// The tiles (I, J), I <= J, of nb 64-sketch blocks, column by column: tile
// J * (J + 1) / 2 + I.  A batch is `bb` whole columns, so its tiles are one range.
SKS_PLAN_HD inline uint64_t cluster_tiles_before(uint64_t J) { return J * (J + 1) / 2; }

inline uint32_t cluster_batches(uint32_t nb, uint32_t bb) { return (nb + bb - 1) / bb; }

struct ClusterRange {
  uint64_t begin, end;
};
// the tiles of batch b: columns [b * bb, min(nb, (b + 1) * bb))
inline ClusterRange cluster_batch_range(uint32_t nb, uint32_t bb, uint32_t b) {
  const uint64_t j0 = (uint64_t)b * bb, j1 = j0 + bb < nb ? j0 + bb : nb;
  return {cluster_tiles_before(j0), cluster_tiles_before(j1)};
}

// the (I, J) list of every tile, in tile order (2 words a tile)
inline std::vector<uint32_t> cluster_tile_list(uint32_t nb) {
  std::vector<uint32_t> t;
  t.reserve((size_t)cluster_tiles_before(nb) * 2);
  for (uint32_t J = 0; J < nb; ++J)
    for (uint32_t I = 0; I <= J; ++I) {
      t.push_back(I);
      t.push_back(J);
    }
  return t;
}

// ---- union by index ----------------------------------------------------------------------
// parent[x] <= x, parent[x] == x: x is a root.  parent[x] changes once, from x to
// something smaller, and only by unite's compare-and-swap: a parent is smaller
// than its child, chains end, and a component's root is its smallest member.
// Ops supplies the two memory operations (device: relaxed agent-scope atomics;
// host: the same on std::atomic or the compiler's atomic builtins): load(p) and cas(p, expected, desired) returning
// the value found.  A load may be stale (it then shows x where parent[x] has
// already moved): the walk stops early at a node that is no root any more, the
// compare-and-swap on it fails and hands back the true parent, and the walk
// goes on from there.  Nothing is decided on a plain read.
template <class Ops>
SKS_PLAN_HD inline uint32_t cluster_find(const Ops& ops, uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = ops.load(parent + x);
    if (p == x) return x;
    x = p;
  }
}

template <class Ops>
SKS_PLAN_HD inline void cluster_unite(const Ops& ops, uint32_t* parent, uint32_t a, uint32_t b) {
  a = cluster_find(ops, parent, a);
  b = cluster_find(ops, parent, b);
  while (a != b) {
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t was = ops.cas(parent + hi, hi, lo);
    if (was == hi) return;  // hi was a root and now hangs under lo
    // hi already has a parent `was` < hi: go on from it; max(a, b) falls every round
    a = cluster_find(ops, parent, was);
    b = lo;
  }
}

}  // namespace sks
