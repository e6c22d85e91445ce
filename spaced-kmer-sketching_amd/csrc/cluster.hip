// Single-linkage clusters of a sketch set, formed on the device from the
// packed 64 x 64 count tiles of the set joined with itself.
//
// The set's clusters at a containment threshold are the connected components of
// the graph whose edges are the pairs passing the link rule (cluster_plan.hpp).
// k_cluster_link reads each tile of the upper triangle once and, for every
// linking cell, unites the two sketches in a parent array by hooking the larger
// root under the smaller with one atomicCAS (cluster_unite): memory is n words,
// whatever the number of links, and no hit list exists.
//
// Visibility.  The workgroups of the link launch run on every XCD; the XCDs'
// L2s are not coherent with each other and a CU's L1 is never refreshed by
// another CU's stores.  The union therefore rests on its atomics alone:
// parent[x] is written only by atomicCAS(&parent[x], x, smaller), so it changes
// once; there is no path compression and no plain store to `parent` in the
// link kernel; reads of `parent` are relaxed agent-scope atomic loads (they
// bypass the L1); and when a compare-and-swap fails the walk goes on from the
// value it returned.  A stale load can only show x as its own parent after it
// stopped being one, which costs a failed compare-and-swap, never a wrong link
// or an endless loop (every retry moves strictly downward).
//
// The numbering kernels run as separate launches, after which every link is
// visible to plain loads: roots by walking `parent`, the representative of a
// root by atomicMax of (size << 32 | ~index), ids by an exclusive scan of the
// root marks (per-chunk sums, then each chunk adds the sums before it).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cluster.hpp"
#include "cluster_plan.hpp"
#include "code_objects.hpp"
#include "wave_prims.hpp"

namespace sks {

namespace {

constexpr int kCB = 256;                  // threads per workgroup: 4 wavefronts
constexpr int kTile = 64;
constexpr int kRows = kTile / (kCB / 64);  // tile rows per wavefront
static_assert(kClusterChunk == (uint32_t)kCB, "one sketch per thread of a numbering workgroup");

struct DeviceParentOps {
  __device__ __forceinline__ uint32_t load(const uint32_t* p) const {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expected, uint32_t desired) const {
    return atomicCAS(p, expected, desired);
  }
};

__global__ __launch_bounds__(kCB) void k_cluster_init(uint32_t* __restrict__ parent,
                                                      unsigned long long* __restrict__ key, uint32_t n) {
  const uint32_t i = blockIdx.x * kCB + threadIdx.x;
  if (i >= n) return;
  parent[i] = i;
  key[i] = 0;
}

// A workgroup per tile, a wavefront per 16 rows, lanes along the row (each load
// is one contiguous 256-byte row of the tile), as k_search_hits.  Every linking
// cell unites its row and column sketch; cluster_unite first finds both roots,
// so a cell whose sketches are already in one component issues no atomic.
__global__ __launch_bounds__(kCB) void k_cluster_link(const int32_t* __restrict__ packed,
                                                      const uint32_t* __restrict__ tiles, uint32_t n,
                                                      const uint32_t* __restrict__ sizes, double min_containment,
                                                      int32_t min_shared, const uint32_t* __restrict__ stat,
                                                      uint32_t* parent) {
  if (stat[1]) return;  // an invalid layout's counts are not counts
  const uint32_t t = blockIdx.x, I = tiles[2 * t], J = tiles[2 * t + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t col = J * kTile + lane;
  const bool col_ok = col < n;
  const uint32_t col_size = col_ok ? sizes[col] : 0;
  const int32_t* tile = packed + (uint64_t)t * (kTile * kTile);
  const DeviceParentOps ops;
  for (int i = 0; i < kRows; ++i) {
    const uint32_t r = wave * kRows + i, row = I * kTile + r;
    if (row >= n) break;  // uniform over the wavefront
    const int32_t cnt = tile[r * kTile + lane];
    // above the diagonal only: a diagonal tile holds both (i, j) and (j, i)
    if (col_ok && col > row && cluster_linked(cnt, sizes[row], col_size, min_containment, min_shared))
      cluster_unite(ops, parent, row, col);
  }
}

// root[i], the representative key of each root, the roots per chunk
__global__ __launch_bounds__(kCB) void k_cluster_flatten(const uint32_t* __restrict__ parent,
                                                         const uint32_t* __restrict__ sizes, uint32_t n,
                                                         uint32_t* __restrict__ root,
                                                         unsigned long long* __restrict__ key,
                                                         uint32_t* __restrict__ chunk_roots) {
  __shared__ uint32_t wsum[kCB / 64];
  const uint32_t i = blockIdx.x * kCB + threadIdx.x;
  bool is_root = false;
  if (i < n) {
    uint32_t x = i;
    for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
    root[i] = x;
    is_root = x == i;
    atomicMax(&key[x], ((unsigned long long)sizes[i] << 32) | (uint32_t)~i);
  }
  uint32_t total;
  (void)block_rank<kCB / 64>(is_root, wsum, &total);
  if (threadIdx.x == 0) chunk_roots[blockIdx.x] = total;
}

// id[i] of every root i = the roots before it; the last chunk leaves the total
__global__ __launch_bounds__(kCB) void k_cluster_ids(const uint32_t* __restrict__ root,
                                                     const uint32_t* __restrict__ chunk_roots, uint32_t n,
                                                     uint32_t* __restrict__ id, uint32_t* __restrict__ n_clusters) {
  __shared__ uint32_t wsum[kCB / 64], wbase[kCB / 64];
  // the roots of the chunks before this one: a strided partial sum per thread, then a workgroup sum
  uint32_t part = 0;
  for (uint32_t w = threadIdx.x; w < blockIdx.x; w += kCB) part += chunk_roots[w];
  uint32_t base;
  (void)block_excl_scan<kCB / 64>(part, wbase, &base);
  const uint32_t i = blockIdx.x * kCB + threadIdx.x;
  const bool is_root = i < n && root[i] == i;
  uint32_t total;
  const uint32_t rank = block_rank<kCB / 64>(is_root, wsum, &total);
  if (is_root) id[i] = base + rank;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_clusters = base + total;
}

__global__ __launch_bounds__(kCB) void k_cluster_labels(const uint32_t* __restrict__ root,
                                                        const unsigned long long* __restrict__ key,
                                                        const uint32_t* __restrict__ id, uint32_t n,
                                                        uint32_t* __restrict__ d_cluster,
                                                        uint32_t* __restrict__ d_rep) {
  const uint32_t i = blockIdx.x * kCB + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = root[i];
  if (d_cluster) d_cluster[i] = id[x];
  if (d_rep && x == i) d_rep[id[i]] = ~(uint32_t)key[i];
}

}  // namespace

hipError_t launch_cluster_init(uint32_t* parent, unsigned long long* key, uint32_t n, hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_cluster_init, dim3((n + kCB - 1) / kCB), dim3(kCB), 0, s, parent, key, n);
  return hipGetLastError();
}

hipError_t launch_cluster_link(const int32_t* packed, const uint32_t* tiles, uint64_t n_tiles, uint32_t n,
                               const uint32_t* sizes, double min_containment, int32_t min_shared,
                               const uint32_t* stat, uint32_t* parent, hipStream_t s) {
  if (!n_tiles) return hipSuccess;
  if (n_tiles > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cluster_link, dim3((unsigned)n_tiles), dim3(kCB), 0, s, packed, tiles, n, sizes,
                     min_containment, min_shared, stat, parent);
  return hipGetLastError();
}

hipError_t launch_cluster_number(const uint32_t* parent, const uint32_t* sizes, uint32_t n, uint32_t* root,
                                 unsigned long long* key, uint32_t* id, uint32_t* chunk_roots,
                                 uint32_t* n_clusters, uint32_t* d_cluster, uint32_t* d_rep, hipStream_t s) {
  if (!n) return hipSuccess;
  const dim3 grid((n + kCB - 1) / kCB), block(kCB);
  hipLaunchKernelGGL(k_cluster_flatten, grid, block, 0, s, parent, sizes, n, root, key, chunk_roots);
  hipLaunchKernelGGL(k_cluster_ids, grid, block, 0, s, root, chunk_roots, n, id, n_clusters);
  if (d_cluster || d_rep) hipLaunchKernelGGL(k_cluster_labels, grid, block, 0, s, root, key, id, n, d_cluster, d_rep);
  return hipGetLastError();
}

SKS_CODE_OBJECT_HOOK(cluster)

}  // namespace sks
