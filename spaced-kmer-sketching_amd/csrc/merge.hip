// Grouped unions of sketches (sks_sketch_set_merge): the members of a group are
// sorted runs, so the union is a k-way merge, not a sort.
//
// k_merge_round merges adjacent runs pairwise.  A workgroup owns one tile of
// kMergeTile consecutive outputs of one pair: two merge-path searches on the
// tile's diagonals (merge_plan.hpp, the code the CPU test runs) give the two
// input ranges, which are staged in LDS; every thread then finds the inputs of
// its four consecutive outputs by the same search in LDS, merges them, and the
// tile leaves through LDS again so the global stores are contiguous.  The runs
// come as absolute addresses: round 0 reads the source sets where they lie.
//
// k_mu_count / k_mu_scatter drop the duplicates of the fully merged groups with
// the count -> scan -> scatter shape of downsample.hip (the scan and the new
// starts and sizes are downsample_offsets): an element stays iff it differs
// from its predecessor, the first of a tile reading the last of the tile before
// it from global memory.  No atomics: the output order is the input order.
#include <hip/hip_runtime.h>

#include "code_objects.hpp"
#include "downsample.hpp"
#include "merge.hpp"
#include "merge_device.hpp"

namespace sks {

SKS_CODE_OBJECT_HOOK(merge)

namespace {

static_assert(kMergeTile == kDownsampleChunk, "the duplicate filter's chunks are counted by downsample_offsets");

template <int EW>
struct Reader {
  const typename MElem<EW>::type* p;
  __device__ __forceinline__ typename MElem<EW>::type operator()(uint32_t i) const { return p[i]; }
};
template <int EW>
struct Less {
  __device__ __forceinline__ bool operator()(typename MElem<EW>::type x, typename MElem<EW>::type y) const {
    return MElem<EW>::less(x, y);
  }
};

template <int EW>
__global__ __launch_bounds__(kMgB) void k_merge_round(const uint64_t* __restrict__ pairs,
                                                      const uint64_t* __restrict__ tile_off, uint32_t n_pairs) {
  using T = typename MElem<EW>::type;
  __shared__ T tile[kMergeTile];
  __shared__ uint32_t cut[2];
  const uint32_t p = tile_owner(tile_off, n_pairs, blockIdx.x);
  const uint64_t* pd = pairs + 4 * (uint64_t)p;
  const T* A = reinterpret_cast<const T*>(pd[0]);
  const T* B = reinterpret_cast<const T*>(pd[1]);
  T* out = reinterpret_cast<T*>(pd[2]);
  const uint32_t na = (uint32_t)pd[3], nb = (uint32_t)(pd[3] >> 32);
  const uint32_t n = na + nb;  // < 2^32 (checked on the host)
  const uint32_t d0 = (uint32_t)(blockIdx.x - tile_off[p]) * kMergeTile;
  const uint32_t m = n - d0 < kMergeTile ? n - d0 : kMergeTile;  // outputs of this tile
  // the two diagonals, one wave each
  if ((threadIdx.x & 63) == 0 && threadIdx.x < 128) {
    const uint32_t d = threadIdx.x == 0 ? d0 : d0 + m;
    cut[threadIdx.x >> 6] = merge_path(Reader<EW>{A}, na, Reader<EW>{B}, nb, d, Less<EW>{});
  }
  __syncthreads();
  const uint32_t a0 = cut[0], la = cut[1] - a0, b0 = d0 - a0, lb = m - la;
  for (uint32_t i = threadIdx.x; i < m; i += kMgB) tile[i] = i < la ? A[a0 + i] : B[b0 + (i - la)];
  __syncthreads();
  // this thread's outputs [q0, q0 + kMgItems) of the tile
  const uint32_t q0 = threadIdx.x * kMgItems < m ? threadIdx.x * kMgItems : m;
  uint32_t i = merge_path(Reader<EW>{tile}, la, Reader<EW>{tile + la}, lb, q0, Less<EW>{});
  uint32_t j = q0 - i;
  T r[kMgItems];
#pragma unroll
  for (int k = 0; k < kMgItems; ++k) {
    r[k] = T{};
    if (q0 + k < m) {
      const bool left = j >= lb || (i < la && !MElem<EW>::less(tile[la + j], tile[i]));
      r[k] = left ? tile[i] : tile[la + j];
      i += left ? 1u : 0u;
      j += left ? 0u : 1u;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kMgItems; ++k)
    if (q0 + k < m) tile[q0 + k] = r[k];
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < m; t += kMgB) out[(uint64_t)d0 + t] = tile[t];
}

// An element stays iff it is the first of its value in its group.
template <int EW>
struct FirstOfValue {
  GroupChunk<EW> ch;
  __device__ __forceinline__ bool operator()(uint64_t i, typename MElem<EW>::type& v) const {
    return ch.first_of_value(i, v);
  }
};

template <int EW>
__global__ __launch_bounds__(kMgB) void k_mu_count(const uint64_t* __restrict__ runs,
                                                   const uint64_t* __restrict__ chunk_off, uint32_t n_groups,
                                                   uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kMgWaves];
  FirstOfValue<EW> keep;
  keep.ch.open(runs, chunk_off, n_groups);
  chunk_count<EW>(keep.ch.base, keep, wsum, counts);
}

template <int EW>
__global__ __launch_bounds__(kMgB) void k_mu_scatter(const uint64_t* __restrict__ runs,
                                                     const uint64_t* __restrict__ chunk_off, uint32_t n_groups,
                                                     const uint64_t* __restrict__ offs,
                                                     uint64_t* __restrict__ out_words) {
  using T = typename MElem<EW>::type;
  __shared__ uint32_t wsum[kMgItems * kMgWaves];
  FirstOfValue<EW> keep;
  keep.ch.open(runs, chunk_off, n_groups);
  T* out = reinterpret_cast<T*>(out_words) + offs[blockIdx.x];
  chunk_scatter<EW>(keep.ch.base, keep, wsum, [out](uint32_t rank, uint64_t, T v) { out[rank] = v; });
}

}  // namespace

hipError_t merge_round(const uint64_t* pairs, const uint64_t* tile_off, uint32_t n_pairs, uint64_t n_tiles, int ew,
                       hipStream_t s) {
  if (n_pairs == 0 || n_tiles == 0) return hipSuccess;
  if (n_tiles > kMgMaxGrid) return hipErrorInvalidValue;
  if (ew == 1)
    hipLaunchKernelGGL(k_merge_round<1>, dim3((unsigned)n_tiles), dim3(kMgB), 0, s, pairs, tile_off, n_pairs);
  else
    hipLaunchKernelGGL(k_merge_round<2>, dim3((unsigned)n_tiles), dim3(kMgB), 0, s, pairs, tile_off, n_pairs);
  return hipGetLastError();
}

hipError_t merge_unique_count(const uint64_t* runs, const uint64_t* chunk_off, uint32_t n_groups, uint64_t n_chunks,
                              int ew, uint32_t* counts, hipStream_t s) {
  if (n_groups == 0 || n_chunks == 0) return hipSuccess;
  if (n_chunks > kMgMaxGrid) return hipErrorInvalidValue;
  if (ew == 1)
    hipLaunchKernelGGL(k_mu_count<1>, dim3((unsigned)n_chunks), dim3(kMgB), 0, s, runs, chunk_off, n_groups, counts);
  else
    hipLaunchKernelGGL(k_mu_count<2>, dim3((unsigned)n_chunks), dim3(kMgB), 0, s, runs, chunk_off, n_groups, counts);
  return hipGetLastError();
}

hipError_t merge_unique_scatter(const uint64_t* runs, const uint64_t* chunk_off, uint32_t n_groups,
                                uint64_t n_chunks, int ew, const uint64_t* offs, uint64_t* out, hipStream_t s) {
  if (n_groups == 0 || n_chunks == 0) return hipSuccess;
  if (n_chunks > kMgMaxGrid) return hipErrorInvalidValue;
  if (ew == 1)
    hipLaunchKernelGGL(k_mu_scatter<1>, dim3((unsigned)n_chunks), dim3(kMgB), 0, s, runs, chunk_off, n_groups, offs,
                       out);
  else
    hipLaunchKernelGGL(k_mu_scatter<2>, dim3((unsigned)n_chunks), dim3(kMgB), 0, s, runs, chunk_off, n_groups, offs,
                       out);
  return hipGetLastError();
}

}  // namespace sks
