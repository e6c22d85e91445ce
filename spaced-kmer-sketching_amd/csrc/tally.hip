// Grouped tallies of sketches (sks_sketch_set_tally): the values held by
// lo .. hi of a group's members.  merge.hip's rounds leave every group as one
// sorted run in which a value appears once per member that holds it;
// k_tally_count / k_tally_scatter are k_mu_count / k_mu_scatter with another
// keep rule (merge_device.hpp has the chunk, the ballots and the ranks): an
// element stays iff it is the first of its value and the two reads of
// tally_keeps (tally_plan.hpp, the code the CPU test runs) find the value at
// position i + lo - 1 and not at i + hi.  Those reads lie at most hi elements
// ahead, mostly in lines the chunk reads anyway, and are plain global loads.
// With a multiplicity array the scatter bisects for the end of each kept value's
// run (tally_run_length).  Every position is 64-bit and below the group's own
// length: the next group's run, or the source set's next sketch, lies right
// behind and may start with the same value.  No atomics: the output order is
// the input order.
#include <hip/hip_runtime.h>

#include "code_objects.hpp"
#include "downsample.hpp"
#include "merge_device.hpp"
#include "tally.hpp"

namespace sks {

SKS_CODE_OBJECT_HOOK(tally)

namespace {

static_assert(kMergeTile == kDownsampleChunk, "the tally's chunks are counted by downsample_offsets");

template <int EW>
struct At {
  const typename MElem<EW>::type* p;
  __device__ __forceinline__ typename MElem<EW>::type operator()(uint64_t i) const { return p[i]; }
};
template <int EW>
struct Same {
  __device__ __forceinline__ bool operator()(typename MElem<EW>::type x, typename MElem<EW>::type y) const {
    return MElem<EW>::same(x, y);
  }
};

// An element stays iff it heads a run of lo .. hi equal values of its group.
template <int EW>
struct HeldByLoToHi {
  GroupChunk<EW> ch;
  uint32_t lo, hi, m;
  __device__ __forceinline__ void open(const uint64_t* runs, const uint64_t* chunk_off, const uint64_t* limits,
                                       uint32_t n_groups) {
    ch.open(runs, chunk_off, n_groups);
    const uint64_t l = limits[2 * (uint64_t)ch.g];
    lo = (uint32_t)l;
    hi = (uint32_t)(l >> 32);
    m = (uint32_t)limits[2 * (uint64_t)ch.g + 1];
  }
  __device__ __forceinline__ bool operator()(uint64_t i, typename MElem<EW>::type& v) const {
    if (i >= ch.size) return false;
    return tally_keeps(At<EW>{ch.src}, Same<EW>{}, i, ch.size, lo, hi, &v);
  }
  __device__ __forceinline__ uint32_t occurrences(uint64_t i, typename MElem<EW>::type v) const {
    return tally_run_length(At<EW>{ch.src}, Same<EW>{}, v, i, ch.size, lo, hi, m);
  }
};

template <int EW>
__global__ __launch_bounds__(kMgB) void k_tally_count(const uint64_t* __restrict__ runs,
                                                      const uint64_t* __restrict__ chunk_off,
                                                      const uint64_t* __restrict__ limits, uint32_t n_groups,
                                                      uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kMgWaves];
  HeldByLoToHi<EW> keep;
  keep.open(runs, chunk_off, limits, n_groups);
  chunk_count<EW>(keep.ch.base, keep, wsum, counts);
}

template <int EW, bool MULT>
__global__ __launch_bounds__(kMgB) void k_tally_scatter(const uint64_t* __restrict__ runs,
                                                        const uint64_t* __restrict__ chunk_off,
                                                        const uint64_t* __restrict__ limits, uint32_t n_groups,
                                                        const uint64_t* __restrict__ offs,
                                                        uint64_t* __restrict__ out_words,
                                                        uint32_t* __restrict__ mult_all) {
  using T = typename MElem<EW>::type;
  __shared__ uint32_t wsum[kMgItems * kMgWaves];
  HeldByLoToHi<EW> keep;
  keep.open(runs, chunk_off, limits, n_groups);
  T* out = reinterpret_cast<T*>(out_words) + offs[blockIdx.x];
  uint32_t* mult = MULT ? mult_all + offs[blockIdx.x] : nullptr;
  chunk_scatter<EW>(keep.ch.base, keep, wsum, [&](uint32_t rank, uint64_t i, T v) {
    out[rank] = v;
    if (MULT) mult[rank] = keep.occurrences(i, v);
  });
}

}  // namespace

hipError_t tally_count(const uint64_t* runs, const uint64_t* chunk_off, const uint64_t* limits, uint32_t n_groups,
                       uint64_t n_chunks, int ew, uint32_t* counts, hipStream_t s) {
  if (n_groups == 0 || n_chunks == 0) return hipSuccess;
  if (n_chunks > kMgMaxGrid) return hipErrorInvalidValue;
  const dim3 grid((unsigned)n_chunks), block(kMgB);
  if (ew == 1)
    hipLaunchKernelGGL(k_tally_count<1>, grid, block, 0, s, runs, chunk_off, limits, n_groups, counts);
  else
    hipLaunchKernelGGL(k_tally_count<2>, grid, block, 0, s, runs, chunk_off, limits, n_groups, counts);
  return hipGetLastError();
}

hipError_t tally_scatter(const uint64_t* runs, const uint64_t* chunk_off, const uint64_t* limits, uint32_t n_groups,
                         uint64_t n_chunks, int ew, const uint64_t* offs, uint64_t* out, uint32_t* mult,
                         hipStream_t s) {
  if (n_groups == 0 || n_chunks == 0) return hipSuccess;
  if (n_chunks > kMgMaxGrid) return hipErrorInvalidValue;
  const dim3 grid((unsigned)n_chunks), block(kMgB);
#define SKS_TALLY_SCATTER(EW, MULT) \
  hipLaunchKernelGGL((k_tally_scatter<EW, MULT>), grid, block, 0, s, runs, chunk_off, limits, n_groups, offs, out, mult)
  if (ew == 1 && mult)
    SKS_TALLY_SCATTER(1, true);
  else if (ew == 1)
    SKS_TALLY_SCATTER(1, false);
  else if (mult)
    SKS_TALLY_SCATTER(2, true);
  else
    SKS_TALLY_SCATTER(2, false);
#undef SKS_TALLY_SCATTER
  return hipGetLastError();
}

}  // namespace sks
