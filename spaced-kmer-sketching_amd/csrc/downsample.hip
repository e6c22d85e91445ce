// Downsampling of a device sketch set (sks_sketch_set_downsample): an
// order-preserving segmented filter over the set's CSR arrays.
//
// A sketch's elements are its masked canonical k-mers in ascending order, and
// frac_min_hash is a function of the element and the set's (mask, window, nonce,
// flavour), so the elements a coarser parameter keeps are decided from the
// sketch alone: FracMinHash keeps x iff fmh(x) % c' == 0; bottom-s' keeps the
// s' elements smallest by (fmh, k-mer), marked beforehand in a flag array.
//
// Every workgroup owns one chunk of kDownsampleChunk consecutive elements of
// one sketch, on a (chunk, sketch) grid.  Pass 1 (k_ds_count) counts the kept
// elements of each chunk; an exclusive scan over the chunk counts gives every
// chunk's output offset and, read at the sketch boundaries, every sketch's new
// start and size (k_ds_meta); pass 2 (k_ds_scatter) recomputes the predicate
// and stores the kept elements at offset + rank, the rank from wave ballots and
// a per-wave prefix in LDS.  No atomics: the output is the input order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <type_traits>

#include "code_objects.hpp"
#include "downsample.hpp"
#include "sks_hash.hpp"

namespace sks {

SKS_CODE_OBJECT_HOOK(downsample)

namespace {

constexpr int kDsB = 256;
constexpr int kDsWaves = kDsB / 64;
constexpr int kDsItems = (int)kDownsampleChunk / kDsB;  // elements per thread, striped by kDsB
constexpr uint32_t kDsMaxGridY = 65535;
static_assert(kDsItems * kDsB == (int)kDownsampleChunk, "chunk is a whole number of block strides");

// One element: a u64 (narrow) or a 16-byte (lo, hi) pair (wide), moved whole.
template <int EW>
struct Elem;
template <>
struct Elem<1> {
  using type = uint64_t;
  static __device__ __forceinline__ uint64_t lo(type v) { return v; }
  static __device__ __forceinline__ uint64_t hi(type) { return 0; }
};
template <>
struct Elem<2> {
  using type = ulong2;
  static __device__ __forceinline__ uint64_t lo(type v) { return v.x; }
  static __device__ __forceinline__ uint64_t hi(type v) { return v.y; }
};

template <int EW, int FLAVOUR>
__device__ __forceinline__ uint64_t fmh_of(typename Elem<EW>::type v, uint64_t kconst) {
  return hash_bitset128<FLAVOUR>(Elem<EW>::lo(v), Elem<EW>::hi(v)) ^ kconst;
}

// Whether element `v`, the `dense`-th of the set, stays.
template <int EW, int FLAVOUR, int MODE>
__device__ __forceinline__ bool keeps(const DownsampleArgs& a, typename Elem<EW>::type v, uint64_t dense) {
  if constexpr (MODE == kDownsampleFrac)
    return div_test(fmh_of<EW, FLAVOUR>(v, a.kconst), a.low_mask, a.high_mask, a.dinv, a.dlim);
  else if constexpr (MODE == kDownsampleFlag)
    return a.keep_flag[dense] != 0;
  else
    return true;
}

// The chunk of this workgroup: sketch g, its elements [base, size) from
// src[0 ..), dense index of src[0].  False: the chunk lies beyond the sketch.
template <int EW>
struct Chunk {
  const typename Elem<EW>::type* src;
  uint64_t size, base, dense0;
  uint32_t g;
  __device__ __forceinline__ bool open(const DownsampleArgs& a) {
    g = a.g0 + blockIdx.y;
    size = a.sizes[g];
    base = (uint64_t)blockIdx.x * kDownsampleChunk;
    if (base >= size) return false;
    src = reinterpret_cast<const typename Elem<EW>::type*>(a.data) + a.starts[g];
    dense0 = a.dense_off ? a.dense_off[g] : 0;
    return true;
  }
};

template <int EW, int FLAVOUR, int MODE>
__global__ __launch_bounds__(kDsB) void k_ds_count(const DownsampleArgs a, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kDsWaves];
  Chunk<EW> ch;
  if (!ch.open(a)) return;  // the whole workgroup
  uint32_t cnt = 0;         // of this wave
#pragma unroll
  for (int j = 0; j < kDsItems; ++j) {
    const uint64_t i = ch.base + (uint64_t)j * kDsB + threadIdx.x;
    bool p = false;
    if (i < ch.size) {
      typename Elem<EW>::type v{};
      if constexpr (MODE == kDownsampleFrac) v = ch.src[i];
      p = keeps<EW, FLAVOUR, MODE>(a, v, ch.dense0 + i);
    }
    cnt += (uint32_t)__popcll(__ballot(p));
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t all = 0;
#pragma unroll
    for (int w = 0; w < kDsWaves; ++w) all += wsum[w];
    counts[a.chunk_off[ch.g] + blockIdx.x] = all;
  }
}

template <int EW, int FLAVOUR, int MODE>
__global__ __launch_bounds__(kDsB) void k_ds_scatter(const DownsampleArgs a, const uint64_t* __restrict__ offs,
                                                     uint64_t* __restrict__ out_words) {
  using T = typename Elem<EW>::type;
  __shared__ uint32_t wsum[kDsItems * kDsWaves];  // kept per (stride j, wave), in element order
  Chunk<EW> ch;
  if (!ch.open(a)) return;  // the whole workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T v[kDsItems];
  bool p[kDsItems];
  uint32_t in_wave[kDsItems];
#pragma unroll
  for (int j = 0; j < kDsItems; ++j) {
    const uint64_t i = ch.base + (uint64_t)j * kDsB + threadIdx.x;
    v[j] = T{};
    p[j] = false;
    if (i < ch.size) {
      v[j] = ch.src[i];
      p[j] = keeps<EW, FLAVOUR, MODE>(a, v[j], ch.dense0 + i);
    }
    const uint64_t bal = __ballot(p[j]);
    in_wave[j] = (uint32_t)__popcll(bal & ((1ull << lane) - 1));
    if (lane == 0) wsum[j * kDsWaves + wave] = (uint32_t)__popcll(bal);
  }
  __syncthreads();
  T* out = reinterpret_cast<T*>(out_words) + offs[a.chunk_off[ch.g] + blockIdx.x];
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < kDsItems; ++j) {
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < kDsWaves; ++w) {
      if (w == wave) before = run;
      run += wsum[j * kDsWaves + w];
    }
    if (p[j]) out[before + in_wave[j]] = v[j];
  }
}

// starts[g], sizes[g] of the filtered set from the scanned chunk counts.
__global__ void k_ds_meta(const uint64_t* __restrict__ offs, const uint64_t* __restrict__ chunk_off, uint32_t n,
                          uint64_t* __restrict__ starts, uint32_t* __restrict__ sizes) {
  const uint32_t g = blockIdx.x * kDsB + threadIdx.x;
  if (g >= n) return;
  const uint64_t b = offs[chunk_off[g]], e = offs[chunk_off[g + 1]];
  starts[g] = b;
  sizes[g] = (uint32_t)(e - b);
}

// Bottom-s: fmh[d] = frac_min_hash of the set's d-th element, idx[d] = d.
template <int EW, int FLAVOUR>
__global__ __launch_bounds__(kDsB) void k_ds_fmh(const DownsampleArgs a, uint64_t* __restrict__ fmh,
                                                 uint64_t* __restrict__ idx) {
  Chunk<EW> ch;
  if (!ch.open(a)) return;
#pragma unroll
  for (int j = 0; j < kDsItems; ++j) {
    const uint64_t i = ch.base + (uint64_t)j * kDsB + threadIdx.x;
    if (i < ch.size) {
      fmh[ch.dense0 + i] = fmh_of<EW, FLAVOUR>(ch.src[i], a.kconst);
      idx[ch.dense0 + i] = ch.dense0 + i;
    }
  }
}

// Bottom-s: the first min(limit, size) entries of each sketch's fmh-sorted index
// list name the kept elements (distinct indices: plain stores, no order).
__global__ __launch_bounds__(kDsB) void k_ds_mark(const DownsampleArgs a, const uint64_t* __restrict__ idx_sorted,
                                                  uint64_t limit, uint32_t* __restrict__ keep_flag) {
  const uint32_t g = a.g0 + blockIdx.y;
  const uint64_t size = a.sizes[g];
  const uint64_t take = size < limit ? size : limit;
  const uint64_t base = (uint64_t)blockIdx.x * kDownsampleChunk;
  const uint64_t d0 = a.dense_off[g];
#pragma unroll
  for (int j = 0; j < kDsItems; ++j) {
    const uint64_t r = base + (uint64_t)j * kDsB + threadIdx.x;
    if (r < take) keep_flag[idx_sorted[d0 + r]] = 1u;
  }
}

// fn(grid, args) for every slice of at most kDsMaxGridY sketches.
template <class F>
hipError_t for_sketch_slices(DownsampleArgs a, uint32_t n, uint64_t max_len, F fn) {
  if (n == 0 || max_len == 0) return hipSuccess;
  const uint64_t chunks = (max_len + kDownsampleChunk - 1) / kDownsampleChunk;
  for (uint32_t g0 = 0; g0 < n; g0 += kDsMaxGridY) {
    a.g0 = g0;
    fn(dim3((unsigned)chunks, std::min<uint32_t>(n - g0, kDsMaxGridY)), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// f.template operator()<EW, FLAVOUR, MODE>() for the runtime (ew, flavour, mode)
template <class F>
void dispatch(int ew, int flavour, int mode, F f) {
  auto by_mode = [&](auto e, auto fl) {
    constexpr int E = decltype(e)::value, FL = decltype(fl)::value;
    if (mode == kDownsampleFrac) f.template operator()<E, FL, kDownsampleFrac>();
    else if (mode == kDownsampleFlag) f.template operator()<E, 0, kDownsampleFlag>();
    else f.template operator()<E, 0, kDownsampleAll>();
  };
  auto by_flavour = [&](auto e) {
    if (flavour == 0) by_mode(e, std::integral_constant<int, 0>{});
    else by_mode(e, std::integral_constant<int, 1>{});
  };
  if (ew == 1) by_flavour(std::integral_constant<int, 1>{});
  else by_flavour(std::integral_constant<int, 2>{});
}

struct CountLaunch {
  dim3 grid;
  const DownsampleArgs& a;
  uint32_t* counts;
  hipStream_t s;
  template <int EW, int FLAVOUR, int MODE>
  void operator()() const {
    hipLaunchKernelGGL((k_ds_count<EW, FLAVOUR, MODE>), grid, dim3(kDsB), 0, s, a, counts);
  }
};

struct ScatterLaunch {
  dim3 grid;
  const DownsampleArgs& a;
  const uint64_t* offs;
  uint64_t* out;
  hipStream_t s;
  template <int EW, int FLAVOUR, int MODE>
  void operator()() const {
    hipLaunchKernelGGL((k_ds_scatter<EW, FLAVOUR, MODE>), grid, dim3(kDsB), 0, s, a, offs, out);
  }
};

struct FmhLaunch {
  dim3 grid;
  const DownsampleArgs& a;
  uint64_t* fmh;
  uint64_t* idx;
  hipStream_t s;
  template <int EW, int FLAVOUR, int MODE>
  void operator()() const {
    hipLaunchKernelGGL((k_ds_fmh<EW, FLAVOUR>), grid, dim3(kDsB), 0, s, a, fmh, idx);
  }
};

}  // namespace

hipError_t downsample_count(const DownsampleArgs& args, int ew, int flavour, int mode, uint32_t n, uint64_t max_len,
                            uint32_t* counts, hipStream_t s) {
  return for_sketch_slices(args, n, max_len, [&](dim3 grid, const DownsampleArgs& a) {
    dispatch(ew, flavour, mode, CountLaunch{grid, a, counts, s});
  });
}

hipError_t downsample_offsets(uint32_t* counts, uint64_t n_chunks, uint64_t* offs, const uint64_t* chunk_off,
                              uint32_t n, uint64_t* starts, uint32_t* sizes, Scratch& tmp, hipStream_t s) {
  hipError_t e;
  // one closing zero: offs[n_chunks] is the total, and an empty last sketch reads it
  if ((e = hipMemsetAsync(counts + n_chunks, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
  size_t need = 0;
  e = rocprim::exclusive_scan(nullptr, need, counts, offs, (uint64_t)0, (size_t)(n_chunks + 1),
                              rocprim::plus<uint64_t>(), s);
  if (e != hipSuccess) return e;
  if ((e = tmp.reserve(need)) != hipSuccess) return e;
  need = tmp.bytes;
  e = rocprim::exclusive_scan(tmp.ptr, need, counts, offs, (uint64_t)0, (size_t)(n_chunks + 1),
                              rocprim::plus<uint64_t>(), s);
  if (e != hipSuccess || n == 0) return e;
  hipLaunchKernelGGL(k_ds_meta, dim3((n + kDsB - 1) / kDsB), dim3(kDsB), 0, s, offs, chunk_off, n, starts, sizes);
  return hipGetLastError();
}

hipError_t downsample_scatter(const DownsampleArgs& args, int ew, int flavour, int mode, uint32_t n,
                              uint64_t max_len, const uint64_t* offs, uint64_t* out, hipStream_t s) {
  return for_sketch_slices(args, n, max_len, [&](dim3 grid, const DownsampleArgs& a) {
    dispatch(ew, flavour, mode, ScatterLaunch{grid, a, offs, out, s});
  });
}

hipError_t downsample_fmh(const DownsampleArgs& args, int ew, int flavour, uint32_t n, uint64_t max_len,
                          uint64_t* fmh, uint64_t* idx, hipStream_t s) {
  return for_sketch_slices(args, n, max_len, [&](dim3 grid, const DownsampleArgs& a) {
    dispatch(ew, flavour, kDownsampleFrac, FmhLaunch{grid, a, fmh, idx, s});
  });
}

hipError_t downsample_mark(const DownsampleArgs& args, uint32_t n, uint64_t limit, uint64_t max_len,
                           const uint64_t* idx_sorted, uint32_t* keep_flag, hipStream_t s) {
  return for_sketch_slices(args, n, std::min(limit, max_len), [&](dim3 grid, const DownsampleArgs& a) {
    hipLaunchKernelGGL(k_ds_mark, grid, dim3(kDsB), 0, s, a, idx_sorted, limit, keep_flag);
  });
}

}  // namespace sks
