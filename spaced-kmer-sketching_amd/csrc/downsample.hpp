// Sketch-set downsampling (downsample.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_mem.hpp"

namespace sks {

// An order-preserving filter over a set's CSR arrays: workgroups own chunks of
// kDownsampleChunk consecutive elements of one sketch on a (chunk, sketch) grid;
// chunk_off[g] = chunks before sketch g (chunk_off[n] = all chunks).
constexpr uint32_t kDownsampleChunk = 1024;
constexpr int kDownsampleFrac = 0;  // keep x iff frac_min_hash(x) % c == 0 (the DivTest words below)
constexpr int kDownsampleFlag = 1;  // keep the set's d-th element iff keep_flag[d] != 0
constexpr int kDownsampleAll = 2;   // a copy
struct DownsampleArgs {
  const uint64_t* data;        // the source set's arrays
  const uint64_t* starts;
  const uint32_t* sizes;
  const uint64_t* chunk_off;   // [n + 1]
  const uint64_t* dense_off;   // [n + 1] elements before each sketch (flag mode and the bottom-s helpers)
  const uint32_t* keep_flag;   // flag mode
  uint64_t kconst;             // fmh_const of the set
  uint32_t low_mask, high_mask;
  uint64_t dinv, dlim;
  uint32_t g0;                 // set by the launchers: first sketch of a grid slice
};
// counts[chunk] = kept elements of every chunk (n sketches, the longest of max_len elements)
hipError_t downsample_count(const DownsampleArgs& args, int ew, int flavour, int mode, uint32_t n, uint64_t max_len,
                            uint32_t* counts, hipStream_t s);
// offs[0 .. n_chunks] = exclusive scan of counts (counts needs n_chunks + 1 words), and from it
// starts[g], sizes[g] of the filtered set
hipError_t downsample_offsets(uint32_t* counts, uint64_t n_chunks, uint64_t* offs, const uint64_t* chunk_off,
                              uint32_t n, uint64_t* starts, uint32_t* sizes, Scratch& tmp, hipStream_t s);
// out[offs[chunk] + rank] = the chunk's kept elements, in order
hipError_t downsample_scatter(const DownsampleArgs& args, int ew, int flavour, int mode, uint32_t n,
                              uint64_t max_len, const uint64_t* offs, uint64_t* out, hipStream_t s);
// bottom-s: fmh[d] = frac_min_hash of the d-th element, idx[d] = d; and, from idx sorted by fmh
// within each sketch (stable), keep_flag[d] = 1 for each sketch's first min(limit, size) (keep_flag zeroed)
hipError_t downsample_fmh(const DownsampleArgs& args, int ew, int flavour, uint32_t n, uint64_t max_len,
                          uint64_t* fmh, uint64_t* idx, hipStream_t s);
hipError_t downsample_mark(const DownsampleArgs& args, uint32_t n, uint64_t limit, uint64_t max_len,
                           const uint64_t* idx_sorted, uint32_t* keep_flag, hipStream_t s);

}  // namespace sks
