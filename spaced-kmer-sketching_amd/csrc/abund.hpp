// K-mer abundances (abund.hip): run lengths of a counted build, the trim of a
// counted set, the weighted overlap of sketch pairs and a set's totals.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "abund_plan.hpp"

namespace sks {

// From seg_unique_scan's flags and positions over n_seg sorted segments
// [off[g], off[g + 1]) (the longest of max_len records): run_start[rank] = the
// index of each run's first record (T + 1 words of scratch), then abund[rank] =
// the clamped run length, dense in distinct rank as seg_unique_scatter places the
// elements without a dst_off.  starts / sizes (may both be null): [n_seg] first
// rank and distinct count of each segment.
hipError_t abund_run_lengths(const uint32_t* d_flag, const uint64_t* d_pos, const uint64_t* d_off, uint32_t n_seg,
                             uint64_t max_len, uint64_t* run_start, uint32_t* abund, uint64_t* starts,
                             uint32_t* sizes, hipStream_t s);

// An order-preserving trim by abundance over CSR arrays, in the count -> scan ->
// scatter shape of downsample.hip and filter.hip: workgroups own chunks of
// kDownsampleChunk consecutive elements of one sketch; chunk_off[g] = chunks
// before sketch g, counted from sizes on the host that bound the device's
// (chunk_off[n] = n_chunks; a chunk past a sketch's device size keeps nothing).
struct AbundTrimArgs {
  const uint64_t* data;       // elements (elem_words u64 each)
  const uint32_t* abund;      // one per element
  const uint64_t* starts;     // [n] device
  const uint32_t* sizes;      // [n] device
  const uint64_t* chunk_off;  // [n + 1] device
  uint32_t n;
  uint32_t min_abund, max_abund;
};
// bitmap: filter_bitmap_words(n_chunks) words, the ballots of the keep rule in
// element order; counts[chunk] = kept elements
hipError_t abund_trim_mark(const AbundTrimArgs& args, uint64_t n_chunks, uint64_t* bitmap, uint32_t* counts,
                           hipStream_t s);
// out[offs[chunk] + rank], out_abund[offs[chunk] + rank] = the chunk's kept elements and abundances, in order
hipError_t abund_trim_scatter(const AbundTrimArgs& args, int ew, uint64_t n_chunks, const uint64_t* bitmap,
                              const uint64_t* offs, uint64_t* out, uint32_t* out_abund, hipStream_t s);

// sks_abund_pairs: sketch d_a[p] of the samples (with abundances) against sketch
// d_b[p] of the references; an index outside its set gives shared -1, weight 0.
struct AbundPairsArgs {
  const uint64_t *s_data, *s_starts;
  const uint32_t *s_sizes, *s_abund;
  uint32_t s_n;
  const uint64_t *r_data, *r_starts;
  const uint32_t* r_sizes;
  uint32_t r_n;
  const int32_t *d_a, *d_b;
  uint64_t n_pairs;
  int32_t* shared;
  unsigned long long* weight;
};
hipError_t abund_pairs(const AbundPairsArgs& args, int ew, hipStream_t s);

// totals[i] = the sum of sketch i's abundances
hipError_t abund_totals(const uint32_t* abund, const uint64_t* starts, const uint32_t* sizes, uint32_t n,
                        unsigned long long* totals, hipStream_t s);

}  // namespace sks
