// Grouped unions of sorted sketches (merge.hip): pairwise merge rounds over
// run tables and an order-preserving duplicate filter.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "merge_plan.hpp"

namespace sks {

// One round: pair p is the four words pairs[4p ..] = address of the left run's
// first element, of the right run's, of the output's, and left length | right
// length << 32 (a carried run has right length 0).  Workgroup t of the dense
// grid owns tile t - tile_off[p] of its pair p (kMergeTile outputs).  Stable:
// the left run first on equal keys; duplicates are kept.
hipError_t merge_round(const uint64_t* pairs, const uint64_t* tile_off, uint32_t n_pairs, uint64_t n_tiles, int ew,
                       hipStream_t s);

// The duplicate filter over fully merged groups: group g is the two words
// runs[2g ..] = address of its first element and its length, chunk_off[g] the
// kDownsampleChunk-element chunks before it.  An element stays iff it differs
// from its predecessor in the group.  counts[chunk] = kept elements (then
// downsample_offsets); out[offs[chunk] + rank] = the kept elements, in order.
hipError_t merge_unique_count(const uint64_t* runs, const uint64_t* chunk_off, uint32_t n_groups, uint64_t n_chunks,
                              int ew, uint32_t* counts, hipStream_t s);
hipError_t merge_unique_scatter(const uint64_t* runs, const uint64_t* chunk_off, uint32_t n_groups,
                                uint64_t n_chunks, int ew, const uint64_t* offs, uint64_t* out, hipStream_t s);

}  // namespace sks
