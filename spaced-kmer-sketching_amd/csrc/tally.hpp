// Grouped tallies of sorted sketches (tally.hip): the threshold filter over the
// runs merge.hip's rounds leave, duplicates kept.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tally_plan.hpp"

namespace sks {

// Groups as merge_unique_count takes them (runs[2g ..] = address and length of
// group g's one sorted run, chunk_off[g] the kDownsampleChunk-element chunks
// before it) and limits[2g ..] = lo | hi << 32 (tally_lo, tally_hi) and the
// group's listed members.  An element stays iff it is the first of its value in
// the group and the value occurs lo .. hi times there (tally_keeps); every read
// lies inside the group's own run.  counts[chunk] = kept elements (then
// downsample_offsets); out[offs[chunk] + rank] = the kept elements, in order,
// and, with `mult`, mult[offs[chunk] + rank] = how often each occurs.
hipError_t tally_count(const uint64_t* runs, const uint64_t* chunk_off, const uint64_t* limits, uint32_t n_groups,
                       uint64_t n_chunks, int ew, uint32_t* counts, hipStream_t s);
hipError_t tally_scatter(const uint64_t* runs, const uint64_t* chunk_off, const uint64_t* limits, uint32_t n_groups,
                         uint64_t n_chunks, int ew, const uint64_t* offs, uint64_t* out, uint32_t* mult,
                         hipStream_t s);

}  // namespace sks
