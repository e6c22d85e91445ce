// Subtracting or intersecting sketches (filter.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "filter_plan.hpp"

namespace sks {

// An order-preserving membership filter over a source set's CSR arrays against
// the sketches of a filter set: workgroups own chunks of kFilterChunk
// consecutive elements of one source sketch on a dense grid of n_chunks.
struct FilterArgs {
  const uint64_t* data;       // the source set's elements and starts
  const uint64_t* starts;
  const uint64_t* chunk_off;  // [n + 1] chunks before each source sketch
  const uint64_t* dense_off;  // [n + 1] elements before each source sketch
  const uint64_t* fdata;      // the filter set's elements
  const uint64_t* frange;     // [2 n] per source sketch: its filter sketch's start (element index into fdata)
                              // and size, the size kFilterNone for a sketch that is copied
  uint32_t n;                 // source sketches (>= 1)
  int kind;                   // sks_filter_kind
  int no_stage;               // SKS_FILTER_NO_STAGE: every chunk searches its bracket where it lies
};
// pass 1: bitmap[chunk * kFilterChunkWords ..] = the kept elements of every chunk in element order
// (zero bits past the end of a sketch), counts[chunk] = their number
hipError_t filter_mark(const FilterArgs& args, int ew, uint64_t n_chunks, uint64_t* bitmap, uint32_t* counts,
                       hipStream_t s);
// pass 2: out[offs[chunk] + rank] = the chunk's kept elements, in order
hipError_t filter_scatter(const FilterArgs& args, int ew, uint64_t n_chunks, const uint64_t* bitmap,
                          const uint64_t* offs, uint64_t* out, hipStream_t s);

}  // namespace sks
