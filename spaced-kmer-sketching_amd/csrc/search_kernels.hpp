// Query-vs-reference search: hits from count tiles (search.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct sks_hit;  // include/sks.h

namespace sks {

// Hits of one reference batch: `packed` holds the batch's count tiles
// [b_blocks][q_blocks][64][64] (tile bj * q_blocks + qi: query block qi against
// batch block bj, rows = queries).  Cell (q, r) with q < nq and r < n_batch is
// a hit iff count >= min_shared (>= 1) and containment_of(count, q_sizes[q]) >=
// min_containment; its record {q, ref0 + r, count, |Q_q|, containment, ANI}
// goes to hits[slot], slot taken from *counter (one atomicAdd per wavefront),
// and is stored only when slot < cap: *counter ends as the exact hit count.
// stat_q / stat_b: the two layouts' status words; a non-zero word 1 (invalid
// layout) makes the launch a no-op.  root: optional ANI table for query sets of
// root_size elements (sks_ctx_ani_table).
hipError_t launch_search_hits(const int32_t* packed, uint32_t q_blocks, uint32_t b_blocks, uint32_t nq,
                              uint32_t ref0, uint32_t n_batch, const uint32_t* q_sizes, double min_containment,
                              int32_t min_shared, int kmer_num_ones, const double* root, uint32_t root_size,
                              const uint32_t* stat_q, const uint32_t* stat_b, sks_hit* hits, uint64_t cap,
                              unsigned long long* counter, hipStream_t s);
// keys[i] = hits[i].query << ref_bits | hits[i].ref, idx[i] = i; and
// dst[i] = src[idx[i]] (the records in sorted-key order).
hipError_t launch_search_keys(const sks_hit* hits, uint64_t n, int ref_bits, uint64_t* keys, uint64_t* idx,
                              hipStream_t s);
hipError_t launch_search_gather(const sks_hit* src, const uint64_t* idx, uint64_t n, sks_hit* dst, hipStream_t s);

}  // namespace sks
