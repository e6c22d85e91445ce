// Greedy min-set cover of one query sketch by reference sketches (gather.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct sks_gather_hit;  // include/sks.h

namespace sks {

// The device state of one sks_gather call (u32 words).
enum GatherState : uint32_t {
  kGatherDone = 0,       // raised by the round that finds nothing left to report
  kGatherHits = 1,       // rounds reported so far (counted past the capacity too)
  kGatherRemaining = 2,  // |Q_rem|
  kGatherCands = 3,      // candidates: references with shared >= thr
  kGatherListTotal = 4,  // the candidates' position lists together
  kGatherBadTotal = 5,   // the sizes' sum exceeds r_total: nothing was searched
  kGatherLongest = 6,    // the longest candidate list
  kGatherStateWords = 8
};

// off[r] = the sizes before r (r < r_n).  A sum above r_total raises
// state[kGatherBadTotal], and the membership launch then does nothing.
hipError_t launch_gather_offsets(const uint32_t* r_sizes, uint32_t r_n, uint64_t r_total, uint32_t* off,
                                 uint32_t* state, hipStream_t s);
// Membership: for reference r, list[off[r] ..) receives the ascending positions
// in the query (q, q_size elements of elem_words words, ascending) of the
// elements of r that the query holds, and shared[r] their number.  A workgroup
// per reference.
hipError_t launch_gather_member(const uint64_t* q, uint32_t q_size, const uint64_t* r_data,
                                const uint64_t* r_starts, const uint32_t* r_sizes, uint32_t r_n, int elem_words,
                                const uint32_t* off, uint32_t* list, int32_t* shared, const uint32_t* state,
                                hipStream_t s);
// The candidates (shared[r] >= thr) in index order: cand[c] = r, last[c] =
// shared[r]; state[kGatherCands], state[kGatherListTotal]; and the round state:
// the bitmap of q_size set bits, both best keys 0, no hits, every element
// remaining.
hipError_t launch_gather_begin(const int32_t* shared, uint32_t r_n, int32_t thr, uint32_t q_size, uint32_t* cand,
                               int32_t* last, uint32_t* bitmap, unsigned long long* best, uint32_t* state,
                               hipStream_t s);
// One round: score every live candidate against the bitmap into best[round & 1],
// then take the winner (or raise done).  Both return at once when done is up.
struct GatherRound {
  const uint32_t* cand;
  uint32_t n_cand;
  uint32_t per;  // workgroups per candidate of the scoring launch (gather_blocks_per_candidate)
  const uint32_t* off;
  const uint32_t* list;
  const int32_t* shared;
  const uint32_t* r_sizes;
  int32_t* last;
  uint32_t* bitmap;
  unsigned long long* arrive;  // [n_cand], zero: where a candidate's scoring workgroups meet
  unsigned long long* best;
  uint32_t* state;
  uint32_t q_size;
  int32_t thr;
  uint32_t max_rounds;
  double inv_k;
  sks_gather_hit* hits;  // or null
  uint64_t cap;
};
hipError_t launch_gather_round(const GatherRound& g, uint32_t round, hipStream_t s);

}  // namespace sks
