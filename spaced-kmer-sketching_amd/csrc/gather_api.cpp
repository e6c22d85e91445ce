// C-ABI implementation (include/sks.h): greedy min-set cover of one query sketch
// by reference sketches (kernels in gather.hip, arithmetic in gather_plan.hpp).
#include "gather_plan.hpp"
#include "sks_ctx.hpp"

using namespace sks;

namespace {

int gather_core(sks_ctx* c, const char* who, const uint64_t* d_q, uint32_t q_size, const SketchSpan& R, int ew,
                int kmer_num_ones, int32_t min_shared, uint32_t max_rounds, sks_gather_hit* d_hits,
                uint64_t hit_cap, uint64_t* n_hits, uint32_t* n_unexplained) {
  const std::string me(who);
  *n_hits = 0;
  if (n_unexplained) *n_unexplained = q_size;
  if (q_size == 0 || R.n == 0) return SKS_OK;
  if (q_size > 0x7fffffffu || R.n > 0x7fffffffu)
    return sks::fail(SKS_E_UNSUPPORTED, me + ": >= 2^31 query elements or references");
  DeviceGuard g(c->device);
  const int32_t thr = gather_threshold(min_shared);
  const uint32_t words = gather_bitmap_words(q_size);
  // c->lay: the state words, the two best keys, the candidates' arrival words,
  // off / shared / cand / last (r_n words each), the position lists (r_total
  // words) and the bitmap
  Carver cv;
  const Region<uint32_t> r_state = cv.take<uint32_t>(kGatherStateWords);
  const Region<unsigned long long> r_best = cv.take<unsigned long long>(2);
  const Region<unsigned long long> r_arrive = cv.take<unsigned long long>(R.n);
  const Region<uint32_t> r_off = cv.take<uint32_t>(R.n);
  const Region<int32_t> r_shared = cv.take<int32_t>(R.n);
  const Region<uint32_t> r_cand = cv.take<uint32_t>(R.n);
  const Region<int32_t> r_last = cv.take<int32_t>(R.n);
  const Region<uint32_t> r_list = cv.take<uint32_t>((size_t)std::max<uint64_t>(R.total, 1));
  const Region<uint32_t> r_bitmap = cv.take<uint32_t>(words);
  SKS_HIP(c->lay.reserve(cv.need()));
  void* w = c->lay.ptr;
  uint32_t* state = r_state.in(w);

  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  SKS_HIP(hipMemsetAsync(state, 0, kGatherStateWords * sizeof(uint32_t), c->stream));
  SKS_HIP(hipMemsetAsync(r_arrive.in(w), 0, (size_t)R.n * sizeof(unsigned long long), c->stream));
  SKS_HIP(sks::launch_gather_offsets(R.sizes, R.n, R.total, r_off.in(w), state, c->stream));
  SKS_HIP(sks::launch_gather_member(d_q, q_size, R.data, R.starts, R.sizes, R.n, ew, r_off.in(w), r_list.in(w),
                                    r_shared.in(w), state, c->stream));
  SKS_HIP(sks::launch_gather_begin(r_shared.in(w), R.n, thr, q_size, r_cand.in(w), r_last.in(w), r_bitmap.in(w),
                                   r_best.in(w), state, c->stream));
  // the number of candidates sizes the scoring grid (the one wait of the membership phase)
  uint32_t h_state[kGatherStateWords];
  SKS_HIP(sks::pinned_d2h(h_state, state, sizeof h_state, c->stream));
  if (h_state[kGatherBadTotal]) {
    SKS_HIP(hipEventRecord(c->ev_end, c->stream));
    return sks::fail(SKS_E_ARG, me + ": the references' sizes add up to more than r_total");
  }
  GatherRound round{};
  round.cand = r_cand.in(w);
  round.n_cand = h_state[kGatherCands];
  round.per = gather_blocks_per_candidate(h_state[kGatherLongest], round.n_cand);
  round.arrive = r_arrive.in(w);
  round.off = r_off.in(w);
  round.list = r_list.in(w);
  round.shared = r_shared.in(w);
  round.r_sizes = R.sizes;
  round.last = r_last.in(w);
  round.bitmap = r_bitmap.in(w);
  round.best = r_best.in(w);
  round.state = state;
  round.q_size = q_size;
  round.thr = thr;
  round.max_rounds = max_rounds;
  round.inv_k = ((double)1.0) / ((double)kmer_num_ones);
  round.hits = d_hits;
  round.cap = d_hits ? hit_cap : 0;
  // groups of rounds, one wait a group (gather_plan.hpp); kernels queued behind
  // the round that raised done return at once
  const uint64_t limit = round.n_cand ? gather_round_limit(round.n_cand, max_rounds) : 0;
  uint64_t queued = 0;
  bool done = round.n_cand == 0;
  while (!done && queued < limit) {
    const uint32_t group = gather_group_rounds(c->gather_rounds, queued, limit);
    for (uint32_t i = 0; i < group; ++i) SKS_HIP(sks::launch_gather_round(round, (uint32_t)(queued + i), c->stream));
    queued += group;
    SKS_HIP(sks::pinned_d2h(h_state, state, sizeof h_state, c->stream));
    done = h_state[kGatherDone] != 0;
  }
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  if (!done) return sks::fail(SKS_E_HIP, me + ": the rounds did not finish within their bound");
  *n_hits = h_state[kGatherHits];
  if (n_unexplained) *n_unexplained = h_state[kGatherRemaining];
  if (d_hits && *n_hits > hit_cap)
    return sks::fail(SKS_E_LENGTH, me + ": " + std::to_string(*n_hits) + " hits, capacity " + std::to_string(hit_cap));
  return SKS_OK;
}

}  // namespace

extern "C" {

int sks_gather(sks_ctx* c, const uint64_t* d_q, uint32_t q_size, const uint64_t* d_r_data,
               const uint64_t* d_r_starts, const uint32_t* d_r_sizes, uint32_t r_n, uint32_t r_max_size,
               uint64_t r_total, int elem_words, int kmer_num_ones, int32_t min_shared, uint32_t max_rounds,
               sks_gather_hit* d_hits, uint64_t hit_cap, uint64_t* n_hits, uint32_t* n_unexplained) {
  if (n_hits) *n_hits = 0;
  if (!c) return sks::fail(SKS_E_ARG, "sks_gather: null ctx");
  if (!n_hits) return sks::fail(SKS_E_ARG, "sks_gather: null n_hits");
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_gather: kmer_num_ones must be positive");
  if ((q_size && !d_q) || (r_n && (!d_r_starts || !d_r_sizes)) || (r_n && r_total && !d_r_data))
    return sks::fail(SKS_E_ARG, "sks_gather: null argument");
  SKS_TRY(check_span_totals("sks_gather", "in the references", r_total));
  // r_max_size is taken for symmetry with sks_search: a workgroup walks a reference whatever its size
  const SketchSpan R{d_r_data, d_r_starts, d_r_sizes, r_n, r_max_size, r_total, nullptr};
  return gather_core(c, "sks_gather", d_q, q_size, R, elem_words, kmer_num_ones, min_shared, max_rounds, d_hits,
                     hit_cap, n_hits, n_unexplained);
}

int sks_gather_sets(sks_ctx* c, const sks_sketch_set* queries, uint32_t q, const sks_sketch_set* refs,
                    int32_t min_shared, uint32_t max_rounds, sks_gather_hit* d_hits, uint64_t hit_cap,
                    uint64_t* n_hits, uint32_t* n_unexplained) {
  if (n_hits) *n_hits = 0;
  if (!c) return sks::fail(SKS_E_ARG, "sks_gather_sets: null ctx");
  if (!queries || !refs || !n_hits) return sks::fail(SKS_E_ARG, "sks_gather_sets: null argument");
  if (q >= queries->n)
    return sks::fail(SKS_E_ARG, "sks_gather_sets: query index " + std::to_string(q) + " out of range (" +
                                    std::to_string(queries->n) + " sketches)");
  sks_sketch_info qi{};
  int k = 0;
  // subtraction only means something when every sketch samples the same hash space
  SKS_TRY(search_sets_compatible(c, "sks_gather_sets", queries, refs, &qi, &k,
                                 "the sets' policy kind must be SKS_FRAC_MOD (a bottom-s sketch samples a hash range "
                                 "of its own)"));
  const SketchSpan R = span_of(refs);
  SKS_TRY(check_span_totals("sks_gather_sets", "in the references", R.total));
  const uint64_t* d_q = queries->d_data() + queries->starts[q] * (uint64_t)qi.elem_words;
  return gather_core(c, "sks_gather_sets", d_q, queries->sizes[q], R, qi.elem_words, k, min_shared, max_rounds,
                     d_hits, hit_cap, n_hits, n_unexplained);
}

}  // extern "C"
