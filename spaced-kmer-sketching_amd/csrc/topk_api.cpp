// C-ABI implementation (include/sks.h): the k best references per query
// (kernels in topk.hip, arithmetic in topk_plan.hpp, the walk over reference
// batches shared with the search in search_walk.hpp).
#include "search_walk.hpp"

using namespace sks;

namespace {

struct TopkRule {
  int rank_kind;
  uint32_t k;
  double min_score;
  int32_t min_shared;
  bool skip_same_index;
};

// The checks the two forms share, in the contract's order (ctx first, before
// any device is touched).
int topk_check(const char* who, const sks_ctx* c, uint32_t q_n, const sks_top_hit* d_hits, const TopkRule& t) {
  const std::string me(who);
  if (!c) return sks::fail(SKS_E_ARG, me + ": null ctx");
  if (q_n && !d_hits) return sks::fail(SKS_E_ARG, me + ": null d_hits");
  if (t.k == 0) return sks::fail(SKS_E_ARG, me + ": k must be at least 1");
  if (!(t.min_score == t.min_score)) return sks::fail(SKS_E_ARG, me + ": min_score is NaN");
  if (t.rank_kind != SKS_RANK_QUERY && t.rank_kind != SKS_RANK_REF && t.rank_kind != SKS_RANK_MAX)
    return sks::fail(SKS_E_ARG, me + ": unknown rank_kind " + std::to_string(t.rank_kind));
  return SKS_OK;
}

int topk_check_k(const char* who, const TopkRule& t) {
  if (t.k > SKS_TOPK_MAX)
    return sks::fail(SKS_E_UNSUPPORTED, std::string(who) + ": k = " + std::to_string(t.k) + " is above SKS_TOPK_MAX (" +
                                            std::to_string(SKS_TOPK_MAX) + ")");
  return SKS_OK;
}

// h_bounds, invalid_layout: as search_core.
int topk_core(sks_ctx* c, const char* who, const SketchSpan& Q, const SketchSpan& R, int ew, int kmer_num_ones,
              const TopkRule& t, const std::vector<uint64_t>* h_bounds, sks_top_hit* d_hits, uint32_t* d_counts,
              bool* invalid_layout = nullptr) {
  const std::string me(who);
  if (Q.n == 0) return SKS_OK;
  DeviceGuard g(c->device);
  const size_t state_bytes = (size_t)Q.n * t.k * sizeof(TopkSlot);
  TopkArgs a{nullptr, Q.n, t.k, t.rank_kind, t.min_score, t.min_shared, t.skip_same_index, Q.sizes, R.sizes};
  if (R.n == 0) {
    // nothing to join: every list empty
    SKS_HIP(c->lay.reserve(state_bytes));
    a.state = static_cast<TopkSlot*>(c->lay.ptr);
    SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
    SKS_HIP(sks::launch_topk_init(a.state, Q.n, t.k, c->stream));
    SKS_HIP(sks::launch_topk_finish(a, kmer_num_ones, d_hits, d_counts, c->stream));
    SKS_HIP(hipEventRecord(c->ev_end, c->stream));
    return SKS_OK;
  }
  // the lists between batches: the walk's extra region
  SearchWalk w;
  SKS_TRY(w.plan(c, me, Q, R, ew, 0, state_bytes));
  a.state = static_cast<TopkSlot*>(w.extra);
  SKS_TRY(w.begin(c, Q, R, h_bounds));
  SKS_HIP(sks::launch_topk_init(a.state, Q.n, t.k, c->stream));
  for (uint32_t b = 0; b < w.n_batches; ++b) {
    SKS_TRY(w.batch(c, R, b));
    SKS_HIP(sks::launch_topk_update(a, w.cnt, w.qb, w.nbb, w.r0, w.rn, w.stat, w.bstat, c->stream));
  }
  SKS_HIP(sks::launch_topk_finish(a, kmer_num_ones, d_hits, d_counts, c->stream));
  // every layout's status (the one wait)
  SKS_TRY(w.end(c, me, "the lists are unspecified", invalid_layout));
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

}  // namespace

extern "C" {

int sks_search_topk(sks_ctx* c, const uint64_t* d_q_data, const uint64_t* d_q_starts, const uint32_t* d_q_sizes,
                    uint32_t q_n, uint32_t q_max_size, uint64_t q_total, const uint64_t* d_r_data,
                    const uint64_t* d_r_starts, const uint32_t* d_r_sizes, uint32_t r_n, uint32_t r_max_size,
                    uint64_t r_total, int elem_words, int kmer_num_ones, int rank_kind, uint32_t k, double min_score,
                    int32_t min_shared, int skip_same_index, sks_top_hit* d_hits, uint32_t* d_counts) {
  const TopkRule t{rank_kind, k, min_score, min_shared, skip_same_index != 0};
  SKS_TRY(topk_check("sks_search_topk", c, q_n, d_hits, t));
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_search_topk: kmer_num_ones must be positive");
  if ((q_n && (!d_q_starts || !d_q_sizes)) || (r_n && (!d_r_starts || !d_r_sizes)))
    return sks::fail(SKS_E_ARG, "sks_search_topk: null argument");
  SKS_TRY(topk_check_k("sks_search_topk", t));
  SKS_TRY(check_span_totals("sks_search_topk", "in one set", q_total, r_total));
  const SketchSpan Q{d_q_data, d_q_starts, d_q_sizes, q_n, q_max_size, q_total, nullptr};
  const SketchSpan R{d_r_data, d_r_starts, d_r_sizes, r_n, r_max_size, r_total, nullptr};
  return topk_core(c, "sks_search_topk", Q, R, elem_words, kmer_num_ones, t, nullptr, d_hits, d_counts);
}

int sks_search_topk_sets(sks_ctx* c, const sks_sketch_set* queries, const sks_sketch_set* refs, int rank_kind,
                         uint32_t k, double min_score, int32_t min_shared, int skip_same_index, sks_top_hit* d_hits,
                         uint32_t* d_counts) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_search_topk_sets: null ctx");
  if (!queries || !refs) return sks::fail(SKS_E_ARG, "sks_search_topk_sets: null argument");
  const TopkRule t{rank_kind, k, min_score, min_shared, skip_same_index != 0};
  SKS_TRY(topk_check("sks_search_topk_sets", c, queries->n, d_hits, t));
  SKS_TRY(topk_check_k("sks_search_topk_sets", t));
  sks_sketch_info qi{};
  int ones = 0;
  SKS_TRY(search_sets_compatible(c, "sks_search_topk_sets", queries, refs, &qi, &ones));
  const SketchSpan Q = span_of(queries), R = span_of(refs);
  SKS_TRY(check_span_totals("sks_search_topk_sets", "in one set", Q.total, R.total));
  if (Q.n == 0 || R.n == 0)  // no layout to place
    return topk_core(c, "sks_search_topk_sets", Q, R, qi.elem_words, ones, t, nullptr, d_hits, d_counts);
  // the mask's group bounds for every batch; sampled from the references if they cannot place a layout
  std::vector<uint64_t> mask_bounds;
  SKS_TRY(mask_group_bounds(qi.mask, qi.elem_words, std::max(Q.max_size, R.max_size), &mask_bounds));
  return with_mask_bounds_retry(mask_bounds, [&](const std::vector<uint64_t>* h_bounds, bool* invalid) {
    return topk_core(c, "sks_search_topk_sets", Q, R, qi.elem_words, ones, t, h_bounds, d_hits, d_counts, invalid);
  });
}

}  // extern "C"
