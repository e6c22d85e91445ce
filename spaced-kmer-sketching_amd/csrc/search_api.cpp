// C-ABI implementation (include/sks.h): query-vs-reference search with
// thresholded hit lists (kernels in search.hip, layouts and join as the
// all-pairs calls; the walk over reference batches in search_walk.hpp).
#include "search_walk.hpp"

using namespace sks;

namespace {

// h_bounds, invalid_layout: as the core of with_mask_bounds_retry (null: sampled once from the references).
int search_core(sks_ctx* c, const char* who, const SketchSpan& Q, const SketchSpan& R, int ew, int kmer_num_ones,
                double min_containment, int32_t min_shared, const std::vector<uint64_t>* h_bounds, sks_hit* d_hits,
                uint64_t hit_cap, uint64_t* n_hits, bool* invalid_layout = nullptr) {
  const std::string me(who);
  *n_hits = 0;
  if (Q.n == 0 || R.n == 0) return SKS_OK;
  DeviceGuard g(c->device);
  // the walk's words: the 64-bit hit counter, cleared and read back with the
  // status words
  SearchWalk w;
  SKS_TRY(w.plan(c, me, Q, R, ew, 2, 0));
  // no more hits than pairs: a generous hit_cap does not size the buffers
  const uint64_t cap = d_hits ? std::min<uint64_t>(hit_cap, (uint64_t)Q.n * R.n) : 0;
  // c->hits: unsorted records | keys in, out | indices in, out
  Carver hv;
  const Region<sks_hit> r_raw = hv.take<sks_hit>(cap);
  const Region<uint64_t> r_kin = hv.take<uint64_t>(cap), r_kout = hv.take<uint64_t>(cap);
  const Region<uint64_t> r_iin = hv.take<uint64_t>(cap), r_iout = hv.take<uint64_t>(cap);
  hv.take<char>(256);
  SKS_HIP(c->hits.reserve(hv.need()));
  unsigned long long* counter = reinterpret_cast<unsigned long long*>(w.head);
  sks_hit* raw = r_raw.in(c->hits.ptr);

  SKS_TRY(w.begin(c, Q, R, h_bounds));
  SKS_TRY(sks_ctx_ani_table(c, Q.max_size, kmer_num_ones));
  sks::JoinAni root{};  // only the context's table, if it is for this k
  attach_ani_root(c, kmer_num_ones, root);
  for (uint32_t b = 0; b < w.n_batches; ++b) {
    SKS_TRY(w.batch(c, R, b));
    SKS_HIP(sks::launch_search_hits(w.cnt, w.qb, w.nbb, Q.n, w.r0, w.rn, Q.sizes, min_containment, min_shared,
                                    kmer_num_ones, root.root, root.root_size, w.stat, w.bstat,
                                    d_hits ? raw : nullptr, cap, counter, c->stream));
  }
  // the count and every layout's status (one wait)
  SKS_TRY(w.end(c, me, "no hits are reported", invalid_layout));
  const uint64_t found = (uint64_t)w.h_span[0] | ((uint64_t)w.h_span[1] << 32);
  *n_hits = found;
  if (d_hits && found > hit_cap) {
    SKS_HIP(hipEventRecord(c->ev_end, c->stream));
    return sks::fail(SKS_E_LENGTH, me + ": " + std::to_string(found) + " hits, capacity " + std::to_string(hit_cap));
  }
  if (d_hits && found) {
    // (query, ref) order: sort query << ref_bits | ref with the record index, gather
    void* hw = c->hits.ptr;
    const int ref_bits = end_bit_of(R.n - 1), q_bits = end_bit_of(Q.n - 1);
    SKS_HIP(sks::launch_search_keys(raw, found, ref_bits, r_kin.in(hw), r_iin.in(hw), c->stream));
    const std::vector<uint64_t> off{0, found};
    SKS_HIP(sks::seg_sort_pairs(r_kin.in(hw), r_kout.in(hw), r_iin.in(hw), r_iout.in(hw), found, off, nullptr,
                                ref_bits + q_bits, c->tmp, c->stream));
    SKS_HIP(sks::launch_search_gather(raw, r_iout.in(hw), found, d_hits, c->stream));
  }
  SKS_HIP(hipEventRecord(c->ev_end, c->stream));
  return SKS_OK;
}

}  // namespace

extern "C" {

int sks_search(sks_ctx* c, const uint64_t* d_q_data, const uint64_t* d_q_starts, const uint32_t* d_q_sizes,
               uint32_t q_n, uint32_t q_max_size, uint64_t q_total, const uint64_t* d_r_data,
               const uint64_t* d_r_starts, const uint32_t* d_r_sizes, uint32_t r_n, uint32_t r_max_size,
               uint64_t r_total, int elem_words, int kmer_num_ones, double min_containment, int32_t min_shared,
               sks_hit* d_hits, uint64_t hit_cap, uint64_t* n_hits) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_search: null ctx");
  if (!n_hits) return sks::fail(SKS_E_ARG, "sks_search: null n_hits");
  *n_hits = 0;
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_search: kmer_num_ones must be positive");
  if (!(min_containment == min_containment)) return sks::fail(SKS_E_ARG, "sks_search: min_containment is NaN");
  if ((q_n && (!d_q_starts || !d_q_sizes)) || (r_n && (!d_r_starts || !d_r_sizes)))
    return sks::fail(SKS_E_ARG, "sks_search: null argument");
  SKS_TRY(check_span_totals("sks_search", "in one set", q_total, r_total));
  const SketchSpan Q{d_q_data, d_q_starts, d_q_sizes, q_n, q_max_size, q_total, nullptr};
  const SketchSpan R{d_r_data, d_r_starts, d_r_sizes, r_n, r_max_size, r_total, nullptr};
  return search_core(c, "sks_search", Q, R, elem_words, kmer_num_ones, min_containment, min_shared, nullptr, d_hits,
                     hit_cap, n_hits);
}

int sks_search_sets(sks_ctx* c, const sks_sketch_set* queries, const sks_sketch_set* refs, double min_containment,
                    int32_t min_shared, sks_hit* d_hits, uint64_t hit_cap, uint64_t* n_hits) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_search_sets: null ctx");
  if (!queries || !refs || !n_hits) return sks::fail(SKS_E_ARG, "sks_search_sets: null argument");
  *n_hits = 0;
  if (!(min_containment == min_containment)) return sks::fail(SKS_E_ARG, "sks_search_sets: min_containment is NaN");
  sks_sketch_info qi{};
  int k = 0;
  SKS_TRY(search_sets_compatible(c, "sks_search_sets", queries, refs, &qi, &k));
  const SketchSpan Q = span_of(queries), R = span_of(refs);
  SKS_TRY(check_span_totals("sks_search_sets", "in one set", Q.total, R.total));
  // the mask's group bounds for every batch; sampled from the references if they cannot place a layout
  std::vector<uint64_t> mask_bounds;
  SKS_TRY(mask_group_bounds(qi.mask, qi.elem_words, std::max(Q.max_size, R.max_size), &mask_bounds));
  return with_mask_bounds_retry(mask_bounds, [&](const std::vector<uint64_t>* h_bounds, bool* invalid) {
    return search_core(c, "sks_search_sets", Q, R, qi.elem_words, k, min_containment, min_shared, h_bounds, d_hits,
                       hit_cap, n_hits, invalid);
  });
}

}  // extern "C"
