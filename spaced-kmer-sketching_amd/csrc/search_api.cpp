// C-ABI implementation (include/sks.h): query-vs-reference search with
// thresholded hit lists (kernels in search.hip, layouts and join as the
// all-pairs calls).
#include "sks_ctx.hpp"

using namespace sks;

namespace {

// packed count tiles of one reference batch (16 KB a tile): the default batch is
// the largest number of reference blocks whose tiles fit
constexpr uint64_t kSearchTileBudget = 256ull << 20;

struct SearchSide {
  const uint64_t* data;
  const uint64_t* starts;
  const uint32_t* sizes;
  uint32_t n, max_size;
  uint64_t total;
  const uint32_t* h_sizes;  // host copy of the sizes, or null (batches are then sized by max_size)
};

// h_bounds: the host group bounds to use ((G + 1) * ew words for the log_b below),
// or null to sample them once from the references.
int search_core(sks_ctx* c, const char* who, const SearchSide& Q, const SearchSide& R, int ew, int kmer_num_ones,
                double min_containment, int32_t min_shared, const std::vector<uint64_t>* h_bounds, sks_hit* d_hits,
                uint64_t hit_cap, uint64_t* n_hits, bool* invalid_layout = nullptr) {
  const std::string me(who);
  *n_hits = 0;
  if (invalid_layout) *invalid_layout = false;
  if (Q.n == 0 || R.n == 0) return SKS_OK;
  DeviceGuard g(c->device);
  const uint32_t log_b = sks::join_log_b(std::max<uint32_t>(std::max(Q.max_size, R.max_size), 1));
  const uint32_t G = sks::join_layout_groups(log_b);
  const uint32_t qb = (Q.n + 63) / 64, rb = (R.n + 63) / 64;
  // reference blocks per batch: the caller's, else what the tile budget holds
  uint64_t bb = c->search_batch ? c->search_batch : std::max<uint64_t>(1, kSearchTileBudget / ((uint64_t)qb * 16384));
  bb = std::min<uint64_t>(bb, rb);
  if ((uint64_t)qb * bb > 0x7fffffffull || (uint64_t)qb + rb > (1u << 25))
    return sks::fail(SKS_E_UNSUPPORTED, me + ": too many 64-sketch blocks for one batch");
  const uint32_t n_batches = (uint32_t)((rb + bb - 1) / bb);
  // the largest batch in elements (sizes its layout): one batch holds the whole
  // set, several are measured on the sizes themselves (read back when the
  // caller gave device arrays only)
  uint64_t b_tot = R.total;
  if (n_batches > 1) {
    std::vector<uint32_t> own;
    const uint32_t* h_sizes = R.h_sizes;
    if (!h_sizes) {
      own.resize(R.n);
      SKS_HIP(sks::pinned_d2h(own.data(), R.sizes, (size_t)R.n * sizeof(uint32_t), c->stream));
      h_sizes = own.data();
    }
    b_tot = 0;
    for (uint64_t b0 = 0; b0 < R.n; b0 += bb * 64) {
      uint64_t t = 0;
      for (uint64_t i = b0; i < std::min<uint64_t>(R.n, b0 + bb * 64); ++i) t += h_sizes[i];
      b_tot = std::max(b_tot, t);
    }
  }
  const uint64_t tiles_max = (uint64_t)qb * bb;
  const size_t BW = sks::join_layout_boff_words(log_b);
  const uint32_t b_max_n = (uint32_t)std::min<uint64_t>(R.n, bb * 64);
  // c->lay: the group bounds, the query layout, one batch's layout, the hit
  // counter, [1 + n_batches][2] status words, the (I, J) list of a full batch,
  // its packed counts and the layout builds' temporary storage
  Carver cv;
  const Region<uint64_t> r_bounds = cv.take<uint64_t>((size_t)(G + 1) * ew);
  const LayoutRegions r_q = carve_layout(cv, Q.total, qb, BW, ew);
  const LayoutRegions r_b = carve_layout(cv, b_tot, (uint32_t)bb, BW, ew);
  const Region<unsigned long long> r_counter = cv.take<unsigned long long>(1);
  const Region<uint32_t> r_stat = cv.take<uint32_t>((size_t)(1 + n_batches) * 2);
  const Region<uint32_t> r_tiles = cv.take<uint32_t>(tiles_max * 2);
  const Region<int32_t> r_cnt = cv.take<int32_t>(tiles_max * 4096);
  const Region<char> r_tmp = cv.take<char>(std::max(sks::join_layout_temp_bytes(Q.n, log_b, ew),
                                                    sks::join_layout_temp_bytes(b_max_n, log_b, ew)) + 256);
  SKS_HIP(c->lay.reserve(cv.need()));
  // no more hits than pairs: a generous hit_cap does not size the buffers
  const uint64_t cap = d_hits ? std::min<uint64_t>(hit_cap, (uint64_t)Q.n * R.n) : 0;
  // c->hits: unsorted records | keys in, out | indices in, out
  Carver hv;
  const Region<sks_hit> r_raw = hv.take<sks_hit>(cap);
  const Region<uint64_t> r_kin = hv.take<uint64_t>(cap), r_kout = hv.take<uint64_t>(cap);
  const Region<uint64_t> r_iin = hv.take<uint64_t>(cap), r_iout = hv.take<uint64_t>(cap);
  hv.take<char>(256);
  SKS_HIP(c->hits.reserve(hv.need()));
  void* w = c->lay.ptr;
  uint64_t* bounds = r_bounds.in(w);
  const LayoutArrays AQ = r_q.in(w), AB = r_b.in(w);
  const sks::JoinLayout LQ = view_of(AQ), LB = view_of(AB);
  unsigned long long* counter = r_counter.in(w);
  uint32_t* stat = r_stat.in(w);
  uint32_t* tiles = r_tiles.in(w);
  int32_t* cnt = r_cnt.in(w);
  void* tmp = r_tmp.in(w);
  sks_hit* raw = r_raw.in(c->hits.ptr);
  // the counter and every status word are one span, cleared and read back together
  const size_t span = r_tiles.off - r_counter.off;

  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));
  SKS_HIP(hipMemsetAsync(counter, 0, span, c->stream));
  // tile bj * qb + qi = (query block qi, batch block bj): queries are global
  // blocks [0, qb), the batch's blocks follow them, so I < J; a shorter last
  // batch joins a prefix of the same list
  {
    std::vector<uint32_t> h_tiles(tiles_max * 2);
    for (uint64_t bj = 0; bj < bb; ++bj)
      for (uint32_t qi = 0; qi < qb; ++qi) {
        h_tiles[2 * (bj * qb + qi)] = qi;
        h_tiles[2 * (bj * qb + qi) + 1] = qb + (uint32_t)bj;
      }
    SKS_HIP(sks::pinned_h2d(tiles, h_tiles.data(), h_tiles.size() * 4, c->stream));
  }
  if (h_bounds)
    SKS_HIP(sks::pinned_h2d(bounds, h_bounds->data(), (size_t)(G + 1) * 8 * ew, c->stream));
  else
    SKS_HIP(sks::join_layout_bounds(R.data, R.starts, R.sizes, R.n, log_b, ew, bounds, c->stream));
  // the query layout, once
  SKS_HIP(sks::join_layout_build(Q.data, Q.starts, Q.sizes, Q.n, log_b, ew, bounds, tmp, AQ.vals, AQ.masks, AQ.boff,
                                 AQ.bstart, stat, c->join_check, c->stream));
  SKS_TRY(sks_ctx_ani_table(c, Q.max_size, kmer_num_ones));
  sks::JoinAni root{};  // only the context's table, if it is for this k
  attach_ani_root(c, kmer_num_ones, root);
  for (uint32_t b = 0; b < n_batches; ++b) {
    const uint32_t r0 = (uint32_t)(b * bb * 64), rn = (uint32_t)std::min<uint64_t>(R.n - r0, bb * 64);
    const uint32_t nbb = (rn + 63) / 64;
    const uint64_t nt = (uint64_t)qb * nbb;
    uint32_t* bstat = stat + 2 * (1 + b);
    // the batch's layout with the query layout's log_b and bounds; its second
    // launch clears the batch's count tiles
    const sks::ZeroSpans zs{{reinterpret_cast<uint32_t*>(cnt), nullptr, nullptr}, {nt * 4096, 0, 0}};
    SKS_HIP(sks::join_layout_build(R.data, R.starts + r0, R.sizes + r0, rn, log_b, ew, bounds, tmp, AB.vals, AB.masks,
                                   AB.boff, AB.bstart, bstat, c->join_check, c->stream, &zs));
    // rows: the query layout (block 0 = global block 0); columns: the batch
    // (block 0 = global block qb); every cell of the (qb + nbb) * 64 square is
    // in range for the join, the filter drops the padding rows and columns
    SKS_HIP(sks::join_launch(LQ, 0, LB, 0u - qb, (qb + nbb) * 64, log_b, ew, true, 0, (qb + nbb) * 64, 0, nt, tiles,
                             true, cnt, c->join_check, c->stream));
    SKS_HIP(sks::launch_search_hits(cnt, qb, nbb, Q.n, r0, rn, Q.sizes, min_containment, min_shared, kmer_num_ones,
                                    root.root, root.root_size, stat, bstat, d_hits ? raw : nullptr, cap, counter,
                                    c->stream));
  }
  // the count and every layout's status (one wait)
  std::vector<uint32_t> h_stat(span / 4);
  SKS_HIP(sks::pinned_d2h(h_stat.data(), counter, span, c->stream));
  const size_t s0 = (r_stat.off - r_counter.off) / 4;
  for (uint32_t b = 0; b <= n_batches; ++b)
    if (h_stat[s0 + 2 * b + 1]) {
      SKS_HIP(hipEventRecord(c->ev_end, c->stream));
      if (invalid_layout) *invalid_layout = true;
      return sks::fail(SKS_E_UNSUPPORTED, me + ": the join layout of " +
                                              (b ? "reference batch " + std::to_string(b - 1) : std::string("the queries")) +
                                              " could not be placed (invalid layout); no hits are reported");
    }
  const uint64_t found = (uint64_t)h_stat[0] | ((uint64_t)h_stat[1] << 32);
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
  if (q_total >= (1ull << 32) || r_total >= (1ull << 32))
    return sks::fail(SKS_E_UNSUPPORTED, "sks_search: >= 2^32 elements in one set");
  const SearchSide Q{d_q_data, d_q_starts, d_q_sizes, q_n, q_max_size, q_total, nullptr};
  const SearchSide R{d_r_data, d_r_starts, d_r_sizes, r_n, r_max_size, r_total, nullptr};
  return search_core(c, "sks_search", Q, R, elem_words, kmer_num_ones, min_containment, min_shared, nullptr, d_hits,
                     hit_cap, n_hits);
}

int sks_search_sets(sks_ctx* c, const sks_sketch_set* queries, const sks_sketch_set* refs, double min_containment,
                    int32_t min_shared, sks_hit* d_hits, uint64_t hit_cap, uint64_t* n_hits) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_search_sets: null ctx");
  if (!queries || !refs || !n_hits) return sks::fail(SKS_E_ARG, "sks_search_sets: null argument");
  *n_hits = 0;
  if (!(min_containment == min_containment)) return sks::fail(SKS_E_ARG, "sks_search_sets: min_containment is NaN");
  sks_sketch_info qi{}, ri{};
  SKS_TRY(sks_sketch_set_info(queries, &qi));
  SKS_TRY(sks_sketch_set_info(refs, &ri));
  const char* field = nullptr;
  if (qi.window != ri.window) field = "window";
  else if (qi.mask[0] != ri.mask[0] || qi.mask[1] != ri.mask[1]) field = "mask";
  else if (qi.elem_words != ri.elem_words) field = "elem_words";
  else if (qi.policy.kind != ri.policy.kind) field = "policy kind";
  else if (qi.policy.flavour != ri.policy.flavour) field = "hash flavour";
  else if (qi.policy.nonce != ri.policy.nonce) field = "nonce";
  else if (qi.policy.kind == SKS_FRAC_MOD && qi.policy.param != ri.policy.param) field = "policy param (FracMinHash c)";
  if (field)
    return sks::fail(SKS_E_ARG, std::string("sks_search_sets: the query and reference sets differ in ") + field);
  if (queries->device != c->device || refs->device != c->device)
    return sks::fail(SKS_E_ARG, "sks_search_sets: a set lives on another device than the context");
  const int k = (__builtin_popcountll(qi.mask[0]) + __builtin_popcountll(qi.mask[1])) / 2;
  if (k <= 0) return sks::fail(SKS_E_ARG, "sks_search_sets: the sets' mask selects no position");
  auto side = [](const sks_sketch_set* s) {
    SearchSide S{s->d_data(), s->d_starts(), s->d_sizes(), s->n, 0, 0, s->sizes.data()};
    for (uint32_t v : s->sizes) {
      S.max_size = std::max(S.max_size, v);
      S.total += v;
    }
    return S;
  };
  const SearchSide Q = side(queries), R = side(refs);
  if (Q.total >= (1ull << 32) || R.total >= (1ull << 32))
    return sks::fail(SKS_E_UNSUPPORTED, "sks_search_sets: >= 2^32 elements in one set");
  // group bounds fixed by the mask: no sampling pass, the same for every batch
  const uint32_t log_b = sks::join_log_b(std::max<uint32_t>(std::max(Q.max_size, R.max_size), 1));
  std::vector<uint64_t> h_bounds((size_t)(sks::join_layout_groups(log_b) + 1) * qi.elem_words);
  SKS_TRY(sks_join_layout_bounds_for_mask(qi.mask, log_b, qi.elem_words, h_bounds.data()));
  bool invalid = false;
  const int rc = search_core(c, "sks_search_sets", Q, R, qi.elem_words, k, min_containment, min_shared, &h_bounds,
                             d_hits, hit_cap, n_hits, &invalid);
  if (!invalid) return rc;
  // k-mers far from uniform overfilled a group of the mask's bounds: once more
  // with bounds sampled from the references (SKS_E_UNSUPPORTED if that fails too)
  return search_core(c, "sks_search_sets", Q, R, qi.elem_words, k, min_containment, min_shared, nullptr, d_hits,
                     hit_cap, n_hits);
}

}  // extern "C"
