// Post-processing of one scan pass of a sketch build: from the record regions
// of the segments that fitted to their final sketches in one device block.
// choose_post_path (build_plan.hpp) names the pipeline; each pipeline is one
// function below, a straight line over named working columns.
#include "build_internal.hpp"

using namespace sks;

namespace {

constexpr uint64_t kRetry = ~0ull;  // a segment's size while it has to go round again

// What every pipeline starts from: the k segments' record regions and their
// dense layout.  The arena is not uploaded yet (the fused pipeline adds to it).
struct PostIn {
  uint32_t k;
  uint64_t T, max_len;                 // records in all, and in the longest region
  std::vector<uint64_t> cnt, csr, thr; // [k] records, [k + 1] their prefix, [k] scan thresholds
  MetaArena arena;
  size_t o_src, o_csr, o_uniq;         // record offsets, csr, k zeroed words for the distinct counts
  uint64_t* d_src() const { return arena.ptr(o_src); }
  uint64_t* d_csr() const { return arena.ptr(o_csr); }
  uint64_t* d_uniq() const { return arena.ptr(o_uniq); }
};

uint64_t* rec(const sks_ctx* c, int r) { return reinterpret_cast<uint64_t*>(c->rec[r].ptr); }
uint32_t* flags(sks_ctx* c) { return reinterpret_cast<uint32_t*>(c->flag.ptr); }
uint64_t* positions(sks_ctx* c) { return reinterpret_cast<uint64_t*>(c->pos.ptr); }

// The unfused pipelines' working columns, flags and scan positions for T records.
int reserve_work(sks_ctx* c, uint64_t T) {
  SKS_TRY(reserve_cols(c, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, T + 1));
  SKS_HIP(c->flag.reserve((T + 1) * sizeof(uint32_t)));
  SKS_HIP(c->pos.reserve((T + 1) * sizeof(uint64_t)));
  return SKS_OK;
}

// Narrow bottom-s, every genome's candidates in one workgroup's registers:
// sort, unique and select per genome in one kernel (post.hip k_bottom_fused),
// then the selected runs packed into the pass's block.
int post_bottom_fused(BuildState& S, PostIn& in, std::vector<uint64_t>& size, DevBlock& out) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  const uint32_t k = in.k;
  std::vector<uint64_t> may_retry, pad(1, 0);  // pad: each genome's min(s, candidates) slots
  for (uint32_t i = 0; i < k; ++i) {
    may_retry.push_back(in.thr[i] != ~0ull ? 1 : 0);
    pad.push_back(pad.back() + std::min<uint64_t>(S.pol.param, in.cnt[i]));
  }
  const size_t o_cnt = in.arena.add(in.cnt), o_retry = in.arena.add(may_retry), o_pad = in.arena.add(pad),
               o_res = in.arena.add_zero(k);
  SKS_TRY(in.arena.upload());
  SKS_TRY(reserve_cols(c, {5}, pad[k] + 1));
  uint64_t* padded = col(c, 5);
  SKS_HIP(sks::launch_bottom_fused(rec(c, 0), in.d_src(), in.arena.ptr(o_cnt), in.arena.ptr(o_retry),
                                   in.arena.ptr(o_pad), k, in.max_len, S.pol.param, S.key_bits, S.runs, S.kconst,
                                   S.pol.flavour, padded, in.arena.ptr(o_res), st));
  std::vector<uint64_t> res(k);
  SKS_HIP(sks::pinned_d2h(res.data(), in.arena.ptr(o_res), k * sizeof(uint64_t), st));
  std::vector<uint64_t> limit(k, 0);
  uint64_t max_lim = 0;
  for (uint32_t i = 0; i < k; ++i) {
    if (res[i] == ~0ull) continue;  // too few distinct candidates under the threshold
    limit[i] = size[i] = res[i];
    max_lim = std::max(max_lim, res[i]);
  }
  const std::vector<uint64_t> dense = prefix(limit);
  MetaArena arena2(c);  // uploads are stream-ordered: safe to rewrite the arena
  const size_t o_psrc = arena2.add(pad), o_pdst = arena2.add(dense);
  SKS_TRY(arena2.upload());
  SKS_TRY(alloc_u64(out, dense[k], st));
  SKS_HIP(sks::compact_regions(padded, out.as<uint64_t>(), arena2.ptr(o_psrc), arena2.ptr(o_pdst), k, max_lim, st));
  return SKS_OK;
}

// The sorted records of a FracMinHash pass: K the column the runs are found in
// (128-bit: the high words, K2 the low, else K2 null), `keep` the key bits below
// a segment tag.
struct FracSorted {
  const uint64_t* K = nullptr;
  const uint64_t* K2 = nullptr;
  uint64_t keep = ~0ull;
};

// The first half of the FracMinHash pipelines: the records dense (narrow keys
// packed for the sorts) and sorted as `sort` says.  The arena is uploaded already.
int frac_compact_sort(BuildState& S, PostIn& in, FracSort sort, FracSorted* sorted) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  const uint32_t k = in.k;
  const uint64_t T = in.T, max_len = in.max_len;
  uint64_t* d_csr = in.d_csr();
  const int mask_lo_bits = end_bit_of(S.mask_lo), mask_hi_bits = end_bit_of(S.mask_hi);
  // tagged: the segment index above the key (128-bit: above the high word)
  const bool tagged = sort == FracSort::kTagged;
  const int tag_bits = sks::seg_tag_bits(k);
  const int tag_at = S.wide ? mask_hi_bits : S.key_bits;
  const uint64_t keep = tag_at >= 64 ? ~0ull : (1ull << tag_at) - 1;  // the key bits below the tag
  const std::vector<uint64_t> one_seg{0, T};
  const std::vector<uint64_t>& sort_off = tagged ? one_seg : in.csr;
  const uint64_t* d_sort_off = tagged ? nullptr : d_csr;
  uint64_t *key = col(c, 0), *hi = col(c, 1);  // dense: the narrow key or the low word; the high word
  SKS_HIP(sks::compact_regions(rec(c, 0), key, in.d_src(), d_csr, k, max_len, st, &S.runs,
                               tagged && !S.wide ? S.key_bits : -1));
  if (S.wide)
    SKS_HIP(sks::compact_regions(rec(c, 1), hi, in.d_src(), d_csr, k, max_len, st, nullptr,
                                 tagged ? mask_hi_bits : -1));
  const uint64_t*& K = sorted->K;
  const uint64_t*& K2 = sorted->K2;
  sorted->keep = keep;
  if (S.wide) {
    // (lo, hi) -> sort by lo, then stable by hi  => ascending 128-bit order
    SKS_HIP(sks::seg_sort_pairs(key, col(c, 3), hi, col(c, 4), T, sort_off, d_sort_off, mask_lo_bits, c->tmp, st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 4), col(c, 5), col(c, 3), col(c, 6), T, sort_off, d_sort_off,
                                mask_hi_bits + (tagged ? tag_bits : 0), c->tmp, st));
    K = col(c, 5);   // hi (tagged)
    K2 = col(c, 6);  // lo
  } else if (sort == FracSort::kTwoPass) {
    // keys too wide for a tag above them (2k + tag bits > 64): two stable
    // device-wide passes, by key with the segment as value, then by segment
    uint64_t* seg = col(c, 1);
    SKS_HIP(sks::launch_seg_ids(seg, d_csr, k, max_len, st));
    SKS_HIP(sks::seg_sort_pairs(key, col(c, 3), seg, col(c, 4), T, one_seg, nullptr, S.key_bits, c->tmp, st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 4), col(c, 5), col(c, 3), col(c, 6), T, one_seg, nullptr,
                                std::max(1, tag_bits), c->tmp, st));
    K = col(c, 6);
  } else {
    SKS_HIP(sks::seg_sort_keys(key, col(c, 3), T, sort_off, d_sort_off, S.key_bits + (tagged ? tag_bits : 0), c->tmp,
                               st));
    K = col(c, 3);
  }
  return SKS_OK;
}

// The distinct keys of every sorted segment at their rank among all distinct
// keys (dense CSR): narrow ones expanded into `out`, wide ones split into
// columns 7 and 8 and the first `n` interleaved into `out`.
int frac_scatter_distinct(BuildState& S, PostIn& in, const FracSorted& so, uint64_t n, uint64_t* out) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  if (!S.wide) {
    SKS_HIP(sks::seg_unique_scatter(so.K, nullptr, in.T, in.max_len, in.d_csr(), in.k, flags(c), positions(c), nullptr,
                                    nullptr, out, nullptr, st, &S.runs, so.keep));
  } else {
    SKS_HIP(sks::seg_unique_scatter(so.K2, so.K, in.T, in.max_len, in.d_csr(), in.k, flags(c), positions(c), nullptr,
                                    nullptr, col(c, 7), col(c, 8), st, nullptr, ~0ull, so.keep));
    SKS_HIP(sks::launch_interleave(col(c, 7), col(c, 8), n, out, st));
  }
  return SKS_OK;
}

// FracMinHash: the records dense, sorted as `sort` says, then the distinct
// keys of every segment written out.
int post_frac(BuildState& S, PostIn& in, FracSort sort, std::vector<uint64_t>& size, DevBlock& out) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  const uint32_t k = in.k;
  SKS_TRY(in.arena.upload());
  FracSorted so;
  SKS_TRY(frac_compact_sort(S, in, sort, &so));
  SKS_HIP(sks::seg_unique_scan(so.K, so.K2, in.T, in.max_len, in.d_csr(), k, flags(c), positions(c), in.d_uniq(),
                               c->tmp, st));
  SKS_HIP(sks::pinned_d2h(size.data(), in.d_uniq(), k * sizeof(uint64_t), st));
  uint64_t U = 0;
  for (uint64_t v : size) U += v;
  SKS_TRY(alloc_u64(out, U * S.ew, st));
  return frac_scatter_distinct(S, in, so, U, out.as<uint64_t>());
}

// The counted FracMinHash pipeline (sks_sketch_build_counted): as post_frac, and
// the length of every run of equal keys becomes the abundance of its element
// (abund.hip).  Limits that keep everything: the distinct counts are read back
// and the elements and run lengths go straight into the pass's blocks.  Other
// limits: the distinct elements and their run lengths are laid out in working
// columns (column 2 the runs' first indices, 1 the lengths, 7 or 9 the elements,
// 0 the bitmap), trimmed by the pass sks_sketch_set_abund_trim runs, chunked by
// the record counts (which bound the distinct counts the device holds), and the
// trimmed sizes are read back.  Either way one host round trip.
int post_frac_counted(BuildState& S, PostIn& in, FracSort sort, std::vector<uint64_t>& size, DevBlock& out,
                      DevBlock& out_abund) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  const uint32_t k = in.k;
  const uint64_t T = in.T, max_len = in.max_len;
  const bool trims = !abund_keeps_all(S.min_abund, S.max_abund);
  std::vector<uint64_t> chunk_off, dense_off;
  size_t o_chunk = 0, o_starts = 0, o_sizes = 0, o_nstarts = 0, o_nsizes = 0;
  uint64_t n_chunks = 0;
  if (trims) {
    std::vector<uint32_t> bound(k);
    for (uint32_t i = 0; i < k; ++i) {
      if (in.cnt[i] >> 32)
        return sks::fail(SKS_E_UNSUPPORTED, "sks_sketch_build_counted: >= 2^32 records in a segment");
      bound[i] = (uint32_t)in.cnt[i];
    }
    chunk_prefixes(bound, &chunk_off, &dense_off);
    n_chunks = chunk_off[k];
    o_chunk = in.arena.add(chunk_off);
    o_starts = in.arena.add_zero(k);
    o_sizes = in.arena.add_zero(k);   // u32 each, in u64 slots
    o_nstarts = in.arena.add_zero(k);
    o_nsizes = in.arena.add_zero(k);  // u32 each
    // the working columns, flags and positions also serve the trim: sized for both before anything is queued
    SKS_TRY(reserve_cols(c, {0}, std::max<uint64_t>(T + 1, filter_bitmap_words(n_chunks))));
    if (S.wide) SKS_TRY(reserve_cols(c, {9}, 2 * (T + 1)));
    SKS_HIP(c->flag.reserve((std::max<uint64_t>(T, n_chunks) + 1) * sizeof(uint32_t)));
    SKS_HIP(c->pos.reserve((std::max<uint64_t>(T, n_chunks) + 1) * sizeof(uint64_t)));
  }
  SKS_TRY(in.arena.upload());
  uint64_t* d_csr = in.d_csr();
  FracSorted so;
  SKS_TRY(frac_compact_sort(S, in, sort, &so));
  SKS_HIP(sks::seg_unique_scan(so.K, so.K2, T, max_len, d_csr, k, flags(c), positions(c), in.d_uniq(), c->tmp, st));
  uint64_t* run_start = col(c, 2);
  if (!trims) {
    SKS_HIP(sks::pinned_d2h(size.data(), in.d_uniq(), k * sizeof(uint64_t), st));
    uint64_t U = 0;
    for (uint64_t v : size) U += v;
    SKS_TRY(alloc_u64(out, U * S.ew, st));
    SKS_HIP(out_abund.alloc(std::max<uint64_t>(U, 1) * sizeof(uint32_t), st));
    SKS_TRY(frac_scatter_distinct(S, in, so, U, out.as<uint64_t>()));
    SKS_HIP(sks::abund_run_lengths(flags(c), positions(c), d_csr, k, max_len, run_start, out_abund.as<uint32_t>(),
                                   nullptr, nullptr, st));
    return SKS_OK;
  }
  uint32_t* lengths = reinterpret_cast<uint32_t*>(col(c, 1));
  uint64_t* distinct = S.wide ? col(c, 9) : col(c, 7);
  uint64_t* d_starts = in.arena.ptr(o_starts);
  uint32_t* d_sizes = reinterpret_cast<uint32_t*>(in.arena.ptr(o_sizes));
  uint64_t* d_nstarts = in.arena.ptr(o_nstarts);
  uint32_t* d_nsizes = reinterpret_cast<uint32_t*>(in.arena.ptr(o_nsizes));
  SKS_HIP(sks::abund_run_lengths(flags(c), positions(c), d_csr, k, max_len, run_start, lengths, d_starts, d_sizes,
                                 st));
  // the distinct count is on the device only: T bounds it (the interleave of a wide pass moves T pairs)
  SKS_TRY(frac_scatter_distinct(S, in, so, T, distinct));
  // the flags and positions are spent: the trim's chunk counters take their place
  AbundTrimArgs a{distinct, lengths, d_starts, d_sizes, in.arena.ptr(o_chunk), k, S.min_abund, S.max_abund};
  SKS_HIP(sks::abund_trim_mark(a, n_chunks, col(c, 0), chunk_counts(c), st));
  SKS_HIP(sks::downsample_offsets(chunk_counts(c), n_chunks, chunk_offs(c), a.chunk_off, k, d_nstarts, d_nsizes,
                                  c->tmp, st));
  std::vector<uint32_t> kept(k, 0);
  SKS_HIP(sks::pinned_d2h(kept.data(), d_nsizes, k * sizeof(uint32_t), st));
  uint64_t U = 0;
  for (uint32_t i = 0; i < k; ++i) {
    if (kept[i] > in.cnt[i])
      return sks::fail(SKS_E_HIP, "sks_sketch_build_counted: a sketch is larger than its records");
    size[i] = kept[i];
    U += kept[i];
  }
  SKS_TRY(alloc_u64(out, U * S.ew, st));
  SKS_HIP(out_abund.alloc(std::max<uint64_t>(U, 1) * sizeof(uint32_t), st));
  SKS_HIP(sks::abund_trim_scatter(a, S.ew, n_chunks, col(c, 0), chunk_offs(c), out.as<uint64_t>(),
                                  out_abund.as<uint32_t>(), st));
  return SKS_OK;
}

// Once the distinct counts are known: a genome with s distinct candidates, or
// with an open threshold, is done with min(s, distinct) elements (its limit);
// the others (limit 0) keep kRetry as size and go round again.
std::vector<uint64_t> bottom_limits(const BuildState& S, const PostIn& in, const std::vector<uint64_t>& uniq,
                                    std::vector<uint64_t>& size) {
  const uint64_t s = S.pol.param;
  std::vector<uint64_t> limit(in.k, 0);
  for (uint32_t i = 0; i < in.k; ++i)
    if (uniq[i] >= s || in.thr[i] == ~0ull) limit[i] = size[i] = std::min<uint64_t>(s, uniq[i]);
  return limit;
}

// Bottom-s on (fmh, k-mer): order each genome's candidates by (fmh, k-mer),
// unique, keep the first s, and sort those by k-mer.  128-bit builds start
// here; a narrow one only arrives from post_bottom_select, with the arena
// uploaded, the fmh in column 0 and the k-mer in column 1.
int post_bottom_pairs(BuildState& S, PostIn& in, std::vector<uint64_t>& size, DevBlock& out) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  const uint32_t k = in.k;
  const uint64_t T = in.T, max_len = in.max_len;
  const int mask_lo_bits = end_bit_of(S.mask_lo), mask_hi_bits = end_bit_of(S.mask_hi);
  uint64_t max_thr = 0;
  for (uint64_t t : in.thr) max_thr = std::max(max_thr, t);
  if (S.wide) SKS_TRY(in.arena.upload());
  uint64_t* d_csr = in.d_csr();
  uint32_t* d_flag = flags(c);
  uint64_t* d_pos = positions(c);
  const uint64_t* LO;  // columns ordered by (fmh, k-mer)
  const uint64_t* HI = nullptr;
  if (!S.wide) {
    uint64_t *fmh = col(c, 0), *kmer = col(c, 1);
    SKS_HIP(sks::seg_sort_pairs(fmh, col(c, 3), kmer, col(c, 4), T, in.csr, d_csr, end_bit_of(max_thr), c->tmp, st));
    LO = col(c, 4);
    SKS_HIP(sks::seg_unique_scan(col(c, 3), nullptr, T, max_len, d_csr, k, d_flag, d_pos, in.d_uniq(), c->tmp, st));
  } else {
    uint64_t *fmh = col(c, 0), *lo = col(c, 1), *hi = col(c, 2), *idx = col(c, 9);
    SKS_HIP(sks::compact_regions(rec(c, 0), fmh, in.d_src(), d_csr, k, max_len, st, &S.runs, -1));
    SKS_HIP(sks::compact_regions(rec(c, 1), lo, in.d_src(), d_csr, k, max_len, st, nullptr, -1));
    SKS_HIP(sks::compact_regions(rec(c, 2), hi, in.d_src(), d_csr, k, max_len, st));
    // order (fmh, hi, lo) by an index permutation (LSD: lo, hi, fmh)
    SKS_HIP(sks::launch_iota(idx, T, st));
    SKS_HIP(sks::seg_sort_pairs(lo, col(c, 3), idx, col(c, 4), T, in.csr, d_csr, 64, c->tmp, st));
    SKS_HIP(sks::launch_gather(hi, col(c, 4), T, col(c, 5), st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 5), col(c, 3), col(c, 4), col(c, 6), T, in.csr, d_csr, mask_hi_bits, c->tmp,
                                st));
    SKS_HIP(sks::launch_gather(fmh, col(c, 6), T, col(c, 5), st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 5), col(c, 3), col(c, 6), col(c, 4), T, in.csr, d_csr, end_bit_of(max_thr),
                                c->tmp, st));
    SKS_HIP(sks::launch_gather(lo, col(c, 4), T, col(c, 7), st));
    SKS_HIP(sks::launch_gather(hi, col(c, 4), T, col(c, 8), st));
    LO = col(c, 7);
    HI = col(c, 8);
    SKS_HIP(sks::seg_unique_scan(LO, HI, T, max_len, d_csr, k, d_flag, d_pos, in.d_uniq(), c->tmp, st));
  }
  std::vector<uint64_t> uniq(k);
  SKS_HIP(sks::pinned_d2h(uniq.data(), in.d_uniq(), k * sizeof(uint64_t), st));
  const std::vector<uint64_t> limit = bottom_limits(S, in, uniq, size);
  // not-done segments get limit 0, so this prefix is also the pass's CSR
  const std::vector<uint64_t> dst = prefix(limit);
  const uint64_t U = dst[k];
  MetaArena arena2(c);  // uploads are stream-ordered: safe to rewrite the arena
  const size_t o_csr2 = arena2.add(in.csr), o_lim = arena2.add(limit), o_dst = arena2.add(dst);
  SKS_TRY(arena2.upload());
  d_csr = arena2.ptr(o_csr2);
  uint64_t *d_lim = arena2.ptr(o_lim), *d_dst = arena2.ptr(o_dst);
  SKS_TRY(alloc_u64(out, U * S.ew, st));
  if (!S.wide) {
    SKS_HIP(sks::seg_unique_scatter(LO, nullptr, T, max_len, d_csr, k, d_flag, d_pos, d_lim, d_dst, col(c, 5),
                                    nullptr, st));
    SKS_HIP(sks::seg_sort_keys(col(c, 5), out.as<uint64_t>(), U, dst, d_dst, mask_lo_bits, c->tmp, st));
  } else {
    SKS_HIP(sks::seg_unique_scatter(LO, HI, T, max_len, d_csr, k, d_flag, d_pos, d_lim, d_dst, col(c, 0), col(c, 1),
                                    st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 0), col(c, 3), col(c, 1), col(c, 4), U, dst, d_dst, 64, c->tmp, st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 4), col(c, 5), col(c, 3), col(c, 6), U, dst, d_dst, mask_hi_bits, c->tmp, st));
    SKS_HIP(sks::launch_interleave(col(c, 6), col(c, 5), U, out.as<uint64_t>(), st));
  }
  return SKS_OK;
}

// Narrow bottom-s: sort the candidate k-mers, unique them, then select the s
// with the smallest (fmh, k-mer) per genome in LDS (k_bottom_select, post.hip):
// one key-only sort instead of a (fmh, k-mer) pair sort followed by a second
// sort.  A genome with more distinct candidates than the LDS select holds
// sends the pass to post_bottom_pairs.
int post_bottom_select(BuildState& S, PostIn& in, std::vector<uint64_t>& size, DevBlock& out) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  const uint32_t k = in.k;
  const uint64_t T = in.T, max_len = in.max_len, s = S.pol.param;
  SKS_TRY(in.arena.upload());
  uint64_t* d_csr = in.d_csr();
  uint64_t *packed = col(c, 0), *sorted = col(c, 3);  // the candidates' packed k-mers, dense; then sorted
  SKS_HIP(sks::compact_regions(rec(c, 0), packed, in.d_src(), d_csr, k, max_len, st, &S.runs, -1));
  SKS_HIP(sks::seg_sort_keys(packed, sorted, T, in.csr, d_csr, S.key_bits, c->tmp, st));
  SKS_HIP(sks::seg_unique_scan(sorted, nullptr, T, max_len, d_csr, k, flags(c), positions(c), in.d_uniq(), c->tmp,
                               st));
  std::vector<uint64_t> uniq(k);
  SKS_HIP(sks::pinned_d2h(uniq.data(), in.d_uniq(), k * sizeof(uint64_t), st));
  uint64_t max_keep_uniq = 0;
  for (uint32_t i = 0; i < k; ++i)
    if (uniq[i] >= s || in.thr[i] == ~0ull) max_keep_uniq = std::max(max_keep_uniq, uniq[i]);
  if (max_keep_uniq > sks::bottom_select_capacity()) {
    // the general path, on (fmh, k-mer) pairs: column 0 the fmh, column 1 the k-mer
    SKS_HIP(sks::launch_bits_expand(packed, T, S.runs, st));
    SKS_HIP(hipMemcpyAsync(col(c, 1), packed, T * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    SKS_HIP(sks::launch_fmh_narrow(packed, T, S.kconst, S.pol.flavour, st));
    return post_bottom_pairs(S, in, size, out);
  }
  const std::vector<uint64_t> limit = bottom_limits(S, in, uniq, size);
  const std::vector<uint64_t> dst = prefix(limit), uoff = prefix(uniq);
  // every distinct candidate, contiguous per genome at uoff
  uint64_t* distinct = col(c, 5);
  SKS_HIP(sks::seg_unique_scatter(sorted, nullptr, T, max_len, d_csr, k, flags(c), positions(c), nullptr, nullptr,
                                  distinct, nullptr, st, &S.runs));
  MetaArena arena2(c);  // uploads are stream-ordered: safe to rewrite the arena
  const size_t o_uoff = arena2.add(uoff), o_lim = arena2.add(limit), o_dst = arena2.add(dst);
  SKS_TRY(arena2.upload());
  SKS_TRY(alloc_u64(out, dst[k], st));
  SKS_HIP(sks::launch_bottom_select(distinct, arena2.ptr(o_uoff), arena2.ptr(o_dst), arena2.ptr(o_lim), k, S.kconst,
                                    S.pol.flavour, out.as<uint64_t>(), st));
  return SKS_OK;
}

}  // namespace

int sks::post_process(BuildState& S, const std::vector<uint32_t>& seg_ids, const std::vector<uint64_t>& out_off,
                      const std::vector<uint64_t>& counts, const std::vector<uint64_t>& thresh,
                      const std::vector<uint32_t>& ok, std::vector<PassOut>& passes,
                      std::vector<uint32_t>& retry_local, std::vector<uint64_t>& final_size_local) {
  const uint32_t k = (uint32_t)ok.size();
  if (k == 0) return SKS_OK;
  PostIn in{k, 0, 0, std::vector<uint64_t>(k), {}, std::vector<uint64_t>(k), MetaArena(S.c), 0, 0, 0};
  std::vector<uint64_t> src_off(k);
  for (uint32_t i = 0; i < k; ++i) {
    src_off[i] = out_off[ok[i]];
    in.cnt[i] = counts[ok[i]];
    in.thr[i] = thresh[ok[i]];
    in.max_len = std::max(in.max_len, in.cnt[i]);
  }
  in.csr = prefix(in.cnt);
  in.T = in.csr[k];
  in.o_src = in.arena.add(src_off);
  in.o_csr = in.arena.add(in.csr);
  in.o_uniq = in.arena.add_zero(k);

  const PostPath path = sks::choose_post_path(S.pol.kind == SKS_BOTTOM_S, S.wide, k, in.max_len, S.key_bits,
                                              end_bit_of(S.mask_hi), sks::bottom_fused_capacity(), S.knobs);
  if (path.pipe != PostPipe::kBottomFused) SKS_TRY(reserve_work(S.c, in.T));
  PassOut po;
  std::vector<uint64_t> size(k, kRetry);
  int rc = SKS_OK;
  switch (path.pipe) {
    case PostPipe::kBottomFused: rc = post_bottom_fused(S, in, size, po.d); break;
    case PostPipe::kFrac:
      rc = S.counted ? post_frac_counted(S, in, path.sort, size, po.d, po.abund)
                     : post_frac(S, in, path.sort, size, po.d);
      break;
    case PostPipe::kBottomSelect: rc = post_bottom_select(S, in, size, po.d); break;
    case PostPipe::kBottomPairs: rc = post_bottom_pairs(S, in, size, po.d); break;
  }
  SKS_TRY(rc);
  // the finished segments, in order, are the pass's CSR; the others go round again
  po.off.assign(1, 0);
  for (uint32_t i = 0; i < k; ++i) {
    if (size[i] == kRetry) {
      retry_local.push_back(ok[i]);
      continue;
    }
    final_size_local[ok[i]] = size[i];
    po.segs.push_back(seg_ids[ok[i]]);
    po.off.push_back(po.off.back() + size[i]);
  }
  // no stream sync: the pass's outputs are consumed in stream order
  passes.push_back(std::move(po));
  return SKS_OK;
}
