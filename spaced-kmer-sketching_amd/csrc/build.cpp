// C-ABI implementation (include/sks.h): sketch builds — the scan's metadata,
// the general pass loop with its post-processing, the two single-genome fast
// paths — the sketch-set accessors and the ordered k-mer lists.
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <utility>

#include "sks_ctx.hpp"
#include "sks_hash.hpp"

using namespace sks;

namespace {

std::vector<uint64_t> prefix(const std::vector<uint64_t>& v) {
  std::vector<uint64_t> o(v.size() + 1, 0);
  for (size_t i = 0; i < v.size(); ++i) o[i + 1] = o[i] + v[i];
  return o;
}

// One completed pass: final sketches of `segs` (global segment ids) in CSR.
struct PassOut {
  uint64_t* d = nullptr;          // elements (elem_words u64 each)
  size_t bytes = 0;               // allocation size of d
  std::vector<uint32_t> segs;
  std::vector<uint64_t> off;      // CSR in elements, size segs.size() + 1
};

// Pass buffers are only used on the ctx stream, synchronised before this runs.
void free_passes(std::vector<PassOut>& passes) {
  for (auto& p : passes)
    if (p.d) dev_release(p.d, p.bytes);
  passes.clear();
}

struct BuildState {
  sks_ctx* c;
  int w;
  bool wide;
  int ew;
  uint64_t mask_lo, mask_hi;
  sks_policy pol;
  uint64_t kconst;
  sks::DivTest dt;
  // narrow keys are packed to their mask bits for the sorts (sks::BitRuns) and
  // expanded again when the unique elements are written out; wide keys are not
  sks::BitRuns runs;
  int key_bits;
};

// Post-process the segments `ok` (pass-local indices into the pass arrays) whose
// survivors sit in the record regions [out_off[i], out_off[i] + count[i]).
// Appends a PassOut; for bottom-s reports segments that need a larger threshold.
int post_process(BuildState& S, const std::vector<uint32_t>& seg_ids, const std::vector<uint64_t>& out_off,
                 const std::vector<uint64_t>& counts, const std::vector<uint64_t>& thresh,
                 const std::vector<uint32_t>& ok, std::vector<PassOut>& passes, std::vector<uint32_t>& retry_local,
                 std::vector<uint64_t>& final_size_local) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  const uint32_t k = (uint32_t)ok.size();
  if (k == 0) return SKS_OK;
  std::vector<uint64_t> src_off(k), cnt(k);
  uint64_t max_len = 0;
  for (uint32_t i = 0; i < k; ++i) {
    src_off[i] = out_off[ok[i]];
    cnt[i] = counts[ok[i]];
    max_len = std::max(max_len, cnt[i]);
  }
  std::vector<uint64_t> csr = prefix(cnt);
  const uint64_t T = csr[k];
  const bool bottom = S.pol.kind == SKS_BOTTOM_S;

  MetaArena arena(c);
  size_t o_src = arena.add(src_off), o_csr = arena.add(csr), o_uniq = arena.add_zero(k);
  // narrow bottom-s with every genome's candidates in one workgroup's registers:
  // sort, unique and select per genome in one kernel (post.hip k_bottom_fused).
  // A single genome goes the device-wide way instead: one workgroup sorting its
  // ~1.1 s candidates alone takes longer than the multi-workgroup radix sort
  // (config 2: 0.35 vs 0.30 ms per build; from two genomes on the fused kernel
  // wins, tools/ab_c2.sh)
  const bool fused = bottom && !S.wide && max_len <= sks::bottom_fused_capacity() &&
                     (k >= 2 || getenv("SKS_FUSED_SINGLE") != nullptr) &&
                     getenv("SKS_NO_FUSED_BOTTOM") == nullptr;
  std::vector<uint64_t> f_retry, f_pad(1, 0);
  size_t o_cnt = 0, o_retry = 0, o_pad = 0, o_res = 0;
  if (fused) {
    for (uint32_t i = 0; i < k; ++i) {
      f_retry.push_back(thresh[ok[i]] != ~0ull ? 1 : 0);
      f_pad.push_back(f_pad.back() + std::min<uint64_t>(S.pol.param, cnt[i]));
    }
    o_cnt = arena.add(cnt);
    o_retry = arena.add(f_retry);
    o_pad = arena.add(f_pad);
    o_res = arena.add_zero(k);
  }
  SKS_TRY(arena.upload());
  uint64_t* d_src = arena.ptr(o_src);
  uint64_t* d_csr = arena.ptr(o_csr);
  uint64_t* d_uniq = arena.ptr(o_uniq);

  if (fused) {
    SKS_TRY(reserve_cols(c, {5}, f_pad[k] + 1));
    SKS_HIP(sks::launch_bottom_fused(reinterpret_cast<uint64_t*>(c->rec[0].ptr), d_src, arena.ptr(o_cnt),
                                     arena.ptr(o_retry), arena.ptr(o_pad), k, max_len, S.pol.param, S.key_bits, S.runs,
                                     S.kconst, S.pol.flavour, col(c, 5), arena.ptr(o_res), st));
    std::vector<uint64_t> res(k);
    SKS_HIP(sks::pinned_d2h(res.data(), arena.ptr(o_res), k * sizeof(uint64_t), st));
    PassOut po;
    std::vector<uint64_t> limit(k, 0), keep_off(1, 0);
    uint64_t max_lim = 0;
    for (uint32_t i = 0; i < k; ++i) {
      if (res[i] == ~0ull) {
        retry_local.push_back(ok[i]);  // too few distinct candidates under the threshold
        continue;
      }
      limit[i] = res[i];
      max_lim = std::max(max_lim, res[i]);
      final_size_local[ok[i]] = res[i];
      po.segs.push_back(seg_ids[ok[i]]);
      keep_off.push_back(keep_off.back() + res[i]);
    }
    std::vector<uint64_t> dense = prefix(limit);
    MetaArena arena2(c);  // uploads are stream-ordered: safe to rewrite the arena
    const size_t o_psrc = arena2.add(f_pad), o_pdst = arena2.add(dense);
    SKS_TRY(arena2.upload());
    SKS_TRY(alloc_u64(&po.d, dense[k], &po.bytes));
    SKS_HIP(sks::compact_regions(col(c, 5), po.d, arena2.ptr(o_psrc), arena2.ptr(o_pdst), k, max_lim, st));
    po.off = keep_off;
    // no stream sync: the pass's outputs are consumed in stream order
    passes.push_back(po);
    return SKS_OK;
  }

  SKS_TRY(reserve_cols(c, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, T + 1));
  SKS_HIP(c->flag.reserve((T + 1) * sizeof(uint32_t)));
  SKS_HIP(c->pos.reserve((T + 1) * sizeof(uint64_t)));
  uint32_t* d_flag = reinterpret_cast<uint32_t*>(c->flag.ptr);
  uint64_t* d_pos = reinterpret_cast<uint64_t*>(c->pos.ptr);
  const uint64_t* rk = reinterpret_cast<uint64_t*>(c->rec[0].ptr);
  const uint64_t* rv = reinterpret_cast<uint64_t*>(c->rec[1].ptr);
  const uint64_t* rh = reinterpret_cast<uint64_t*>(c->rec[2].ptr);

  // dense columns, narrow keys packed (S.runs)
  const sks::BitRuns& runs = S.runs;
  const int key_bits = S.key_bits;
  const int mask_lo_bits = end_bit_of(S.mask_lo);
  const int mask_hi_bits = end_bit_of(S.mask_hi);
  // FracMinHash over several genomes: the segment index rides above the key (or,
  // 128-bit, above the high word) and every sort below is ONE device-wide radix
  // sort over all segments (compact_regions); a segmented sort gives each genome
  // one workgroup (reference sweep, 64 x 5 Mb at c = 200: 0.50 ms per narrow
  // sort, 2 x 0.68 ms per 128-bit one)
  const int tag_bits = sks::seg_tag_bits(k);
  const int tag_at = S.wide ? mask_hi_bits : key_bits;
  const bool tagged = !bottom && k >= 2 && tag_at + tag_bits <= 64 && getenv("SKS_SEGMENTED_SORT") == nullptr;
  const std::vector<uint64_t> one_seg{0, T};
  const std::vector<uint64_t>& sort_off = tagged ? one_seg : csr;
  const uint64_t* d_sort_off = tagged ? nullptr : d_csr;
  const uint64_t keep = tag_at >= 64 ? ~0ull : (1ull << tag_at) - 1;  // the key bits below the tag
  SKS_HIP(sks::compact_regions(rk, col(c, 0), d_src, d_csr, k, max_len, st, &runs, tagged && !S.wide ? key_bits : -1));
  // narrow bottom-s records carry the k-mer as key (its fmh is recomputed here)
  const bool has_val = S.wide || (bottom && S.wide);
  if (has_val)
    SKS_HIP(sks::compact_regions(rv, col(c, 1), d_src, d_csr, k, max_len, st, nullptr, tagged ? mask_hi_bits : -1));
  if (bottom && S.wide) SKS_HIP(sks::compact_regions(rh, col(c, 2), d_src, d_csr, k, max_len, st));

  uint64_t max_thr = 0;
  for (uint32_t i = 0; i < k; ++i) max_thr = std::max(max_thr, thresh[ok[i]]);

  PassOut po;
  for (uint32_t i = 0; i < k; ++i) po.segs.push_back(seg_ids[ok[i]]);
  std::vector<uint64_t> uniq(k);

  if (!bottom) {
    const uint64_t* K;   // sorted unique columns source
    const uint64_t* K2 = nullptr;
    if (!S.wide && (tagged || k < 2 || getenv("SKS_SEGMENTED_SORT"))) {
      SKS_HIP(sks::seg_sort_keys(col(c, 0), col(c, 3), T, sort_off, d_sort_off,
                                 key_bits + (tagged ? tag_bits : 0), c->tmp, st));
      K = col(c, 3);
    } else if (!S.wide) {
      // keys too wide for a tag above them (2k + tag bits > 64): two stable
      // device-wide passes, by key with the segment as value, then by segment
      SKS_HIP(sks::launch_seg_ids(col(c, 1), d_csr, k, max_len, st));
      SKS_HIP(sks::seg_sort_pairs(col(c, 0), col(c, 3), col(c, 1), col(c, 4), T, one_seg, nullptr, key_bits,
                                  c->tmp, st));
      SKS_HIP(sks::seg_sort_pairs(col(c, 4), col(c, 5), col(c, 3), col(c, 6), T, one_seg, nullptr,
                                  std::max(1, tag_bits), c->tmp, st));
      K = col(c, 6);
    } else {
      // (lo, hi) -> sort by lo, then stable by hi  => ascending 128-bit order
      SKS_HIP(sks::seg_sort_pairs(col(c, 0), col(c, 3), col(c, 1), col(c, 4), T, sort_off, d_sort_off,
                                  mask_lo_bits, c->tmp, st));
      SKS_HIP(sks::seg_sort_pairs(col(c, 4), col(c, 5), col(c, 3), col(c, 6), T, sort_off, d_sort_off,
                                  mask_hi_bits + (tagged ? tag_bits : 0), c->tmp, st));
      K = col(c, 5);   // hi (tagged)
      K2 = col(c, 6);  // lo
    }
    SKS_HIP(sks::seg_unique_scan(K, K2, T, max_len, d_csr, k, d_flag, d_pos, d_uniq, c->tmp, st));
    SKS_HIP(sks::pinned_d2h(uniq.data(), d_uniq, k * sizeof(uint64_t), st));
    po.off = prefix(uniq);
    const uint64_t U = po.off[k];
    SKS_TRY(alloc_u64(&po.d, U * S.ew, &po.bytes));
    if (!S.wide) {
      SKS_HIP(sks::seg_unique_scatter(K, nullptr, T, max_len, d_csr, k, d_flag, d_pos, nullptr, nullptr,
                                      po.d, nullptr, st, &runs, keep));
    } else {
      SKS_HIP(sks::seg_unique_scatter(K2, K, T, max_len, d_csr, k, d_flag, d_pos, nullptr, nullptr,
                                      col(c, 7), col(c, 8), st, nullptr, ~0ull, keep));
      SKS_HIP(sks::launch_interleave(col(c, 7), col(c, 8), U, po.d, st));
    }
    for (uint32_t i = 0; i < k; ++i) final_size_local[ok[i]] = uniq[i];
    passes.push_back(po);
    return SKS_OK;
  }

  // bottom-s
  const uint64_t s = S.pol.param;
  // Once uniq is known: a genome with s distinct candidates, or with an open
  // threshold, is done and joins po (segs, off) with the returned size; the
  // others (limit 0) go round again.
  auto keep_done = [&] {
    std::vector<uint64_t> limit(k, 0);
    po.segs.clear();
    po.off.assign(1, 0);
    for (uint32_t i = 0; i < k; ++i) {
      if (uniq[i] >= s || thresh[ok[i]] == ~0ull) {
        limit[i] = std::min<uint64_t>(s, uniq[i]);
        final_size_local[ok[i]] = limit[i];
        po.segs.push_back(seg_ids[ok[i]]);
        po.off.push_back(po.off.back() + limit[i]);
      } else {
        retry_local.push_back(ok[i]);  // too few candidates under the threshold
      }
    }
    return limit;
  };
  if (!S.wide) {
    // sort the candidate k-mers, unique them, then select the s with the smallest
    // (fmh, k-mer) per genome in LDS (k_bottom_select, post.hip): one key-only
    // sort instead of a (fmh, k-mer) pair sort followed by a second sort
    SKS_HIP(sks::seg_sort_keys(col(c, 0), col(c, 3), T, csr, d_csr, key_bits, c->tmp, st));
    SKS_HIP(sks::seg_unique_scan(col(c, 3), nullptr, T, max_len, d_csr, k, d_flag, d_pos, d_uniq, c->tmp, st));
    SKS_HIP(sks::pinned_d2h(uniq.data(), d_uniq, k * sizeof(uint64_t), st));
    uint64_t max_keep_uniq = 0;
    for (uint32_t i = 0; i < k; ++i)
      if (uniq[i] >= s || thresh[ok[i]] == ~0ull) max_keep_uniq = std::max(max_keep_uniq, uniq[i]);
    if (max_keep_uniq <= sks::bottom_select_capacity()) {
      const std::vector<uint64_t> limit = keep_done();
      std::vector<uint64_t> dst = prefix(limit), uoff = prefix(uniq);
      const uint64_t U = dst[k];
      // every distinct candidate, contiguous per genome at uoff
      SKS_HIP(sks::seg_unique_scatter(col(c, 3), nullptr, T, max_len, d_csr, k, d_flag, d_pos,
                                      nullptr, nullptr, col(c, 5), nullptr, st, &runs));
      MetaArena arena2(c);  // uploads are stream-ordered: safe to rewrite the arena
      size_t o_uoff = arena2.add(uoff), o_lim = arena2.add(limit), o_dst = arena2.add(dst);
      SKS_TRY(arena2.upload());
      SKS_TRY(alloc_u64(&po.d, U, &po.bytes));
      SKS_HIP(sks::launch_bottom_select(col(c, 5), arena2.ptr(o_uoff), arena2.ptr(o_dst),
                                        arena2.ptr(o_lim), k, S.kconst, S.pol.flavour, po.d, st));
      // no stream sync: the pass's outputs are consumed in stream order
      passes.push_back(po);
      return SKS_OK;
    }
    // a genome with more distinct candidates than the LDS select holds: the
    // general path below, on (fmh, k-mer) pairs
    SKS_HIP(sks::launch_bits_expand(col(c, 0), T, runs, st));
    SKS_HIP(hipMemcpyAsync(col(c, 1), col(c, 0), T * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    SKS_HIP(sks::launch_fmh_narrow(col(c, 0), T, S.kconst, S.pol.flavour, st));
  }
  const uint64_t* LO;  // columns ordered by (fmh, C)
  const uint64_t* HI = nullptr;
  if (!S.wide) {
    SKS_HIP(sks::seg_sort_pairs(col(c, 0), col(c, 3), col(c, 1), col(c, 4), T, csr, d_csr,
                                end_bit_of(max_thr), c->tmp, st));
    LO = col(c, 4);
    SKS_HIP(sks::seg_unique_scan(col(c, 3), nullptr, T, max_len, d_csr, k, d_flag, d_pos, d_uniq, c->tmp, st));
  } else {
    // order (fmh, hi, lo) by an index permutation (LSD: lo, hi, fmh)
    uint64_t* idx = col(c, 9);
    SKS_HIP(sks::launch_iota(idx, T, st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 1), col(c, 3), idx, col(c, 4), T, csr, d_csr, 64, c->tmp, st));
    SKS_HIP(sks::launch_gather(col(c, 2), col(c, 4), T, col(c, 5), st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 5), col(c, 3), col(c, 4), col(c, 6), T, csr, d_csr, mask_hi_bits, c->tmp, st));
    SKS_HIP(sks::launch_gather(col(c, 0), col(c, 6), T, col(c, 5), st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 5), col(c, 3), col(c, 6), col(c, 4), T, csr, d_csr,
                                end_bit_of(max_thr), c->tmp, st));
    SKS_HIP(sks::launch_gather(col(c, 1), col(c, 4), T, col(c, 7), st));  // lo
    SKS_HIP(sks::launch_gather(col(c, 2), col(c, 4), T, col(c, 8), st));  // hi
    LO = col(c, 7);
    HI = col(c, 8);
    SKS_HIP(sks::seg_unique_scan(LO, HI, T, max_len, d_csr, k, d_flag, d_pos, d_uniq, c->tmp, st));
  }
  SKS_HIP(sks::pinned_d2h(uniq.data(), d_uniq, k * sizeof(uint64_t), st));
  const std::vector<uint64_t> limit = keep_done();
  // not-done segments get limit 0, so this prefix is also po.off's layout
  std::vector<uint64_t> dst = prefix(limit);
  const uint64_t U = dst[k];
  MetaArena arena2(c);  // uploads are stream-ordered: safe to rewrite the arena
  size_t o_csr2 = arena2.add(csr), o_lim = arena2.add(limit), o_dst = arena2.add(dst);
  SKS_TRY(arena2.upload());
  d_csr = arena2.ptr(o_csr2);
  uint64_t* d_lim = arena2.ptr(o_lim);
  uint64_t* d_dst = arena2.ptr(o_dst);
  SKS_TRY(alloc_u64(&po.d, U * S.ew, &po.bytes));
  if (!S.wide) {
    SKS_HIP(sks::seg_unique_scatter(LO, nullptr, T, max_len, d_csr, k, d_flag, d_pos, d_lim, d_dst,
                                    col(c, 5), nullptr, st));
    SKS_HIP(sks::seg_sort_keys(col(c, 5), po.d, U, dst, d_dst, mask_lo_bits, c->tmp, st));
  } else {
    SKS_HIP(sks::seg_unique_scatter(LO, HI, T, max_len, d_csr, k, d_flag, d_pos, d_lim, d_dst, col(c, 0),
                                    col(c, 1), st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 0), col(c, 3), col(c, 1), col(c, 4), U, dst, d_dst, 64, c->tmp, st));
    SKS_HIP(sks::seg_sort_pairs(col(c, 4), col(c, 5), col(c, 3), col(c, 6), U, dst, d_dst, mask_hi_bits, c->tmp, st));
    SKS_HIP(sks::launch_interleave(col(c, 6), col(c, 5), U, po.d, st));
  }
  // no stream sync: the pass's outputs are consumed in stream order
  passes.push_back(po);
  return SKS_OK;
}

// The per-segment host arrays of one scan launch (launch-local segment index);
// the record regions lie back to back in segment order.
struct ScanSegs {
  std::vector<uint64_t> beg, end, thresh, cap, off;  // [m]; thresh: bottom-s pre-filter (~0: none)
  std::vector<uint64_t> tiles{0};                    // [m + 1] tiles before each segment
  uint64_t total_cap = 0;
  void push(uint64_t b, uint64_t e, uint64_t thr, uint64_t c) {
    beg.push_back(b);
    end.push_back(e);
    thresh.push_back(thr);
    cap.push_back(c);
    off.push_back(total_cap);
    tiles.push_back(tiles.back() + sks::scan_tiles_for(e - b));
    total_cap += c;
  }
  uint32_t m() const { return (uint32_t)beg.size(); }
  uint64_t n_tiles() const { return tiles.back(); }
};

// A scan's metadata on the device, laid out in this one place.  The arena holds,
// in this order: begin, end, tile prefix, threshold (not in list mode),
// capacity, record offset, the caller's `extra` words for its post kernel, the
// counters block, and the tile queue's counter (not in list mode).  The
// counters block is contiguous, so one read-back fetches it whole:
//   [0, m) survivors, 0, [m + 1, 2m + 1) windows, 0, then `result_words` words a fused post kernel writes
struct ScanMeta {
  sks::ScanParams p;
  uint64_t* extra;
  uint64_t* counters;
  uint64_t* results;
};

int scan_meta(const BuildState& S, const uint8_t* d_seq, const ScanSegs& g, bool list_mode,
              const std::vector<uint64_t>& extra, size_t result_words, ScanMeta* out) {
  sks_ctx* c = S.c;
  const size_t m = g.m();
  MetaArena arena(c);
  const size_t o_beg = arena.add(g.beg), o_end = arena.add(g.end), o_tiles = arena.add(g.tiles);
  const size_t o_thr = list_mode ? 0 : arena.add(g.thresh);
  const size_t o_cap = arena.add(g.cap), o_off = arena.add(g.off);
  const size_t o_extra = extra.empty() ? 0 : arena.add(extra);
  const size_t o_cnt = arena.add_zero(2 * (m + 1) + (result_words ? result_words + 1 : 0) - 1);
  const size_t o_queue = list_mode ? 0 : arena.add_zero(1);
  SKS_TRY(arena.upload());
  *out = {{}, arena.ptr(o_extra), arena.ptr(o_cnt), arena.ptr(o_cnt) + 2 * (m + 1)};
  sks::ScanParams& p = out->p;
  p.seq = d_seq;
  p.seg_begin = arena.ptr(o_beg);
  p.seg_end = arena.ptr(o_end);
  p.tile_prefix = arena.ptr(o_tiles);
  p.n_seg = g.m();
  p.n_tiles = g.n_tiles();
  p.w = S.w;
  p.mask_lo = S.mask_lo;
  p.mask_hi = S.mask_hi;
  p.kconst = S.kconst;
  p.low_mask = S.dt.low_mask;
  p.high_mask = S.dt.rot > 32 ? (uint32_t)((1ull << (S.dt.rot - 32)) - 1) : 0u;
  p.dinv = S.dt.dinv;
  p.dlim = S.dt.lim;
  p.seg_thresh = arena.ptr(list_mode ? o_cap : o_thr);  // unused in list mode
  p.out_key = reinterpret_cast<uint64_t*>(c->rec[0].ptr);
  p.seg_out_off = arena.ptr(o_off);
  p.seg_out_cap = arena.ptr(o_cap);
  p.seg_count = reinterpret_cast<unsigned long long*>(out->counters);
  p.seg_windows = reinterpret_cast<unsigned long long*>(out->counters + m + 1);
  if (list_mode) return SKS_OK;  // positions only, static tile ranges
  p.out_val = reinterpret_cast<uint64_t*>(c->rec[1].ptr);
  p.out_hi = reinterpret_cast<uint64_t*>(c->rec[2].ptr);
  static const bool static_tiles = getenv("SKS_SCAN_STATIC") != nullptr;
  p.tile_queue = static_tiles ? nullptr : reinterpret_cast<unsigned long long*>(arena.ptr(o_queue));
  return SKS_OK;
}

// ---- single-genome fast paths: what the two share, then each path's scratch, post launch and status ----
constexpr int kFastFallback = -1;      // not an SKS status: take the general build
constexpr int kFastPostFallback = -2;  // not an SKS status: the scan stands, take the general post_process

// The 1-sketch set a fast path fills from the device.  Its arrays go back to the
// block cache on scope exit (the device has not used them yet, or is idle after
// a synchronisation) unless the set is handed over to the caller.
class SingleSet {
 public:
  // oversized: the data array is larger than the sketch will be, so the set records its allocation
  int alloc(sks_ctx* c, uint64_t slots, bool oversized) {
    set_ = new (std::nothrow) sks_sketch_set();
    if (!set_) return sks::fail(SKS_E_NOMEM, "sks_sketch_build: out of memory");
    set_->device = c->device;
    set_->n = 1;
    SKS_TRY(alloc_u64(&set_->d_data, slots, &data_bytes_));
    if (oversized) set_->data_bytes = data_bytes_;
    SKS_TRY(alloc_u64(&set_->d_starts, 1));
    if (dev_alloc(reinterpret_cast<void**>(&set_->d_sizes), sizeof(uint32_t)) != hipSuccess)
      return sks::fail(SKS_E_HIP, "sks_sketch_build: device allocation failed");
    return SKS_OK;
  }
  ~SingleSet() {
    if (!set_) return;
    dev_release(set_->d_data, data_bytes_);
    dev_release(set_->d_starts, 8);
    dev_release(set_->d_sizes, 8);
    delete set_;
  }
  sks_sketch_set* operator->() const { return set_; }
  sks_sketch_set* hand_over() { return std::exchange(set_, nullptr); }

 private:
  sks_sketch_set* set_ = nullptr;
  size_t data_bytes_ = 0;
};

// Queues ev_s0, the scan, ev_s1, the path's post kernel and ev_end, then reads
// the first six words of the counters block into h (survivors, -, windows, -,
// and two result words), which synchronises the stream.
template <class Post>
int run_single(const BuildState& S, const ScanMeta& meta, int mode, Post post, uint64_t h[6]) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  hipError_t e = hipEventRecord(c->ev_s0, st);
  if (e == hipSuccess) e = sks::launch_scan(meta.p, mode, S.pol.flavour, false, c->device, st, c->grid_override);
  if (e == hipSuccess) e = hipEventRecord(c->ev_s1, st);
  if (e == hipSuccess) e = post();
  if (e == hipSuccess) e = hipEventRecord(c->ev_end, st);
  if (e == hipSuccess) e = sks::pinned_d2h(h, meta.counters, 6 * sizeof(uint64_t), st);
  if (e == hipSuccess) return SKS_OK;
  (void)hipStreamSynchronize(st);
  return sks::fail(SKS_E_HIP, std::string("sks_sketch_build: ") + hipGetErrorString(e));
}

void scan_timings(sks_ctx* c, uint64_t n_tiles, uint64_t survivors, sks_timings& tm) {
  (void)hipEventElapsedTime(&tm.scan_ms, c->ev_s0, c->ev_s1);  // tm comes in zeroed
  tm.scan_launches = n_tiles ? 1 : 0;
  tm.survivors = survivors;
}

// The build succeeded: the rest of the timings, the set's metadata, and the set to the caller.
void finish_single(const BuildState& S, sks_timings& tm, uint64_t windows, uint64_t size, SingleSet& one,
                   sks_sketch_set** out) {
  (void)hipEventElapsedTime(&tm.total_ms, S.c->ev_begin, S.c->ev_end);
  tm.windows = windows;
  tm.post_ms = tm.total_ms - tm.scan_ms;
  one->elem_words = 1;
  one->sizes = {(uint32_t)size};
  one->starts = {0};
  one->windows = {windows};
  one->window = S.w;
  one->mask[0] = S.mask_lo;
  one->mask[1] = S.mask_hi;
  one->policy = S.pol;
  S.c->last = tm;
  *out = one.hand_over();
}

// One narrow bottom-s genome (kmer_set_from_fasta_file's shape, kmer_set.cpp:
// 54-68) whose candidates fit k_bottom_fused: the scan and the fused
// post-processing write the sketch set's own arrays, and the build's only host
// round trip is one read-back of (survivors, windows, size) at the end — instead
// of a count read-back, compaction, a device-wide sort and unique with a
// distinct-count read-back, select and a metadata upload.  A genome whose scan
// overflows the candidate region or that has fewer than s distinct candidates
// (both rare) returns kFastFallback and the general build runs instead.
int build_bottom_single(BuildState& S, const uint8_t* d_seq, const uint64_t* seg_off, uint64_t thresh,
                        uint64_t cap, sks_timings& tm, sks_sketch_set** out) {
  sks_ctx* c = S.c;
  const uint64_t s = S.pol.param;
  SKS_HIP(c->rec[0].reserve(std::max<uint64_t>(cap, 1) * sizeof(uint64_t)));
  SKS_HIP(c->rec[1].reserve(std::max<uint64_t>(cap, 1) * sizeof(uint64_t)));
  const uint64_t slots = std::max<uint64_t>(std::min(s, cap), 1);
  ScanSegs seg;
  seg.push(seg_off[0], seg_off[1], thresh, cap);
  ScanMeta meta;
  // extra: whether a shortfall may retry (then a zero word), and the sketch's slots as a CSR pair
  SKS_TRY(scan_meta(S, d_seq, seg, false, {thresh != ~0ull ? 1ull : 0ull, 0, 0, slots}, 1, &meta));
  SingleSet one;
  SKS_TRY(one.alloc(c, slots, false));
  uint64_t h[6] = {0, 0, 0, 0, 0, 0};  // survivors, -, windows, -, size, -
  SKS_TRY(run_single(S, meta, sks::kModeBottom, [&] {
    return sks::launch_bottom_fused(reinterpret_cast<uint64_t*>(c->rec[0].ptr), meta.p.seg_out_off, meta.counters,
                                    meta.extra, meta.extra + 2, 1, cap, s, S.key_bits, S.runs, S.kconst,
                                    S.pol.flavour, one->d_data, meta.results, c->stream, meta.p.seg_out_cap,
                                    one->d_sizes, one->d_starts);
  }, h));
  const uint64_t survivors = h[0], windows = h[2], size = h[4];
  if (survivors > cap || size == ~0ull || size == sks::kBottomOverflow || size > slots) return kFastFallback;
  scan_timings(c, seg.n_tiles(), survivors, tm);
  finish_single(S, tm, windows, size, one, out);
  return SKS_OK;
}

// The bucket count (log2) the fused FracMinHash post-processing uses for a
// record region of `cap` keys, or -1 when it does not apply.  The mean bucket
// holds at most a quarter of a bucket's capacity: canonical k-mers (the smaller
// of two strands) are twice as dense at the low end of the key range as on
// average, which leaves a factor of two over the densest bucket.
int frac_plan_log_b(const sks_ctx* c, uint64_t cap) {
  const uint64_t per = sks::frac_bucket_capacity() / 4;
  const uint64_t need = (std::max<uint64_t>(cap, 1) + per - 1) / per;
  int lb = 0;
  while ((1ull << lb) < need) ++lb;
  if (lb > (int)sks::frac_max_log_buckets()) return -1;
  if (c->frac_buckets) {  // test control: fewer buckets
    int fb = 0;
    while ((1u << fb) < c->frac_buckets) ++fb;
    lb = std::min(lb, fb);
  }
  return lb;
}

// One narrow FracMinHash genome (the headline's shape): the scan, then a
// bucketed sort + unique on the device (post.hip launch_frac_fused) that reads
// the survivor count from device memory and writes the sketch set's own arrays;
// one metadata upload, and one read-back of (survivors, windows, size, status)
// at the end as the build's only host round trip — instead of a count
// read-back, compaction, a device-wide radix sort, flags + scan + counts with a
// second read-back, an allocation, a scatter and two uploads.  Returns
// kFastFallback when the scan overflowed its record region (the general build
// rescans with the counted capacity) and kFastPostFallback, with *survivors and
// *windows set, when a bucket or sub-bucket capacity was short (the records
// are intact: the general post_process runs on them without a second scan).
int build_frac_single(BuildState& S, const uint8_t* d_seq, const uint64_t* seg_off, uint64_t cap, int log_b,
                      sks_timings& tm, sks_sketch_set** out, uint64_t* survivors_out, uint64_t* windows_out) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  const uint32_t bucket_cap = c->frac_bucket_cap
                                  ? std::min<uint32_t>(c->frac_bucket_cap, sks::frac_bucket_capacity())
                                  : sks::frac_bucket_capacity();
  const uint64_t slots = std::max<uint64_t>(cap, 1);
  SKS_HIP(c->rec[0].reserve(slots * sizeof(uint64_t)));
  SKS_HIP(c->buf[0].reserve(((uint64_t)bucket_cap << log_b) * sizeof(uint64_t)));
  SKS_HIP(c->fstate.reserve(sks::frac_state_bytes()));
  if (!c->fstate_clean) SKS_HIP(hipMemsetAsync(c->fstate.ptr, 0, sks::frac_state_bytes(), st));
  c->fstate_clean = false;  // until the whole sequence below is queued
  ScanSegs seg;
  seg.push(seg_off[0], seg_off[1], ~0ull, cap);
  ScanMeta meta;
  SKS_TRY(scan_meta(S, d_seq, seg, false, {}, 2, &meta));
  SingleSet one;
  // the record region's capacity bounds the survivors, hence the sketch
  SKS_TRY(one.alloc(c, slots, true));
  uint64_t h[6] = {0, 0, 0, 0, 0, 0};  // survivors, -, windows, -, size, status
  const int rc = run_single(S, meta, sks::kModeFrac, [&] {
    const hipError_t e = sks::launch_frac_fused(
        reinterpret_cast<uint64_t*>(c->rec[0].ptr), meta.counters, meta.p.seg_out_cap, slots, S.key_bits, S.runs,
        (uint32_t)log_b, bucket_cap, col(c, 0), reinterpret_cast<uint32_t*>(c->fstate.ptr), one->d_data, one->d_sizes,
        one->d_starts, meta.results, st);
    if (e == hipSuccess) c->fstate_clean = true;
    return e;
  }, h);
  if (rc != SKS_OK) {
    c->fstate_clean = false;
    return rc;
  }
  const uint64_t survivors = h[0], windows = h[2], size = h[4], status = h[5];
  scan_timings(c, seg.n_tiles(), survivors, tm);
  *survivors_out = survivors;
  if (survivors > cap || size > survivors) return kFastFallback;  // the scan dropped records: rescan, counted capacity
  if (status != 0) {
    *windows_out = windows;
    return kFastPostFallback;
  }
  finish_single(S, tm, windows, size, one, out);
  c->last_path = SKS_BUILD_PATH_FUSED;
  return SKS_OK;
}

// Argument checks shared by sks_sketch_build and sks_kmer_list_build.
int validate_build(const char* fn, sks_ctx* c, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off,
                   uint32_t n_seg, int window, const uint64_t mask[2], const sks_policy* policy) {
  const std::string f(fn);
  if (!c || !mask || !policy || (!seg_off && n_seg)) return sks::fail(SKS_E_ARG, f + ": null argument");
  if (window < 1 || window > 64)
    return sks::fail(SKS_E_ARG, f + ": window must be in [1, 64] (MAX_KMER_LENGTH)");
  if (policy->kind != SKS_FRAC_MOD && policy->kind != SKS_BOTTOM_S)
    return sks::fail(SKS_E_ARG, f + ": unknown policy kind");
  if (policy->flavour != 0 && policy->flavour != 1)
    return sks::fail(SKS_E_ARG, f + ": unknown hash flavour");
  if (policy->param == 0) return sks::fail(SKS_E_ARG, f + ": policy param must be > 0");
  const int bits = 2 * window;
  const uint64_t lo_allowed = bits >= 64 ? ~0ull : ((1ull << bits) - 1);
  const uint64_t hi_allowed = bits <= 64 ? 0 : (bits >= 128 ? ~0ull : ((1ull << (bits - 64)) - 1));
  if ((mask[0] & ~lo_allowed) || (mask[1] & ~hi_allowed))
    return sks::fail(SKS_E_UNSUPPORTED, f + ": mask has bits at or above 2*window (the reference's "
                                            "generate_random_spaced_seed_mask never produces such masks)");
  if (n_bytes && !d_seq) return sks::fail(SKS_E_ARG, f + ": null sequence");
  for (uint32_t g = 0; g < n_seg; ++g)
    if (seg_off[g] > seg_off[g + 1] || seg_off[g + 1] > n_bytes)
      return sks::fail(SKS_E_ARG, f + ": segment offsets must be non-decreasing and <= n_bytes");
  return SKS_OK;
}

BuildState build_state(sks_ctx* c, int window, const uint64_t mask[2], const sks_policy& policy) {
  const bool wide = window > 32;
  BuildState S{c, window, wide, wide ? 2 : 1, mask[0], mask[1], policy,
               sks::fmh_const(mask[0], mask[1], window, policy.nonce, policy.flavour), {},
               wide ? sks::BitRuns{} : sks::bit_runs(mask[0]), wide ? 64 : std::max(1, __builtin_popcountll(mask[0]))};
  if (policy.kind == SKS_FRAC_MOD) S.dt = sks::make_div_test(policy.param);
  return S;
}

}  // namespace

extern "C" {

int sks_sketch_build(sks_ctx* c, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off, uint32_t n_seg,
                     int window, const uint64_t mask[2], const sks_policy* policy, sks_sketch_set** out) {
  if (!out) return sks::fail(SKS_E_ARG, "sks_sketch_build: null argument");
  *out = nullptr;
  SKS_TRY(validate_build("sks_sketch_build", c, d_seq, n_bytes, seg_off, n_seg, window, mask, policy));

  DeviceGuard guard(c->device);
  hipStream_t st = c->stream;
  BuildState S = build_state(c, window, mask, *policy);
  const bool bottom = policy->kind == SKS_BOTTOM_S;
  // bottom-s candidate margin: the first threshold keeps ~alpha*s windows, at
  // least 10 standard deviations above s for s >= 100 (a shortfall re-scans
  // that genome with a larger threshold).
  const double alpha = 1.0 + 10.0 / std::sqrt((double)policy->param) + 1.0 / (double)policy->param;

  sks_timings tm{};
  c->last_path = SKS_BUILD_PATH_GENERAL;
  SKS_HIP(hipEventRecord(c->ev_begin, st));

  std::vector<uint64_t> thresh_g(n_seg, ~0ull), cap_g(n_seg), windows_g(n_seg, 0);
  std::vector<uint64_t> final_size(n_seg, ~0ull);
  for (uint32_t g = 0; g < n_seg; ++g) {
    const uint64_t L = seg_off[g + 1] - seg_off[g];
    double expect;
    if (!bottom) {
      expect = (double)L / (double)policy->param;
    } else {
      double want = alpha * (double)policy->param;
      if ((double)L <= want) {
        thresh_g[g] = ~0ull;
        expect = (double)L;
      } else {
        long double t = (long double)want / (long double)L * 18446744073709551616.0L;
        thresh_g[g] = t >= 18446744073709551615.0L ? ~0ull : (uint64_t)t;
        expect = want;
      }
    }
    double cap = expect + 6.0 * std::sqrt(expect) + 4096.0;
    cap_g[g] = (uint64_t)std::min<double>(cap, (double)L + 1.0);
  }

  // one narrow bottom-s genome: the single-round-trip path when its candidate
  // region fits the fused post-processing (8 standard deviations of the
  // candidate count above its mean, not the general margin, so the kernel runs
  // at the smaller register tile)
  if (bottom && !S.wide && n_seg == 1 && getenv("SKS_NO_FAST_BOTTOM") == nullptr) {
    const uint64_t L = seg_off[1] - seg_off[0];
    const double expect = std::min<double>((double)L, alpha * (double)policy->param);
    const uint64_t cap = std::min<uint64_t>(cap_g[0], (uint64_t)(expect + 8.0 * std::sqrt(expect) + 256.0));
    if (L > 0 && cap <= sks::bottom_fused_capacity()) {
      const int rc = build_bottom_single(S, d_seq, seg_off, thresh_g[0], cap, tm, out);
      if (rc != kFastFallback) return rc;
      tm = sks_timings{};
    }
  }

  // one narrow FracMinHash genome: the single-round-trip path when the expected
  // survivors fit its buckets.  prescan: its scan's records stand (region 0 at
  // offset 0 with capacity cap_g[0], as the first pass below would lay it out)
  // and only the general post-processing is still to run
  bool prescan = false;
  uint64_t pre_survivors = 0, pre_windows = 0;
  if (!bottom && !S.wide && n_seg == 1 && c->frac_mode != SKS_FRAC_POST_GENERAL &&
      (c->frac_mode == SKS_FRAC_POST_FUSED || getenv("SKS_NO_FRAC_FUSED") == nullptr)) {
    const int log_b = frac_plan_log_b(c, cap_g[0]);
    if (log_b >= 0) {
      const int rc = build_frac_single(S, d_seq, seg_off, cap_g[0], log_b, tm, out, &pre_survivors, &pre_windows);
      if (rc == kFastPostFallback) {
        prescan = true;
        c->last_path = SKS_BUILD_PATH_FUSED_THEN_GENERAL_POST;
      } else if (rc != kFastFallback) {
        return rc;
      } else {
        cap_g[0] = std::max(cap_g[0], pre_survivors);  // the general build's first scan then fits
      }
    }
  }

  std::vector<PassOut> passes;
  std::vector<uint32_t> pending(n_seg);
  std::iota(pending.begin(), pending.end(), 0);
  int guard_passes = 0;
  while (!pending.empty()) {
    if (++guard_passes > 64) {
      free_passes(passes);
      return sks::fail(SKS_E_HIP, "sks_sketch_build: selection did not converge");
    }
    const uint32_t m = (uint32_t)pending.size();
    ScanSegs seg;
    for (uint32_t g : pending) seg.push(seg_off[g], seg_off[g + 1], thresh_g[g], cap_g[g]);
    std::vector<uint64_t> counts, wins;
    if (prescan) {
      // build_frac_single's scan: its time and launch are in tm already
      prescan = false;
      counts = {pre_survivors};
      wins = {pre_windows};
      tm.survivors = 0;  // added below
    } else {
      for (int r = 0; r < (bottom && S.wide ? 3 : (bottom || S.wide ? 2 : 1)); ++r)
        SKS_HIP(c->rec[r].reserve(std::max<uint64_t>(seg.total_cap, 1) * sizeof(uint64_t)));
      ScanMeta meta;
      SKS_TRY(scan_meta(S, d_seq, seg, false, {}, 0, &meta));

      SKS_HIP(hipEventRecord(c->ev_s0, st));
      SKS_HIP(sks::launch_scan(meta.p, bottom ? sks::kModeBottom : sks::kModeFrac, policy->flavour, S.wide, c->device,
                               st, c->grid_override));
      SKS_HIP(hipEventRecord(c->ev_s1, st));
      tm.scan_launches += seg.n_tiles() ? 1 : 0;
      // survivor and window counts: the counters block, in one read-back
      std::vector<uint64_t> cw(2 * (m + 1));
      SKS_HIP(sks::pinned_d2h(cw.data(), meta.counters, cw.size() * sizeof(uint64_t), st));
      counts.assign(cw.begin(), cw.begin() + m);
      wins.assign(cw.begin() + (m + 1), cw.begin() + (m + 1) + m);
      float ms = 0;
      SKS_HIP(hipEventElapsedTime(&ms, c->ev_s0, c->ev_s1));
      tm.scan_ms += ms;
    }

    std::vector<uint32_t> ok, next;
    for (uint32_t i = 0; i < m; ++i) {
      tm.survivors += counts[i];
      if (counts[i] > seg.cap[i]) {
        cap_g[pending[i]] = counts[i];
        next.push_back(pending[i]);
      } else {
        ok.push_back(i);
        windows_g[pending[i]] = wins[i];
      }
    }
    std::vector<uint32_t> retry_local;
    std::vector<uint64_t> fsz(m, ~0ull);
    int rc = post_process(S, pending, seg.off, counts, seg.thresh, ok, passes, retry_local, fsz);
    if (rc != SKS_OK) {
      free_passes(passes);
      return rc;
    }
    for (uint32_t i : ok)
      if (fsz[i] != ~0ull) final_size[pending[i]] = fsz[i];
    for (uint32_t i : retry_local) {
      uint32_t g = pending[i];
      uint64_t t = thresh_g[g];
      thresh_g[g] = t > (~0ull >> 3) ? ~0ull : t * 8;
      uint64_t L = seg_off[g + 1] - seg_off[g];
      cap_g[g] = std::min<uint64_t>(L + 1, std::max<uint64_t>(cap_g[g], counts[i]) * 8 + 4096);
      next.push_back(g);
    }
    std::sort(next.begin(), next.end());
    pending.swap(next);
  }

  // assemble the final set in segment order
  sks_sketch_set* set = new (std::nothrow) sks_sketch_set();
  if (!set) {
    free_passes(passes);
    return sks::fail(SKS_E_NOMEM, "sks_sketch_build: out of memory");
  }
  set->device = c->device;
  set->elem_words = S.ew;
  set->n = n_seg;
  set->sizes.resize(n_seg);
  set->starts.resize(n_seg);
  set->windows = windows_g;
  set->window = window;
  set->mask[0] = mask[0];
  set->mask[1] = mask[1];
  set->policy = *policy;
  uint64_t total = 0;
  for (uint32_t g = 0; g < n_seg; ++g) {
    set->starts[g] = total;
    set->sizes[g] = (uint32_t)final_size[g];
    total += final_size[g];
  }
  int rc = SKS_OK;
  const bool single_in_order =
      passes.size() == 1 && passes[0].segs.size() == n_seg &&
      std::is_sorted(passes[0].segs.begin(), passes[0].segs.end());
  if (single_in_order) {
    set->d_data = passes[0].d;
    passes[0].d = nullptr;
  } else {
    rc = alloc_u64(&set->d_data, total * S.ew);
    for (size_t pi = 0; rc == SKS_OK && pi < passes.size(); ++pi) {
      const PassOut& po = passes[pi];
      // each sketch of the pass to its place in segment order
      for (size_t i = 0; i < po.segs.size() && rc == SKS_OK; ++i) {
        const uint64_t len = (po.off[i + 1] - po.off[i]) * S.ew;
        if (!len) continue;
        if (hipMemcpyAsync(set->d_data + set->starts[po.segs[i]] * S.ew, po.d + po.off[i] * S.ew,
                           len * sizeof(uint64_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
          rc = sks::fail(SKS_E_HIP, "sks_sketch_build: assembling copy failed");
      }
    }
  }
  if (rc == SKS_OK) rc = alloc_u64(&set->d_starts, n_seg);
  if (rc == SKS_OK && dev_alloc(reinterpret_cast<void**>(&set->d_sizes),
                                std::max<uint32_t>(n_seg, 1) * sizeof(uint32_t)) != hipSuccess)
    rc = sks::fail(SKS_E_HIP, "sks_sketch_build: device allocation failed");
  if (rc == SKS_OK && n_seg) {
    if (sks::pinned_h2d(set->d_starts, set->starts.data(), n_seg * sizeof(uint64_t), st) !=
            hipSuccess ||
        sks::pinned_h2d(set->d_sizes, set->sizes.data(), n_seg * sizeof(uint32_t), st) != hipSuccess)
      rc = sks::fail(SKS_E_HIP, "sks_sketch_build: metadata upload failed");
  }
  if (rc == SKS_OK && hipEventRecord(c->ev_end, st) != hipSuccess)
    rc = sks::fail(SKS_E_HIP, "hipEventRecord failed");
  if (rc == SKS_OK && hipStreamSynchronize(st) != hipSuccess)
    rc = sks::fail(SKS_E_HIP, "hipStreamSynchronize failed");
  free_passes(passes);
  if (rc != SKS_OK) {
    sks_sketch_set_free(set);
    return rc;
  }
  float tot = 0;
  (void)hipEventElapsedTime(&tot, c->ev_begin, c->ev_end);
  tm.total_ms = tot;
  tm.post_ms = tot - tm.scan_ms;
  for (uint64_t wv : windows_g) tm.windows += wv;
  c->last = tm;
  *out = set;
  return SKS_OK;
}

int sks_sketch_set_free(sks_sketch_set* set) {
  if (!set) return SKS_OK;
  DeviceGuard g(set->device);
  // hipFree's contract: work queued on the arrays (any stream) completes before
  // they are reused; then they go to the block cache instead of being unmapped
  if (set->d_data || set->d_starts || set->d_sizes) (void)hipDeviceSynchronize();
  release_set_arrays(set, nullptr, false);
  delete set;
  return SKS_OK;
}

int sks_sketch_set_free_on_stream(sks_sketch_set* set, void* stream) {
  if (!set) return SKS_OK;
  DeviceGuard g(set->device);
  release_set_arrays(set, reinterpret_cast<hipStream_t>(stream), true);
  delete set;
  return SKS_OK;
}

uint32_t sks_sketch_set_num(const sks_sketch_set* set) { return set ? set->n : 0; }

int sks_sketch_set_elem_words(const sks_sketch_set* set) { return set ? set->elem_words : 0; }

int sks_sketch_set_sizes(const sks_sketch_set* set, uint32_t* sizes) {
  if (!set || !sizes) return sks::fail(SKS_E_ARG, "sks_sketch_set_sizes: null argument");
  std::copy(set->sizes.begin(), set->sizes.end(), sizes);
  return SKS_OK;
}

int sks_sketch_set_windows(const sks_sketch_set* set, uint64_t* windows) {
  if (!set || !windows) return sks::fail(SKS_E_ARG, "sks_sketch_set_windows: null argument");
  std::copy(set->windows.begin(), set->windows.end(), windows);
  return SKS_OK;
}

int sks_sketch_set_starts(const sks_sketch_set* set, uint64_t* starts) {
  if (!set || !starts) return sks::fail(SKS_E_ARG, "sks_sketch_set_starts: null argument");
  std::copy(set->starts.begin(), set->starts.end(), starts);
  return SKS_OK;
}

const uint64_t* sks_sketch_set_device_data(const sks_sketch_set* set) { return set ? set->d_data : nullptr; }
const uint64_t* sks_sketch_set_device_starts(const sks_sketch_set* set) { return set ? set->d_starts : nullptr; }
const uint32_t* sks_sketch_set_device_sizes(const sks_sketch_set* set) { return set ? set->d_sizes : nullptr; }

int sks_sketch_set_copy(const sks_sketch_set* set, uint32_t i, uint64_t* out) {
  if (!set) return sks::fail(SKS_E_ARG, "sks_sketch_set_copy: null set");
  if (i >= set->n) return sks::fail(SKS_E_ARG, "sks_sketch_set_copy: index out of range");
  if (!out && set->sizes[i]) return sks::fail(SKS_E_ARG, "sks_sketch_set_copy: null output");
  DeviceGuard g(set->device);
  uint64_t words = (uint64_t)set->sizes[i] * set->elem_words;
  if (words)
    SKS_HIP(hipMemcpy(out, set->d_data + set->starts[i] * set->elem_words, words * sizeof(uint64_t),
                      hipMemcpyDeviceToHost));
  return SKS_OK;
}

int sks_sketch_set_export(const sks_sketch_set* set, uint64_t* d_dst, uint64_t stride, uint32_t* d_sizes) {
  if (!set || !d_dst || !d_sizes) return sks::fail(SKS_E_ARG, "sks_sketch_set_export: null argument");
  for (uint32_t s : set->sizes)
    if (s > stride) return sks::fail(SKS_E_ARG, "sks_sketch_set_export: stride smaller than a sketch");
  DeviceGuard g(set->device);
  SKS_HIP(sks::launch_export(set->d_data, set->d_starts, set->d_sizes, set->n, set->elem_words,
                             d_dst, stride, d_sizes, nullptr));
  SKS_HIP(hipStreamSynchronize(nullptr));
  return SKS_OK;
}

int sks_sketch_set_export_csr(const sks_sketch_set* set, uint64_t* d_data, uint32_t* d_sizes) {
  if (!set) return sks::fail(SKS_E_ARG, "sks_sketch_set_export_csr: null set");
  DeviceGuard g(set->device);
  uint64_t total = 0;
  for (uint32_t v : set->sizes) total += v;
  if ((total && !d_data) || (set->n && !d_sizes))
    return sks::fail(SKS_E_ARG, "sks_sketch_set_export_csr: null argument");
  // the set's arrays are CSR in sketch order: one copy each
  if (total)
    SKS_HIP(hipMemcpy(d_data, set->d_data + set->starts[0] * set->elem_words,
                      total * set->elem_words * sizeof(uint64_t), hipMemcpyDeviceToDevice));
  if (set->n) SKS_HIP(hipMemcpy(d_sizes, set->d_sizes, set->n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
  return SKS_OK;
}

// ---- ordered k-mer lists (nucleotide_string_list_to_kmers) -----------------------------------

int sks_kmer_list_build(sks_ctx* c, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off, uint32_t n_seg,
                        int window, const uint64_t mask[2], const sks_policy* policy, sks_kmer_list** out) {
  if (!out) return sks::fail(SKS_E_ARG, "sks_kmer_list_build: null argument");
  *out = nullptr;
  SKS_TRY(validate_build("sks_kmer_list_build", c, d_seq, n_bytes, seg_off, n_seg, window, mask, policy));
  if (policy->kind != SKS_FRAC_MOD)
    return sks::fail(SKS_E_UNSUPPORTED,
                     "sks_kmer_list_build: lists take a per-k-mer predicate (SKS_FRAC_MOD); "
                     "bottom-s is a set selection");
  DeviceGuard guard(c->device);
  hipStream_t st = c->stream;
  const BuildState S = build_state(c, window, mask, *policy);
  std::vector<uint64_t> cap(n_seg), counts(n_seg, 0);
  for (uint32_t g = 0; g < n_seg; ++g) {
    const double len = (double)(seg_off[g + 1] - seg_off[g]), expect = len / (double)policy->param;
    cap[g] = (uint64_t)std::min<double>(expect + 6.0 * std::sqrt(expect) + 4096.0, len + 1.0);
  }
  ScanSegs seg;
  for (int pass = 0; pass < 2; ++pass) {  // pass 2 only if a capacity estimate overflowed
    seg = ScanSegs{};
    for (uint32_t g = 0; g < n_seg; ++g) seg.push(seg_off[g], seg_off[g + 1], ~0ull, cap[g]);
    SKS_HIP(c->rec[0].reserve(std::max<uint64_t>(seg.total_cap, 1) * sizeof(uint64_t)));
    ScanMeta meta;
    SKS_TRY(scan_meta(S, d_seq, seg, true, {}, 0, &meta));
    SKS_HIP(sks::launch_scan(meta.p, sks::kModeList, policy->flavour, S.wide, c->device, st, c->grid_override));
    SKS_HIP(sks::pinned_d2h(counts.data(), meta.counters, n_seg * sizeof(uint64_t), st));
    bool overflow = false;
    for (uint32_t g = 0; g < n_seg; ++g)
      if (counts[g] > cap[g]) {
        overflow = true;
        cap[g] = counts[g];
      }
    if (!overflow) break;
    if (pass == 1) return sks::fail(SKS_E_HIP, "sks_kmer_list_build: survivor count changed between passes");
  }
  // dense positions (segments in stream order), then one sort: stream order
  std::vector<uint64_t> csr = prefix(counts);
  const uint64_t T = csr[n_seg];
  uint64_t max_len = 0;
  for (uint64_t v : counts) max_len = std::max(max_len, v);
  sks_kmer_list* kl = new (std::nothrow) sks_kmer_list();
  if (!kl) return sks::fail(SKS_E_NOMEM, "sks_kmer_list_build: out of memory");
  kl->device = c->device;
  kl->n = n_seg;
  kl->total = T;
  kl->counts = counts;
  int rc = alloc_u64(&kl->d_pos, T);
  if (rc == SKS_OK) rc = alloc_u64(&kl->d_bits, 4 * T);
  if (rc == SKS_OK) rc = reserve_cols(c, {0}, T + 1);
  MetaArena arena(c);
  size_t o_src = arena.add(seg.off), o_csr = arena.add(csr), o_beg = arena.add(seg.beg);
  if (rc == SKS_OK) rc = arena.upload();
  hipError_t e = hipSuccess;
  if (rc == SKS_OK && T) {
    e = sks::compact_regions(reinterpret_cast<uint64_t*>(c->rec[0].ptr), col(c, 0), arena.ptr(o_src),
                             arena.ptr(o_csr), n_seg, max_len, st);
    if (e == hipSuccess)
      e = sks::seg_sort_keys(col(c, 0), kl->d_pos, T, {0, T}, nullptr, end_bit_of(n_bytes), c->tmp, st);
    if (e == hipSuccess)
      e = sks::launch_materialise(d_seq, arena.ptr(o_beg), n_seg, kl->d_pos, T, window, mask[0],
                                  mask[1], kl->d_bits, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = sks::fail(SKS_E_HIP, std::string("sks_kmer_list_build: ") + hipGetErrorString(e));
  }
  if (rc != SKS_OK) {
    sks_kmer_list_free(kl);
    return rc;
  }
  *out = kl;
  return SKS_OK;
}

int sks_kmer_list_free(sks_kmer_list* kl) {
  if (!kl) return SKS_OK;
  DeviceGuard g(kl->device);
  if (kl->d_pos) (void)hipFree(kl->d_pos);
  if (kl->d_bits) (void)hipFree(kl->d_bits);
  delete kl;
  return SKS_OK;
}

uint64_t sks_kmer_list_total(const sks_kmer_list* kl) { return kl ? kl->total : 0; }

int sks_kmer_list_counts(const sks_kmer_list* kl, uint64_t* counts) {
  if (!kl || (!counts && kl->n)) return sks::fail(SKS_E_ARG, "sks_kmer_list_counts: null argument");
  std::copy(kl->counts.begin(), kl->counts.end(), counts);
  return SKS_OK;
}

const uint64_t* sks_kmer_list_device_positions(const sks_kmer_list* kl) { return kl ? kl->d_pos : nullptr; }
const uint64_t* sks_kmer_list_device_bits(const sks_kmer_list* kl) { return kl ? kl->d_bits : nullptr; }

int sks_kmer_list_copy(const sks_kmer_list* kl, uint64_t* positions, uint64_t* bits) {
  if (!kl) return sks::fail(SKS_E_ARG, "sks_kmer_list_copy: null list");
  DeviceGuard g(kl->device);
  if (positions && kl->total)
    SKS_HIP(hipMemcpy(positions, kl->d_pos, kl->total * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (bits && kl->total)
    SKS_HIP(hipMemcpy(bits, kl->d_bits, kl->total * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SKS_OK;
}

}  // extern "C"
