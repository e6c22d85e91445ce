// C-ABI implementation (include/sks.h): sks_sketch_build — the scan's
// metadata, the two single-genome fast paths, and the general pass loop (its
// post-processing is build_post.cpp, its arithmetic build_plan.hpp).
#include <cstdlib>
#include <numeric>
#include <utility>

#include "build_internal.hpp"

using namespace sks;

BuildKnobs sks::read_build_knobs() {
  static const bool scan_static = getenv("SKS_SCAN_STATIC") != nullptr;
  BuildKnobs k;
  k.no_fused_bottom = getenv("SKS_NO_FUSED_BOTTOM") != nullptr;
  k.no_fast_bottom = getenv("SKS_NO_FAST_BOTTOM") != nullptr;
  k.no_frac_fused = getenv("SKS_NO_FRAC_FUSED") != nullptr;
  k.scan_static = scan_static;
  return k;
}

int sks::validate_build(const char* fn, sks_ctx* c, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off,
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

int sks::scan_meta(const BuildState& S, const uint8_t* d_seq, const ScanSegs& g, bool list_mode,
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
  p.tile_queue = S.knobs.scan_static ? nullptr : reinterpret_cast<unsigned long long*>(arena.ptr(o_queue));
  return SKS_OK;
}

namespace {

// ---- single-genome fast paths: what the two share, then each path's scratch, post launch and status ----
constexpr int kFastFallback = -1;      // not an SKS status: take the general build
constexpr int kFastPostFallback = -2;  // not an SKS status: the scan stands, take the general post_process

// The 1-sketch set a fast path's kernels fill (data, start and size) on the
// context's stream.  Dropped on a fallback or an error, its blocks go back to
// the cache by themselves.
int make_single_set(const BuildState& S, uint64_t slots, SetPtr* one) {
  const uint64_t mask[2] = {S.mask_lo, S.mask_hi};
  return make_sketch_set(S.c->device, 1, S.w, mask, S.pol, {0}, {0}, {}, &slots, S.c->stream, MetaUpload::kNone, one);
}

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

// The build succeeded: the rest of the timings, the set's host sizes, and the set to the caller.
void finish_single(const BuildState& S, sks_timings& tm, uint64_t windows, uint64_t size, SetPtr& one,
                   sks_sketch_set** out) {
  (void)hipEventElapsedTime(&tm.total_ms, S.c->ev_begin, S.c->ev_end);
  tm.windows = windows;
  tm.post_ms = tm.total_ms - tm.scan_ms;
  one->sizes = {(uint32_t)size};
  one->windows = {windows};
  S.c->last = tm;
  *out = one.release();
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
  SetPtr one;
  SKS_TRY(make_single_set(S, slots, &one));
  uint64_t h[6] = {0, 0, 0, 0, 0, 0};  // survivors, -, windows, -, size, -
  SKS_TRY(run_single(S, meta, sks::kModeBottom, [&] {
    return sks::launch_bottom_fused(reinterpret_cast<uint64_t*>(c->rec[0].ptr), meta.p.seg_out_off, meta.counters,
                                    meta.extra, meta.extra + 2, 1, cap, s, S.key_bits, S.runs, S.kconst,
                                    S.pol.flavour, one->d_data(), meta.results, c->stream, meta.p.seg_out_cap,
                                    one->d_sizes(), one->d_starts());
  }, h));
  const uint64_t survivors = h[0], windows = h[2], size = h[4];
  if (survivors > cap || size == ~0ull || size == sks::kBottomOverflow || size > slots) return kFastFallback;
  scan_timings(c, seg.n_tiles(), survivors, tm);
  finish_single(S, tm, windows, size, one, out);
  return SKS_OK;
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
  SetPtr one;
  // the record region's capacity bounds the survivors, hence the sketch
  SKS_TRY(make_single_set(S, slots, &one));
  uint64_t h[6] = {0, 0, 0, 0, 0, 0};  // survivors, -, windows, -, size, status
  const int rc = run_single(S, meta, sks::kModeFrac, [&] {
    const hipError_t e = sks::launch_frac_fused(
        reinterpret_cast<uint64_t*>(c->rec[0].ptr), meta.counters, meta.p.seg_out_cap, slots, S.key_bits, S.runs,
        (uint32_t)log_b, bucket_cap, col(c, 0), reinterpret_cast<uint32_t*>(c->fstate.ptr), one->d_data(),
        one->d_sizes(), one->d_starts(), meta.results, st);
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

// The general build's state across its passes (per global segment).
struct Passes {
  std::vector<SegPlan> plan;         // threshold and record capacity of the segment's next scan
  std::vector<uint64_t> windows;     // k-mer windows hashed
  std::vector<uint64_t> final_size;  // ~0 until the segment's sketch is made
  std::vector<PassOut> out;
  // the fused FracMinHash path's scan stands in for the first pass's (region 0
  // at offset 0 with capacity plan[0].cap, as the first pass would lay it out)
  bool prescan = false;
  uint64_t pre_survivors = 0, pre_windows = 0;
};

// Scans the pending segments into their record regions and reads back each
// one's survivor and window counts (the counters block, in one read-back).
int scan_pass(BuildState& S, const uint8_t* d_seq, const ScanSegs& seg, sks_timings& tm, std::vector<uint64_t>& counts,
              std::vector<uint64_t>& wins) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  const bool bottom = S.pol.kind == SKS_BOTTOM_S;
  const uint32_t m = seg.m();
  for (int r = 0; r < (bottom && S.wide ? 3 : (bottom || S.wide ? 2 : 1)); ++r)
    SKS_HIP(c->rec[r].reserve(std::max<uint64_t>(seg.total_cap, 1) * sizeof(uint64_t)));
  ScanMeta meta;
  SKS_TRY(scan_meta(S, d_seq, seg, false, {}, 0, &meta));
  SKS_HIP(hipEventRecord(c->ev_s0, st));
  SKS_HIP(sks::launch_scan(meta.p, bottom ? sks::kModeBottom : sks::kModeFrac, S.pol.flavour, S.wide, c->device, st,
                           c->grid_override));
  SKS_HIP(hipEventRecord(c->ev_s1, st));
  tm.scan_launches += seg.n_tiles() ? 1 : 0;
  std::vector<uint64_t> cw(2 * (m + 1));
  SKS_HIP(sks::pinned_d2h(cw.data(), meta.counters, cw.size() * sizeof(uint64_t), st));
  counts.assign(cw.begin(), cw.begin() + m);
  wins.assign(cw.begin() + (m + 1), cw.begin() + (m + 1) + m);
  float ms = 0;
  SKS_HIP(hipEventElapsedTime(&ms, c->ev_s0, c->ev_s1));
  tm.scan_ms += ms;
  return SKS_OK;
}

// Scan, post-process, and go round again with the segments whose record region
// overflowed (counted capacity) or whose bottom-s threshold was too low.
int run_passes(BuildState& S, const uint8_t* d_seq, const uint64_t* seg_off, uint32_t n_seg, Passes& P,
               sks_timings& tm) {
  std::vector<uint32_t> pending(n_seg);
  std::iota(pending.begin(), pending.end(), 0);
  int guard_passes = 0;
  while (!pending.empty()) {
    if (++guard_passes > 64) return sks::fail(SKS_E_HIP, "sks_sketch_build: selection did not converge");
    const uint32_t m = (uint32_t)pending.size();
    ScanSegs seg;
    for (uint32_t g : pending) seg.push(seg_off[g], seg_off[g + 1], P.plan[g].thresh, P.plan[g].cap);
    std::vector<uint64_t> counts, wins;
    if (P.prescan) {
      // build_frac_single's scan: its time and launch are in tm already
      P.prescan = false;
      counts = {P.pre_survivors};
      wins = {P.pre_windows};
      tm.survivors = 0;  // added below
    } else {
      SKS_TRY(scan_pass(S, d_seq, seg, tm, counts, wins));
    }
    std::vector<uint32_t> ok, next;
    for (uint32_t i = 0; i < m; ++i) {
      tm.survivors += counts[i];
      if (counts[i] > seg.cap[i]) {
        P.plan[pending[i]].cap = counts[i];
        next.push_back(pending[i]);
      } else {
        ok.push_back(i);
        P.windows[pending[i]] = wins[i];
      }
    }
    std::vector<uint32_t> retry_local;
    std::vector<uint64_t> fsz(m, ~0ull);
    SKS_TRY(post_process(S, pending, seg.off, counts, seg.thresh, ok, P.out, retry_local, fsz));
    for (uint32_t i : ok)
      if (fsz[i] != ~0ull) P.final_size[pending[i]] = fsz[i];
    for (uint32_t i : retry_local) {
      const uint32_t g = pending[i];
      P.plan[g] = sks::escalate(P.plan[g], counts[i], seg_off[g + 1] - seg_off[g]);
      next.push_back(g);
    }
    std::sort(next.begin(), next.end());
    pending.swap(next);
  }
  return SKS_OK;
}

// The final set in segment order: the one pass's block itself when it holds
// every sketch in order, else each sketch copied to its place.  Waits for the
// stream (the build's end), after which the pass blocks go back without events.
int assemble_set(BuildState& S, uint32_t n_seg, Passes& P, SetPtr* out) {
  sks_ctx* c = S.c;
  hipStream_t st = c->stream;
  std::vector<uint32_t> sizes(n_seg);
  uint64_t total = 0;
  for (uint32_t g = 0; g < n_seg; ++g) {
    sizes[g] = (uint32_t)P.final_size[g];
    total += P.final_size[g];
  }
  const bool single_in_order = P.out.size() == 1 && P.out[0].segs.size() == n_seg &&
                               std::is_sorted(P.out[0].segs.begin(), P.out[0].segs.end());
  const uint64_t mask[2] = {S.mask_lo, S.mask_hi}, words = total * S.ew;
  SetPtr set;
  DevBlock abund;  // a counted build: placed as the elements are
  if (S.counted && !single_in_order) SKS_HIP(abund.alloc(std::max<uint64_t>(total, 1) * sizeof(uint32_t), st));
  SKS_TRY(make_sketch_set(c->device, S.ew, S.w, mask, S.pol, std::move(sizes), P.windows, {},
                          single_in_order ? nullptr : &words, st, MetaUpload::kStream, &set,
                          S.counted ? (single_in_order ? &P.out[0].abund : &abund) : nullptr));
  if (single_in_order) set->data = std::move(P.out[0].d);
  for (const PassOut& po : P.out) {
    if (single_in_order) break;
    // each sketch of the pass to its place in segment order
    for (size_t i = 0; i < po.segs.size(); ++i) {
      const uint64_t len = (po.off[i + 1] - po.off[i]) * S.ew;
      if (len)
        SKS_HIP(hipMemcpyAsync(set->d_data() + set->starts[po.segs[i]] * S.ew, po.d.as<uint64_t>() + po.off[i] * S.ew,
                               len * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
      if (len && S.counted)
        SKS_HIP(hipMemcpyAsync(set->d_abund() + set->starts[po.segs[i]], po.abund.as<uint32_t>() + po.off[i],
                               (po.off[i + 1] - po.off[i]) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    }
  }
  SKS_HIP(hipEventRecord(c->ev_end, st));
  SKS_HIP(hipStreamSynchronize(st));
  for (PassOut& po : P.out) {
    po.d.release();
    po.abund.release();
  }
  *out = std::move(set);
  return SKS_OK;
}

}  // namespace

extern "C" int sks_sketch_build(sks_ctx* c, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off,
                                uint32_t n_seg, int window, const uint64_t mask[2], const sks_policy* policy,
                                sks_sketch_set** out) {
  if (!out) return sks::fail(SKS_E_ARG, "sks_sketch_build: null argument");
  *out = nullptr;
  SKS_TRY(validate_build("sks_sketch_build", c, d_seq, n_bytes, seg_off, n_seg, window, mask, policy));

  DeviceGuard guard(c->device);
  BuildState S = build_state(c, window, mask, *policy);
  const bool bottom = policy->kind == SKS_BOTTOM_S;
  sks_timings tm{};
  c->last_path = SKS_BUILD_PATH_GENERAL;
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));

  Passes P;
  P.windows.assign(n_seg, 0);
  P.final_size.assign(n_seg, ~0ull);
  for (uint32_t g = 0; g < n_seg; ++g)
    P.plan.push_back(sks::plan_segment(bottom, policy->param, seg_off[g + 1] - seg_off[g]));

  // one narrow bottom-s genome: the single-round-trip path when its candidate
  // region fits the fused post-processing
  if (bottom && !S.wide && n_seg == 1 && !S.knobs.no_fast_bottom) {
    const uint64_t L = seg_off[1] - seg_off[0];
    const uint64_t cap = sks::bottom_single_capacity(policy->param, L, P.plan[0].cap);
    if (L > 0 && cap <= sks::bottom_fused_capacity()) {
      const int rc = build_bottom_single(S, d_seq, seg_off, P.plan[0].thresh, cap, tm, out);
      if (rc != kFastFallback) return rc;
      tm = sks_timings{};
    }
  }

  // one narrow FracMinHash genome: the single-round-trip path when the expected
  // survivors fit its buckets.  On kFastPostFallback its scan's records stand
  // and only the general post-processing is still to run
  if (!bottom && !S.wide && n_seg == 1 && c->frac_mode != SKS_FRAC_POST_GENERAL &&
      (c->frac_mode == SKS_FRAC_POST_FUSED || !S.knobs.no_frac_fused)) {
    const int log_b = sks::frac_plan_log_b(P.plan[0].cap, sks::frac_bucket_capacity(), sks::frac_max_log_buckets(),
                                           c->frac_buckets);
    if (log_b >= 0) {
      const int rc =
          build_frac_single(S, d_seq, seg_off, P.plan[0].cap, log_b, tm, out, &P.pre_survivors, &P.pre_windows);
      if (rc == kFastPostFallback) {
        P.prescan = true;
        c->last_path = SKS_BUILD_PATH_FUSED_THEN_GENERAL_POST;
      } else if (rc != kFastFallback) {
        return rc;
      } else {
        P.plan[0].cap = std::max(P.plan[0].cap, P.pre_survivors);  // the general build's first scan then fits
      }
    }
  }

  SKS_TRY(run_passes(S, d_seq, seg_off, n_seg, P, tm));
  SetPtr set;
  SKS_TRY(assemble_set(S, n_seg, P, &set));
  float tot = 0;
  (void)hipEventElapsedTime(&tot, c->ev_begin, c->ev_end);
  tm.total_ms = tot;
  tm.post_ms = tot - tm.scan_ms;
  for (uint64_t wv : P.windows) tm.windows += wv;
  c->last = tm;
  *out = set.release();
  return SKS_OK;
}

extern "C" int sks_sketch_build_counted(sks_ctx* c, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off,
                                        uint32_t n_seg, int window, const uint64_t mask[2], const sks_policy* policy,
                                        uint32_t min_abund, uint32_t max_abund, sks_sketch_set** out) {
  if (!out) return sks::fail(SKS_E_ARG, "sks_sketch_build_counted: null argument");
  *out = nullptr;
  SKS_TRY(validate_build("sks_sketch_build_counted", c, d_seq, n_bytes, seg_off, n_seg, window, mask, policy));
  if (policy->kind != SKS_FRAC_MOD)
    return sks::fail(SKS_E_UNSUPPORTED,
                     "sks_sketch_build_counted: policy kind: FracMinHash only (a bottom-s sketch's windows are "
                     "pre-filtered by a threshold, so its records do not count every occurrence)");

  DeviceGuard guard(c->device);
  BuildState S = build_state(c, window, mask, *policy);
  S.counted = true;
  S.min_abund = min_abund;
  S.max_abund = max_abund;
  sks_timings tm{};
  c->last_path = SKS_BUILD_PATH_GENERAL;
  SKS_HIP(hipEventRecord(c->ev_begin, c->stream));

  // always the general pass loop: the fused single-genome path drops the duplicates it meets
  Passes P;
  P.windows.assign(n_seg, 0);
  P.final_size.assign(n_seg, ~0ull);
  for (uint32_t g = 0; g < n_seg; ++g)
    P.plan.push_back(sks::plan_segment(false, policy->param, seg_off[g + 1] - seg_off[g]));
  SKS_TRY(run_passes(S, d_seq, seg_off, n_seg, P, tm));
  SetPtr set;
  SKS_TRY(assemble_set(S, n_seg, P, &set));
  float tot = 0;
  (void)hipEventElapsedTime(&tot, c->ev_begin, c->ev_end);
  tm.total_ms = tot;
  tm.post_ms = tot - tm.scan_ms;
  for (uint64_t wv : P.windows) tm.windows += wv;
  c->last = tm;
  *out = set.release();
  return SKS_OK;
}
