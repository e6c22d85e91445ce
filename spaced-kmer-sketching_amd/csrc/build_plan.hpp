// The arithmetic that plans a sketch build (host only: no HIP, so
// tests/cpp/plan_test.cpp checks it on any machine): per-segment thresholds
// and record capacities, the retry escalation, the fused FracMinHash bucket
// count, and which post-processing pipeline a pass takes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace sks {

// ---- thresholds and capacities ---------------------------------------------------------
// bottom-s candidate margin: the first threshold keeps ~alpha*s windows, at
// least 10 standard deviations above s for s >= 100 (a shortfall re-scans that
// genome with a larger threshold).
inline double bottom_alpha(uint64_t s) { return 1.0 + 10.0 / std::sqrt((double)s) + 1.0 / (double)s; }

struct SegPlan {
  uint64_t thresh;  // bottom-s pre-filter on the window hash (~0: none)
  uint64_t cap;     // record slots for the segment's survivors
};

// A segment of L bases under FracMinHash 1/param or bottom-param: the expected
// survivors plus six standard deviations and 4096, never more than L + 1.
// (k-mer lists plan as FracMinHash.)
inline SegPlan plan_segment(bool bottom, uint64_t param, uint64_t L) {
  SegPlan p{~0ull, 0};
  double expect;
  if (!bottom) {
    expect = (double)L / (double)param;
  } else {
    double want = bottom_alpha(param) * (double)param;
    if ((double)L <= want) {
      expect = (double)L;
    } else {
      long double t = (long double)want / (long double)L * 18446744073709551616.0L;
      p.thresh = t >= 18446744073709551615.0L ? ~0ull : (uint64_t)t;
      expect = want;
    }
  }
  double cap = expect + 6.0 * std::sqrt(expect) + 4096.0;
  p.cap = (uint64_t)std::min<double>(cap, (double)L + 1.0);
  return p;
}

// One narrow bottom-s genome on the single-round-trip path: 8 standard
// deviations of the candidate count above its mean, not the general margin, so
// the fused kernel runs at the smaller register tile.
inline uint64_t bottom_single_capacity(uint64_t s, uint64_t L, uint64_t general_cap) {
  const double expect = std::min<double>((double)L, bottom_alpha(s) * (double)s);
  return std::min<uint64_t>(general_cap, (uint64_t)(expect + 8.0 * std::sqrt(expect) + 256.0));
}

// A bottom-s genome with too few distinct candidates under its threshold goes
// round again with eight times the threshold (saturating) and capacity.
inline SegPlan escalate(SegPlan p, uint64_t count, uint64_t L) {
  p.thresh = p.thresh > (~0ull >> 3) ? ~0ull : p.thresh * 8;
  p.cap = std::min<uint64_t>(L + 1, std::max<uint64_t>(p.cap, count) * 8 + 4096);
  return p;
}

// The bucket count (log2) the fused FracMinHash post-processing uses for a
// record region of `cap` keys, or -1 when it does not apply.  The mean bucket
// holds at most a quarter of a bucket's capacity: canonical k-mers (the smaller
// of two strands) are twice as dense at the low end of the key range as on
// average, which leaves a factor of two over the densest bucket.
// forced_buckets (test control, 0: none): no more buckets than that.
inline int frac_plan_log_b(uint64_t cap, uint32_t bucket_capacity, uint32_t max_log_b, uint32_t forced_buckets) {
  const uint64_t per = bucket_capacity / 4;
  const uint64_t need = (std::max<uint64_t>(cap, 1) + per - 1) / per;
  int lb = 0;
  while ((1ull << lb) < need) ++lb;
  if (lb > (int)max_log_b) return -1;
  if (forced_buckets) {
    int fb = 0;
    while ((1u << fb) < forced_buckets) ++fb;
    lb = std::min(lb, fb);
  }
  return lb;
}

// ---- the post-processing path ------------------------------------------------------------
// ceil(log2(n_seg)): the bits a segment index takes above a sort key
inline int seg_tag_bits(uint32_t n_seg) {
  int b = 0;
  while (b < 32 && (1ull << b) < n_seg) ++b;
  return b;
}

// Environment knobs of the build (diagnostics and A/B only), read by
// read_build_knobs() in build.cpp.
struct BuildKnobs {
  bool no_fused_bottom = false;  // SKS_NO_FUSED_BOTTOM: several narrow bottom-s genomes skip k_bottom_fused
  bool no_fast_bottom = false;   // SKS_NO_FAST_BOTTOM: one narrow bottom-s genome takes the general build
  bool no_frac_fused = false;    // SKS_NO_FRAC_FUSED: one narrow FracMinHash genome takes the general build
  bool scan_static = false;      // SKS_SCAN_STATIC: static tile ranges instead of the scan's tile queue
};

enum class PostPipe {
  kBottomFused,   // narrow bottom-s: sort, unique and select per genome in one kernel
  kFrac,          // FracMinHash: sort and unique
  kBottomSelect,  // narrow bottom-s: key sort, unique, select in LDS (hands over to pairs past its capacity)
  kBottomPairs,   // bottom-s by (fmh, k-mer) pairs
};

// How FracMinHash sorts the segments of a pass.
enum class FracSort {
  kTagged,     // the segment index rides above the key: one device-wide sort
  kTwoPass,    // narrow keys too wide for a tag: by key, then stable by segment
  kSegmented,  // each segment sorted on its own
};

struct PostPath {
  PostPipe pipe;
  FracSort sort;  // kFrac only
};

// n_seg segments to post-process, the longest region max_len records long.
// key_bits: the packed narrow key (64 when wide); mask_hi_bits: the bits of a
// wide key's high word.
//
// Narrow bottom-s with every genome's candidates in one workgroup's registers
// takes the fused kernel.  A single genome goes the device-wide way instead:
// one workgroup sorting its ~1.1 s candidates alone takes longer than the
// multi-workgroup radix sort (config 2: 0.35 vs 0.30 ms per build; from two
// genomes on the fused kernel wins, tools/ab_c2.sh).
//
// FracMinHash over several genomes: the segment index rides above the key (or,
// 128-bit, above the high word) and every sort is ONE device-wide radix sort
// over all segments; a segmented sort gives each genome one workgroup
// (reference sweep, 64 x 5 Mb at c = 200: 0.50 ms per narrow sort, 2 x 0.68 ms
// per 128-bit one).
inline PostPath choose_post_path(bool bottom, bool wide, uint32_t n_seg, uint64_t max_len, int key_bits,
                                 int mask_hi_bits, uint32_t fused_capacity, const BuildKnobs& knobs) {
  if (bottom) {
    if (wide) return {PostPipe::kBottomPairs, FracSort::kSegmented};
    const bool fused = max_len <= fused_capacity && n_seg >= 2 && !knobs.no_fused_bottom;
    return {fused ? PostPipe::kBottomFused : PostPipe::kBottomSelect, FracSort::kSegmented};
  }
  const int tag_at = wide ? mask_hi_bits : key_bits;
  if (n_seg >= 2 && tag_at + seg_tag_bits(n_seg) <= 64) return {PostPipe::kFrac, FracSort::kTagged};
  return {PostPipe::kFrac, !wide && n_seg >= 2 ? FracSort::kTwoPass : FracSort::kSegmented};
}

}  // namespace sks
