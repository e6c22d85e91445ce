// csrc/build_plan.hpp on the CPU (no HIP, no libsks): the arithmetic that plans
// a sketch build.  Every expected value below is the formula evaluated by hand:
//   FracMinHash:  expect = L / c
//   bottom-s:     alpha = 1 + 10 / sqrt(s) + 1 / s, want = alpha * s;
//                 L <= want: no threshold (~0), expect = L
//                 else threshold = floor(want / L * 2^64), expect = want
//   capacity        = min(floor(expect + 6 sqrt(expect) + 4096), L + 1)
//   single capacity = min(capacity, floor(e + 8 sqrt(e) + 256)), e = min(L, want)
//   retry:  threshold * 8, ~0 once threshold > ~0 >> 3;
//           capacity = min(L + 1, max(capacity, count) * 8 + 4096)
//   fused FracMinHash buckets: the least 2^b >= ceil(max(cap, 1) / (bucket / 4)),
//           -1 above the largest b, never more than a forced bucket count
#include <cstdint>
#include <cstdio>

#include "build_plan.hpp"

namespace {

int failures = 0;

void check(bool ok, const char* what) {
  if (ok) return;
  std::printf("FAIL %s\n", what);
  ++failures;
}

constexpr uint64_t kNone = ~0ull;

void capacities() {
  // FracMinHash, L = 5 000 000, c = 200: expect 25000; sqrt = 158.11..; 25000 + 948.68 + 4096 = 30044.68
  sks::SegPlan p = sks::plan_segment(false, 200, 5000000);
  check(p.thresh == kNone && p.cap == 30044, "frac 5 Mb c=200: capacity 30044, no threshold");

  // bottom-s, s = 10 000, L = 5 000 000: alpha = 1 + 0.1 + 0.0001 = 1.1001, alpha * s = 11001;
  // sqrt(11001) = 104.8856..; general 11001 + 629.31 + 4096 = 15726.31; single 11001 + 839.08 + 256 = 12096.08;
  // threshold floor(11001 * 2^64 / 5 000 000) = 40586526310975755 (remainder 0.47: clear of rounding)
  check(sks::bottom_alpha(10000) * 10000.0 == 11001.0, "bottom s=10000: alpha * s = 11001");
  p = sks::plan_segment(true, 10000, 5000000);
  check(p.cap == 15726, "bottom s=10000 5 Mb: general capacity 15726");
  check(p.thresh == 40586526310975755ull, "bottom s=10000 5 Mb: threshold floor(11001 / 5e6 * 2^64)");
  const uint64_t single = sks::bottom_single_capacity(10000, 5000000, p.cap);
  check(single == 12096, "bottom s=10000 5 Mb: single-genome capacity 12096");
  check(single <= 16384, "bottom s=10000 5 Mb: the single-genome capacity fits the fused kernel (16384)");

  // L <= alpha * s: every window is a candidate; capacity min(11001 + 629.31 + 4096, L + 1) = L + 1
  p = sks::plan_segment(true, 10000, 11001);
  check(p.thresh == kNone && p.cap == 11002, "bottom L = alpha * s: no threshold, capacity L + 1");
  check(sks::bottom_single_capacity(10000, 11001, p.cap) == 11002, "bottom L = alpha * s: single capacity L + 1");
  // one base longer: a threshold just below 2^64 (11001 / 11002 of it), capacity min(15726, 11003)
  p = sks::plan_segment(true, 10000, 11002);
  check(p.thresh != kNone && p.thresh > (kNone / 11002) * 11000 && p.cap == 11003,
        "bottom L = alpha * s + 1: a threshold, capacity L + 1");
  // L = 0: expect 0, min(4096, 1) = 1; single min(1, 0 + 0 + 256) = 1
  p = sks::plan_segment(false, 200, 0);
  check(p.thresh == kNone && p.cap == 1, "frac L = 0: capacity 1");
  p = sks::plan_segment(true, 10000, 0);
  check(p.thresh == kNone && p.cap == 1, "bottom L = 0: capacity 1, no threshold");
  check(sks::bottom_single_capacity(10000, 0, 1) == 1, "bottom L = 0: single capacity 1");
  // L = 1: min(4096.., 2) = 2 either way; single min(2, floor(1 + 8 + 256)) = 2
  p = sks::plan_segment(false, 200, 1);
  check(p.thresh == kNone && p.cap == 2, "frac L = 1: capacity 2");
  p = sks::plan_segment(true, 10000, 1);
  check(p.thresh == kNone && p.cap == 2, "bottom L = 1: capacity 2, no threshold");
  check(sks::bottom_single_capacity(10000, 1, 2) == 2, "bottom L = 1: single capacity 2");
}

void escalation() {
  // ~0 >> 3 = 2305843009213693951: times 8 still fits (2^64 - 8); one more saturates
  sks::SegPlan p = sks::escalate({2305843009213693951ull, 1000}, 2000, 1000000);
  check(p.thresh == 18446744073709551608ull, "retry: threshold ~0 >> 3 goes to 2^64 - 8");
  check(p.cap == 20096, "retry: capacity max(1000, 2000) * 8 + 4096 = 20096");
  p = sks::escalate({2305843009213693952ull, 3000}, 2000, 1000000);
  check(p.thresh == kNone, "retry: threshold above ~0 >> 3 saturates");
  check(p.cap == 28096, "retry: capacity max(3000, 2000) * 8 + 4096 = 28096");
  p = sks::escalate({kNone, 1000}, 2000, 10000);
  check(p.thresh == kNone && p.cap == 10001, "retry: capacity clipped to L + 1");
}

void frac_buckets() {
  // bucket capacity 4096: 1024 keys per mean bucket; at most 2^14 buckets
  check(sks::frac_plan_log_b(0, 4096, 14, 0) == 0, "log_b: an empty region takes one bucket");
  check(sks::frac_plan_log_b(8192, 4096, 14, 0) == 3, "log_b: 8 * 1024 keys take 8 buckets");
  check(sks::frac_plan_log_b(8193, 4096, 14, 0) == 4, "log_b: one key more takes 16 buckets");
  check(sks::frac_plan_log_b(30044, 4096, 14, 0) == 5, "log_b: 30044 keys (ceil 29.3 = 30) take 32 buckets");
  check(sks::frac_plan_log_b(16777216, 4096, 14, 0) == 14, "log_b: 2^14 * 1024 keys take the most buckets");
  check(sks::frac_plan_log_b(16777217, 4096, 14, 0) == -1, "log_b: one key more does not fit");
  check(sks::frac_plan_log_b(30044, 4096, 14, 4) == 2, "log_b: forced to 4 buckets");
  check(sks::frac_plan_log_b(30044, 4096, 14, 3) == 2, "log_b: forced to 3 buckets rounds up to 4");
  check(sks::frac_plan_log_b(8192, 4096, 14, 64) == 3, "log_b: a forced count above the need changes nothing");
}

bool is(sks::PostPath p, sks::PostPipe pipe) { return p.pipe == pipe; }
bool is(sks::PostPath p, sks::FracSort sort) { return p.pipe == sks::PostPipe::kFrac && p.sort == sort; }

void post_paths() {
  using sks::FracSort;
  using sks::PostPipe;
  const sks::BuildKnobs none;
  const uint32_t fuse = 16384;
  // bottom-s, narrow: one genome sorts device-wide, from two the fused kernel; a region past its capacity does not
  check(is(sks::choose_post_path(true, false, 1, 12000, 42, 1, fuse, none), PostPipe::kBottomSelect),
        "bottom narrow k=1: not fused");
  check(is(sks::choose_post_path(true, false, 2, 12000, 42, 1, fuse, none), PostPipe::kBottomFused),
        "bottom narrow k=2: fused");
  check(is(sks::choose_post_path(true, false, 2, fuse, 42, 1, fuse, none), PostPipe::kBottomFused),
        "bottom narrow at the fused capacity: fused");
  check(is(sks::choose_post_path(true, false, 2, fuse + 1, 42, 1, fuse, none), PostPipe::kBottomSelect),
        "bottom narrow one above the fused capacity: not fused");
  check(is(sks::choose_post_path(true, true, 2, 100, 64, 16, fuse, none), PostPipe::kBottomPairs),
        "bottom wide: pairs");
  // FracMinHash narrow, 60 key bits: 16 segments take a 4-bit tag (64 bits), 17 a 5-bit one (65)
  check(is(sks::choose_post_path(false, false, 16, 100, 60, 1, fuse, none), FracSort::kTagged),
        "frac narrow 60 bits, 16 segments: tagged");
  check(is(sks::choose_post_path(false, false, 17, 100, 60, 1, fuse, none), FracSort::kTwoPass),
        "frac narrow 60 bits, 17 segments: two-pass");
  check(is(sks::choose_post_path(false, false, 1, 100, 60, 1, fuse, none), FracSort::kSegmented),
        "frac narrow, one segment: segmented");
  // wide: the tag rides above the high word's mask bits
  check(is(sks::choose_post_path(false, true, 2, 100, 64, 64, fuse, none), FracSort::kSegmented),
        "frac wide, 64 high bits: segmented");
  check(is(sks::choose_post_path(false, true, 2, 100, 64, 16, fuse, none), FracSort::kTagged),
        "frac wide, 16 high bits: tagged");
  check(is(sks::choose_post_path(false, true, 1, 100, 64, 16, fuse, none), FracSort::kSegmented),
        "frac wide, one segment: segmented");
  // the knobs: only no_fused_bottom bears on the post path, and only on narrow bottom-s
  sks::BuildKnobs k;
  k.no_fused_bottom = true;
  check(is(sks::choose_post_path(true, false, 2, 12000, 42, 1, fuse, k), PostPipe::kBottomSelect),
        "no_fused_bottom: not fused");
  check(is(sks::choose_post_path(false, false, 16, 100, 60, 1, fuse, k), FracSort::kTagged),
        "no_fused_bottom: FracMinHash unchanged");
  k = sks::BuildKnobs{};
  k.no_fast_bottom = k.no_frac_fused = k.scan_static = true;
  check(is(sks::choose_post_path(true, false, 2, 12000, 42, 1, fuse, k), PostPipe::kBottomFused),
        "no_fast_bottom, no_frac_fused, scan_static: the post path is unchanged (bottom)");
  check(is(sks::choose_post_path(false, false, 17, 100, 60, 1, fuse, k), FracSort::kTwoPass),
        "no_fast_bottom, no_frac_fused, scan_static: the post path is unchanged (frac)");
  check(!none.no_fused_bottom && !none.no_fast_bottom && !none.no_frac_fused && !none.scan_static,
        "every knob is off by default");
  check(sks::seg_tag_bits(1) == 0 && sks::seg_tag_bits(2) == 1 && sks::seg_tag_bits(16) == 4 &&
            sks::seg_tag_bits(17) == 5,
        "tag bits: ceil(log2(segments))");
}

}  // namespace

int main() {
  capacities();
  escalation();
  frac_buckets();
  post_paths();
  if (failures) return 1;
  std::printf("plan ok\n");
  return 0;
}
