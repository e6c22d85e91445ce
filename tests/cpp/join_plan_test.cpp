// The host arithmetic of the join (csrc/join_plan.hpp) on the CPU: no HIP, no
// libsks.  Bucket groups per tile for every bucket count, for tile counts from
// one to millions and for the default rule and forced workgroup totals; the
// launches a call is cut into; the diagonal-last condition; the choice between
// the contiguous and the piecewise kernel; the bucket count of a layout.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "join_plan.hpp"

using namespace sks;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

namespace {

const uint64_t kTiles[] = {1, 3, 6, 136, 276, 1035, 70000, 5000000};

void test_groups() {
  for (uint32_t log_b = 0; log_b <= 14; ++log_b) {
    const uint32_t B = 1u << log_b;
    for (uint64_t tiles : kTiles) {
      const uint64_t overrides[] = {0, 1, 3 * tiles, 1ull << 40};
      for (uint64_t wgs : overrides) {
        const JoinGroups g = join_plan_groups(B, tiles, wgs);
        CHECK(g.groups >= 1 && g.groups <= B);
        CHECK(g.n_groups >= 1 && g.n_groups <= B && g.n_groups <= g.groups);
        CHECK(g.buckets_per_group >= 1);
        // no empty group, no bucket lost
        CHECK((uint64_t)(g.n_groups - 1) * g.buckets_per_group < B);
        CHECK((uint64_t)g.n_groups * g.buckets_per_group >= B);
        const uint64_t tpl = join_plan_tiles_per_launch(g.n_groups);
        CHECK(tpl >= 1 && tpl * g.n_groups <= kJoinMaxGrid);
        CHECK(tpl * g.n_groups * 512 < (1ull << 32));  // work-items of one launch
        CHECK((tpl + 1) * g.n_groups > kJoinMaxGrid);  // and no fewer tiles than fit
        // a forced total: one group, three groups (while B holds three), one bucket a group
        if (wgs == 1) CHECK(g.n_groups == 1 && g.buckets_per_group == B);
        if (wgs == 3 * tiles && B >= 8) CHECK(g.groups == 3 && g.n_groups == 3 && g.buckets_per_group == (B + 2) / 3);
        if (wgs == (1ull << 40)) CHECK(g.n_groups == B && g.buckets_per_group == 1 && tpl == kJoinMaxGrid / B);
        // the default rule: at least 16 buckets a group, about 1024 workgroups when few tiles
        if (wgs == 0 && B >= 16) CHECK(g.buckets_per_group >= 16);
        if (wgs == 0) CHECK(g.groups <= std::max<uint32_t>(1, (B + 127) / 128) || g.groups * tiles < 1024 + tiles);
      }
    }
  }
  // the groups per tile the tuned cases have had: config 4 (1000 sketches of
  // 10000: B = 4096, 136 tiles) 32, and 150 sketches at log_b = 11 (6 tiles) 128
  CHECK(join_plan_groups(4096, 136, 0).n_groups == 32 && join_plan_groups(4096, 136, 0).buckets_per_group == 128);
  CHECK(join_plan_groups(2048, 6, 0).n_groups == 128 && join_plan_groups(2048, 6, 0).buckets_per_group == 16);
  // very many tiles: fewer, larger groups, down to one
  CHECK(join_plan_groups(16384, 70000, 0).n_groups == 1);
  CHECK(join_plan_groups(16384, 1035, 0).n_groups == 64);
  // 23 blocks at one bucket a group: 276 tiles in launches of 256 and 20
  const JoinGroups g = join_plan_groups(16384, 276, 1ull << 40);
  CHECK(g.n_groups == 16384 && join_plan_tiles_per_launch(g.n_groups) == 256);
  CHECK(join_plan_slices(0, 276, 256) == 2 && join_plan_slice_tiles(0, 276, 1, 256) == 20);
}

void test_slices() {
  for (uint64_t tpl : {1ull, 2ull, 7ull, 256ull, 4194304ull})
    for (uint64_t begin : {0ull, 1ull, 5ull, 255ull, 256ull, 1000003ull})
      for (uint64_t len : {0ull, 1ull, 2ull, 6ull, 7ull, 8ull, 255ull, 256ull, 257ull, 276ull, 513ull}) {
        const uint64_t end = begin + len, n = join_plan_slices(begin, end, tpl);
        if (n > 4096) continue;
        CHECK((len == 0) == (n == 0));
        uint64_t next = begin;  // the launches tile [begin, end) in order, none empty, all but the last full
        for (uint64_t s = 0; s < n; ++s) {
          const uint64_t b = join_plan_slice_begin(begin, s, tpl), nt = join_plan_slice_tiles(begin, end, s, tpl);
          CHECK(b == next && nt >= 1 && nt <= tpl && (s + 1 == n || nt == tpl));
          // packed output and tile counters: the tiles of the earlier launches come first
          CHECK(join_plan_slice_offset(begin, s, tpl) == b - begin && b - begin == s * tpl);
          next = b + nt;
        }
        CHECK(next == end);
      }
}

void test_diag_last() {
  // 3 blocks: 6 tiles
  CHECK(join_plan_diag_last(true, false, 0, 6, 3, 256, false));
  CHECK(!join_plan_diag_last(true, false, 0, 6, 3, 256, true));   // plain order asked for
  CHECK(!join_plan_diag_last(false, false, 0, 6, 3, 256, false));  // row blocks
  CHECK(!join_plan_diag_last(true, true, 0, 6, 3, 256, false));   // a tile list
  CHECK(!join_plan_diag_last(true, false, 0, 5, 3, 256, false));  // a tile range
  CHECK(!join_plan_diag_last(true, false, 1, 6, 3, 256, false));
  CHECK(!join_plan_diag_last(true, false, 0, 6, 3, 5, false));    // more than one launch
  CHECK(join_plan_diag_last(true, false, 0, 6, 3, 6, false));
  CHECK(!join_plan_diag_last(true, false, 0, 276, 23, 256, false));
  // block counts whose tile count needs 64 bits of the product
  CHECK(join_plan_diag_last(true, false, 0, 70000ull * 70001 / 2, 70000, 1ull << 40, false));
}

void test_kernel_choice() {
  for (uint32_t log_b = 0; log_b <= 14; ++log_b)
    for (uint32_t rg = 0; rg <= 3; ++rg) {
      const uint32_t rb = join_plan_region_bucket_log(log_b, rg);
      CHECK(rb == std::min(log_b, 3 + rg) && rb <= kJoinWinLog);
      const bool wide = rb >= kJoinWinLog;  // 64-bucket regions: rg = 3 at log_b >= 6
      CHECK(wide == (rg == 3 && log_b >= 6));
      // one layout of all sketches, no tile list: by the region log its build took
      CHECK(join_plan_contiguous(log_b, rg, -1, true, false, 0, 0) == wide);
      // two layouts, block offsets and tile lists are never known to be contiguous ...
      CHECK(!join_plan_contiguous(log_b, rg, -1, false, false, 0, 0));
      CHECK(!join_plan_contiguous(log_b, rg, -1, true, true, 0, 0));
      CHECK(!join_plan_contiguous(log_b, rg, -1, true, false, 1, 0));
      CHECK(!join_plan_contiguous(log_b, rg, -1, true, false, 0, ~0u));
      // ... unless the caller names the region log of its one layout
      for (uint32_t nat = 0; nat <= 3; ++nat) {
        CHECK(join_plan_contiguous(log_b, nat, (int)rg, true, true, 5, 5) == wide);
        CHECK(!join_plan_contiguous(log_b, nat, (int)rg, false, true, 5, 5));
      }
    }
}

void test_log_b() {
  // cap 1024: 170 raw elements a bucket; 64 sketches of 21760 fill 2^13 buckets exactly
  CHECK(join_plan_log_b(21760, 1024) == 13 && join_plan_log_b(21761, 1024) == 14);
  CHECK(join_plan_log_b(0, 1024) == 0 && join_plan_log_b(1, 1024) == 0 && join_plan_log_b(2, 1024) == 0);
  CHECK(join_plan_log_b(3, 1024) == 1);
  CHECK(join_plan_log_b(~0u, 1024) == 14 && join_plan_log_b(~0u, 64) == 14);
  for (uint32_t cap : {64u, 200u, 1024u}) {
    uint32_t last = 0;
    for (uint32_t size : {0u, 1u, 10u, 100u, 600u, 1000u, 3000u, 10000u, 21760u, 100000u, 400000u, 5000000u}) {
      const uint32_t lb = join_plan_log_b(size, cap);
      CHECK(lb >= last && lb <= kJoinMaxLogB);  // monotone in the size
      CHECK(lb >= join_plan_log_b(size, 1024));  // a smaller chunk never takes fewer buckets
      // the smallest count whose mean raw block-bucket is at most cap / 6, or the limit
      CHECK(lb == kJoinMaxLogB || (1ull << lb) * (cap / 6) >= 64ull * size);
      CHECK(lb == 0 || (1ull << (lb - 1)) * (cap / 6) < 64ull * size);
      last = lb;
    }
  }
  CHECK(join_plan_log_b(600, 64) > join_plan_log_b(600, 1024));  // the bucket count moves with the capacity
}

}  // namespace

int main() {
  test_groups();
  test_slices();
  test_diag_last();
  test_kernel_choice();
  test_log_b();
  std::printf("join plan ok\n");
  return 0;
}
