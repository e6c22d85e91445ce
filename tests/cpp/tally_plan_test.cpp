// CPU check of csrc/tally_plan.hpp (no HIP, no libsks): the keep rule and the
// run-end search of the tally's last pass, exhaustively over small sorted
// multisets against a naive run-length count, with a reader that fails the
// program when asked for a position at or beyond the group's length (the array
// goes on behind the group with the group's last value, as the next group's run
// or the source set's next sketch may); the effective limits; and the
// fraction-to-count rule of the command line against values worked out by hand.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tally_plan.hpp"

using namespace sks;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

namespace {

uint64_t n_reads = 0;

// Reads position i of a group of `size` elements; the array itself is longer.
struct Guarded {
  const int* p;
  uint64_t size;
  int operator()(uint64_t i) const {
    if (i >= size) {
      std::fprintf(stderr, "read of position %llu of a group of %llu elements\n", (unsigned long long)i,
                   (unsigned long long)size);
      std::exit(1);
    }
    ++n_reads;
    return p[i];
  }
};
struct Same {
  bool operator()(int x, int y) const { return x == y; }
};

// every non-decreasing array over {0..3} of length 0..max_len
std::vector<std::vector<int>> sorted_arrays(size_t max_len) {
  std::vector<std::vector<int>> all{{}};
  for (size_t at = 0, len = 0; len < max_len; ++len) {
    const size_t end = all.size();
    for (; at < end; ++at)
      for (int v = all[at].empty() ? 0 : all[at].back(); v < 4; ++v) {
        std::vector<int> next = all[at];
        next.push_back(v);
        all.push_back(next);
      }
  }
  return all;
}

uint64_t check_group(const std::vector<int>& group, const std::vector<uint32_t>& limits) {
  const uint64_t size = group.size();
  // behind the group: its last value again (twice), then a larger one
  std::vector<int> mem = group;
  const int last = group.empty() ? 0 : group.back();
  mem.insert(mem.end(), {last, last, 9});
  // naive: run length of the run each position heads (0: not a head)
  std::vector<uint32_t> heads(size, 0);
  uint32_t longest = 0;
  for (uint64_t i = 0; i < size;) {
    uint64_t e = i;
    while (e < size && group[e] == group[i]) ++e;
    heads[i] = (uint32_t)(e - i);
    if (heads[i] > longest) longest = heads[i];
    i = e;
  }
  const Guarded at{mem.data(), size};
  uint64_t checks = 0;
  for (uint32_t lo : limits) {
    if (lo == 0 || lo == kTallyNoLimit) continue;  // tally_lo never gives 0
    for (uint32_t hi : limits)
      for (uint64_t i = 0; i < size; ++i) {
        int v = -1;
        n_reads = 0;
        const bool keep = tally_keeps(at, Same{}, i, size, lo, hi, &v);
        CHECK(n_reads <= 4);  // the element, its predecessor, and the two of the rule
        CHECK(v == group[i]);
        CHECK(keep == (heads[i] >= lo && heads[i] <= hi && heads[i] > 0));
        ++checks;
        if (!keep) continue;
        // m: the group's listed members, at least the longest run
        for (uint32_t m : {longest, longest + 1, (uint32_t)size, 1100u, kTallyNoLimit}) {
          if (m < longest) continue;
          n_reads = 0;
          CHECK(tally_run_length(at, Same{}, v, i, size, lo, hi, m) == heads[i]);
          const uint32_t range = (hi < m ? hi : m) - lo + 1;  // at most ceil(log2(range + 1)) reads
          uint32_t steps = 0;
          while ((1ull << steps) < (uint64_t)range + 1) ++steps;
          CHECK(n_reads <= steps);
        }
      }
  }
  return checks;
}

void check_limits() {
  const uint32_t lo[4] = {0, 1, 7, kTallyNoLimit}, hi[3] = {0, 5, kTallyNoLimit};
  CHECK(tally_lo(nullptr, 3) == 1 && tally_lo(lo, 0) == 1 && tally_lo(lo, 1) == 1 && tally_lo(lo, 2) == 7);
  CHECK(tally_lo(lo, 3) == kTallyNoLimit);
  CHECK(tally_hi(nullptr, 2) == kTallyNoLimit && tally_hi(hi, 0) == 0 && tally_hi(hi, 1) == 5);
  CHECK(tally_hi(hi, 2) == kTallyNoLimit);
  // a group of nearly 2^32 equal values: the 64-bit sums do not wrap (reads are answered without memory)
  struct Const {
    uint64_t size;
    int operator()(uint64_t i) const {
      CHECK(i < size);
      return 5;
    }
  };
  const uint64_t big = 0xffffffffull;
  int v = 0;
  CHECK(tally_keeps(Const{big}, Same{}, 0, big, 1, kTallyNoLimit, &v));
  CHECK(tally_keeps(Const{big}, Same{}, 0, big, kTallyNoLimit, kTallyNoLimit, &v));
  CHECK(!tally_keeps(Const{big}, Same{}, 0, big, 1, kTallyNoLimit - 1, &v));
  CHECK(!tally_keeps(Const{big}, Same{}, big - 1, big, 1, kTallyNoLimit, &v));  // not a head
  CHECK(tally_run_length(Const{big}, Same{}, 5, 0, big, 1, kTallyNoLimit, kTallyNoLimit) == kTallyNoLimit);
}

void check_fractions() {
  TallyThreshold t;
  CHECK(!tally_parse_threshold("-", &t) && t.kind == TallyThreshold::kNone);
  CHECK(tally_min_of(t, 10) == 1 && tally_max_of(t, 10) == kTallyNoLimit);
  CHECK(!tally_parse_threshold("3", &t) && t.kind == TallyThreshold::kCount && t.count == 3);
  CHECK(tally_min_of(t, 10) == 3 && tally_max_of(t, 10) == 3);
  CHECK(!tally_parse_threshold("0", &t) && t.kind == TallyThreshold::kCount && t.count == 0);
  CHECK(!tally_parse_threshold("4294967295", &t) && t.count == kTallyNoLimit);
  CHECK(!tally_parse_threshold("0.9", &t) && t.kind == TallyThreshold::kFraction && t.num == 9 && t.den == 10);
  // 0.9 of m as a minimum: ceil; as a maximum: floor
  CHECK(tally_min_of(t, 10) == 9 && tally_max_of(t, 10) == 9);
  CHECK(tally_min_of(t, 100) == 90 && tally_max_of(t, 100) == 90);
  CHECK(tally_min_of(t, 8) == 8 && tally_max_of(t, 8) == 7);     // 7.2
  CHECK(tally_min_of(t, 1) == 1 && tally_max_of(t, 1) == 0);     // 0.9
  CHECK(tally_min_of(t, 0) == 1 && tally_max_of(t, 0) == 0);     // an empty group: at least 1
  CHECK(tally_min_of(t, 1000) == 900 && tally_max_of(t, 1000) == 900);
  CHECK(!tally_parse_threshold("1.0", &t) && t.num == 10 && t.den == 10);
  CHECK(tally_min_of(t, 7) == 7 && tally_max_of(t, 7) == 7);
  CHECK(!tally_parse_threshold("1.", &t) && t.kind == TallyThreshold::kFraction && tally_min_of(t, 7) == 7);
  CHECK(!tally_parse_threshold(".5", &t) && t.num == 5 && t.den == 10);
  CHECK(tally_min_of(t, 3) == 2 && tally_max_of(t, 3) == 1);     // 1.5
  CHECK(!tally_parse_threshold("0.0", &t) && tally_min_of(t, 9) == 1 && tally_max_of(t, 9) == 0);
  CHECK(!tally_parse_threshold("0.7", &t) && tally_min_of(t, 10) == 7 && tally_max_of(t, 10) == 7);  // not 8, not 6
  CHECK(!tally_parse_threshold("0.1", &t) && tally_min_of(t, 30) == 3 && tally_max_of(t, 30) == 3);
  CHECK(!tally_parse_threshold("0.333333333", &t) && t.den == 1000000000ull);
  CHECK(tally_min_of(t, 3) == 1 && tally_max_of(t, 3) == 0);     // 0.999999999
  CHECK(tally_min_of(t, 0xffffffffu) == 1431655764u);            // 1431655763.9...
  // refused
  for (const char* bad : {"", "abc", "1.5", "2.0", "1.01", "-1", "0.9x", "0..9", ".", "1e3", "0.1234567891", "--",
                          "4294967296", " 3", "+3", "0,9"})
    CHECK(tally_parse_threshold(bad, &t) != nullptr);
  CHECK(tally_parse_threshold(nullptr, &t) != nullptr);
}

}  // namespace

int main() {
  std::vector<uint32_t> limits;
  for (uint32_t v = 0; v <= 14; ++v) limits.push_back(v);
  limits.push_back(kTallyNoLimit);
  uint64_t checks = 0, groups = 0;
  for (const std::vector<int>& g : sorted_arrays(12)) {
    checks += check_group(g, limits);
    ++groups;
  }
  CHECK(groups == 1820);  // C(16, 4): multisets of up to 12 elements over 4 values
  check_limits();
  check_fractions();
  std::printf("tally plan ok: %llu groups, %llu keep decisions\n", (unsigned long long)groups,
              (unsigned long long)checks);
  return 0;
}
