// CPU test of csrc/abund_plan.hpp (no HIP, no libsks): the run lengths the
// kernels derive from the runs' first indices and the segments' ends, checked
// exhaustively over small sorted multisets cut into segments against a naive
// count; the clamp at UINT32_MAX; the keep rule at its corners; the padded size
// of the sketch file's abundance section.  tests/test_abund_plan.py builds it
// with the address and undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "abund_plan.hpp"

using namespace sks;

namespace {

int failures = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      if (++failures > 20) std::exit(1);                               \
    }                                                                  \
  } while (0)

// What seg_unique_scan and the two run-length kernels compute, in their order:
// flags, their exclusive scan, the runs' first indices by rank, then a length
// per rank and a (first rank, distinct count) per segment.
struct Device {
  std::vector<uint32_t> abund;
  std::vector<uint64_t> starts;
  std::vector<uint32_t> sizes;
};

Device run_lengths(const std::vector<int>& keys, const std::vector<uint64_t>& off) {
  const size_t T = keys.size(), k = off.size() - 1;
  std::vector<uint32_t> flag(T + 1, 0);
  for (size_t g = 0; g < k; ++g)
    for (uint64_t i = off[g]; i < off[g + 1]; ++i) flag[i] = i == off[g] || keys[i] != keys[i - 1];
  std::vector<uint64_t> pos(T + 1, 0);
  for (size_t i = 0; i < T; ++i) pos[i + 1] = pos[i] + flag[i];
  std::vector<uint64_t> run_start(T + 1, ~0ull);
  for (size_t i = 0; i < T; ++i)
    if (flag[i]) run_start[pos[i]] = i;
  Device d;
  d.abund.assign(pos[T], 0);
  for (size_t g = 0; g < k; ++g) {
    const uint64_t rb = pos[off[g]], re = pos[off[g + 1]];
    for (uint64_t r = rb; r < re; ++r) d.abund[r] = abund_run_length(run_start.data(), r, re, off[g + 1]);
    d.starts.push_back(rb);
    d.sizes.push_back((uint32_t)(re - rb));
  }
  return d;
}

void check_case(const std::vector<int>& keys, const std::vector<uint64_t>& off) {
  const Device d = run_lengths(keys, off);
  size_t at = 0;
  for (size_t g = 0; g + 1 < off.size(); ++g) {
    // naive: count every value of the segment
    std::vector<std::pair<int, uint32_t>> want;
    for (uint64_t i = off[g]; i < off[g + 1]; ++i) {
      if (want.empty() || want.back().first != keys[i]) want.push_back({keys[i], 0});
      ++want.back().second;
    }
    CHECK(d.starts[g] == at);
    CHECK(d.sizes[g] == want.size());
    for (size_t j = 0; j < want.size(); ++j) CHECK(d.abund[at + j] == want[j].second);
    at += want.size();
  }
  CHECK(at == d.abund.size());
}

// every non-decreasing sequence of `len` values below `vals`, every way to cut it into `segs` segments
// (equal values on both sides of a cut are two runs: tagged keys of different segments differ)
void exhaustive(int len, int vals, int segs) {
  std::vector<int> keys(len, 0);
  for (;;) {
    std::vector<uint64_t> cut(segs - 1, 0);
    for (;;) {
      std::vector<uint64_t> off{0};
      for (uint64_t c : cut) off.push_back(c);
      off.push_back((uint64_t)len);
      bool ordered = true;
      for (size_t i = 1; i < off.size(); ++i) ordered = ordered && off[i - 1] <= off[i];
      if (ordered) check_case(keys, off);
      int i = 0;
      while (i < segs - 1 && cut[i] == (uint64_t)len) cut[i++] = 0;
      if (i == segs - 1) break;
      ++cut[i];
    }
    // next non-decreasing sequence
    int i = len - 1;
    while (i >= 0 && keys[i] == vals - 1) --i;
    if (i < 0) break;
    const int v = keys[i] + 1;
    for (int j = i; j < len; ++j) keys[j] = v;
  }
}

}  // namespace

int main() {
  check_case({}, {0, 0});
  check_case({}, {0, 0, 0});
  check_case({7}, {0, 0, 1, 1});
  for (int len = 1; len <= 7; ++len)
    for (int segs = 1; segs <= 3; ++segs) exhaustive(len, 3, segs);

  // a last run that ends at the segment's end, and the clamp
  {
    const uint64_t run_start[2] = {10, 14};
    CHECK(abund_run_length(run_start, 0, 2, 20) == 4);
    CHECK(abund_run_length(run_start, 1, 2, 20) == 6);
    CHECK(abund_run_end(run_start, 1, 2, 20) == 20);
    const uint64_t one[1] = {5};
    CHECK(abund_run_length(one, 0, 1, 5 + 0xffffffffull) == 0xffffffffu);
    CHECK(abund_run_length(one, 0, 1, 5 + 0x100000000ull) == 0xffffffffu);
    CHECK(abund_run_length(one, 0, 1, 5 + 0xfffffffeull) == 0xfffffffeu);
    CHECK(abund_run_length(one, 0, 1, 5 + (1ull << 40)) == 0xffffffffu);
    CHECK(abund_clamp(0) == 0 && abund_clamp(1) == 1 && abund_clamp(~0ull) == 0xffffffffu);
  }

  // the keep rule: the minimum is at least 1; both ends inclusive; UINT32_MAX is no limit
  CHECK(abund_floor(0) == 1 && abund_floor(1) == 1 && abund_floor(2) == 2);
  CHECK(abund_keeps(1, 0, kAbundNoLimit) && abund_keeps(1, 1, kAbundNoLimit));
  CHECK(!abund_keeps(1, 2, kAbundNoLimit) && abund_keeps(2, 2, kAbundNoLimit));
  CHECK(abund_keeps(2, 2, 3) && abund_keeps(3, 2, 3) && !abund_keeps(1, 2, 3) && !abund_keeps(4, 2, 3));
  CHECK(abund_keeps(1, 0, 1) && !abund_keeps(2, 0, 1));
  CHECK(!abund_keeps(1, 5, 2) && !abund_keeps(2, 5, 2) && !abund_keeps(3, 5, 2) && !abund_keeps(5, 5, 2));
  CHECK(!abund_keeps(1, 1, 0) && !abund_keeps(1, 0, 0));
  CHECK(abund_keeps(0xffffffffu, 1, kAbundNoLimit) && abund_keeps(0xffffffffu, 0xffffffffu, kAbundNoLimit));
  CHECK(!abund_keeps(0xfffffffeu, 0xffffffffu, kAbundNoLimit) && !abund_keeps(0xffffffffu, 1, 0xfffffffeu));
  CHECK(abund_keeps_all(0, kAbundNoLimit) && abund_keeps_all(1, kAbundNoLimit));
  CHECK(!abund_keeps_all(2, kAbundNoLimit) && !abund_keeps_all(1, 0xfffffffeu) && !abund_keeps_all(0, 0));

  // the file section: 4 bytes an element, zero-padded to 8
  CHECK(abund_section_bytes(0) == 0 && abund_section_bytes(1) == 8 && abund_section_bytes(2) == 8);
  CHECK(abund_section_bytes(3) == 16 && abund_section_bytes(1000001) == 4000008);
  CHECK(abund_section_bytes(1ull << 40) == (1ull << 42));

  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::puts("abund plan ok");
  return 0;
}
