// The arithmetic of sks_sketch_set_merge (no HIP: tests/cpp/merge_plan_test.cpp
// runs it on any machine, and merge.hip runs the same functions on the device):
// the merge-path partition, which workgroup owns which tile of a dense grid,
// and the plan of the pairwise merge rounds.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SKS_PLAN_HD __host__ __device__
#else
#define SKS_PLAN_HD
#endif

namespace sks {

constexpr uint32_t kMergeTile = 1024;        // outputs of one pair per workgroup
constexpr uint32_t kMergeNoRun = 0xffffffffu;  // MergePair::b of a carried (copied) run

// How many of the first d outputs of the stable merge of the sorted runs
// a(0 .. na) and b(0 .. nb) come from a.  Stable: on equal keys the element of
// a goes first.  a(i) and b(j) read one element, less(x, y) is the strict
// order, 0 <= d <= na + nb.  The partitions of growing d never decrease, and
// cutting both runs at the partitions of a tile's two diagonals gives exactly
// the inputs of that tile's outputs.
template <class A, class B, class Less>
SKS_PLAN_HD inline uint32_t merge_path(A a, uint32_t na, B b, uint32_t nb, uint32_t d, Less less) {
  uint32_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    // a(mid) is among the first d outputs iff it does not come after b(d - 1 - mid)
    if (!less(b(d - 1 - mid), a(mid)))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The owner of tile `t` of a dense grid: off[0 .. n] is the non-decreasing
// number of tiles before each of n owners (n >= 1, off[0] == 0, t < off[n]);
// the owner p has off[p] <= t < off[p + 1] (owners without tiles are skipped).
SKS_PLAN_HD inline uint32_t tile_owner(const uint64_t* off, uint32_t n, uint64_t t) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= t)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

SKS_PLAN_HD inline uint64_t tiles_of(uint64_t len, uint32_t tile) { return (len + tile - 1) / tile; }

// ---- the rounds (host) -----------------------------------------------------------------
// Group g's members are the runs member_len[group_off[g] .. group_off[g + 1]).
// Round r merges a group's adjacent runs pairwise, an odd last run is carried
// (copied), until one run is left; a group of m members takes part in
// ceil(log2(m)) rounds and in none once it is down to one run.  Every round
// writes group g's runs back to back from element dense_off[g] of its output
// buffer, so all rounds share one layout and a finished group stays where its
// last round left it.
struct MergePair {
  uint32_t a, b;  // runs of the round's input: round 0, positions in the member list;
                  // later, indices into the previous round's `out`.  b == kMergeNoRun: a is copied
};
struct MergeRun {
  uint64_t off;  // first element in the round's output buffer
  uint32_t len;
};
struct MergeRound {
  std::vector<MergePair> pairs;
  std::vector<MergeRun> out;        // out[p]: the run pair p leaves
  std::vector<uint64_t> tile_off;   // [pairs + 1] tiles before each pair
};
struct MergeFinal {
  int round;     // the round that left the group's one run; -1: a member as it is (or no member)
  uint32_t run;  // index into that round's `out`; round -1: position in the member list (kMergeNoRun: empty group)
  uint64_t len;  // elements of the group, duplicates included
};
struct MergePlan {
  std::vector<MergeRound> rounds;
  std::vector<uint64_t> dense_off;  // [groups + 1] elements before each group, duplicates included
  std::vector<MergeFinal> final_run;
};

inline MergePlan plan_merge(const std::vector<uint32_t>& group_off, const std::vector<uint32_t>& member_len,
                            uint32_t tile = kMergeTile) {
  const uint32_t n_groups = (uint32_t)group_off.size() - 1;
  MergePlan P;
  P.dense_off.assign(n_groups + 1, 0);
  P.final_run.resize(n_groups);
  // the runs each group still holds: indices as MergePair names them, and their lengths
  std::vector<std::vector<uint32_t>> cur(n_groups), len(n_groups);
  bool more = false;
  for (uint32_t g = 0; g < n_groups; ++g) {
    uint64_t sum = 0;
    for (uint32_t j = group_off[g]; j < group_off[g + 1]; ++j) {
      cur[g].push_back(j);
      len[g].push_back(member_len[j]);
      sum += member_len[j];
    }
    P.dense_off[g + 1] = P.dense_off[g] + sum;
    P.final_run[g] = {-1, cur[g].empty() ? kMergeNoRun : cur[g][0], sum};
    more = more || cur[g].size() > 1;
  }
  for (int r = 0; more; ++r) {
    MergeRound R;
    R.tile_off.push_back(0);
    more = false;
    for (uint32_t g = 0; g < n_groups; ++g) {
      if (cur[g].size() < 2) continue;
      std::vector<uint32_t> next, next_len;
      uint64_t at = P.dense_off[g];
      for (size_t i = 0; i < cur[g].size(); i += 2) {
        const bool pair = i + 1 < cur[g].size();
        const uint32_t l = len[g][i] + (pair ? len[g][i + 1] : 0);
        next.push_back((uint32_t)R.pairs.size());
        next_len.push_back(l);
        R.pairs.push_back({cur[g][i], pair ? cur[g][i + 1] : kMergeNoRun});
        R.out.push_back({at, l});
        R.tile_off.push_back(R.tile_off.back() + tiles_of(l, tile));
        at += l;
      }
      cur[g].swap(next);
      len[g].swap(next_len);
      if (cur[g].size() == 1) P.final_run[g] = {r, cur[g][0], P.final_run[g].len};
      more = more || cur[g].size() > 1;
    }
    P.rounds.push_back(std::move(R));
  }
  return P;
}

}  // namespace sks
