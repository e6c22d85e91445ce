// CPU check of csrc/merge_plan.hpp (no HIP, no libsks): the merge-path
// partition the merge kernel cuts its tiles with, exhaustively over small
// sorted arrays against std::merge; the owner search of the dense grids; and the
// plan of the pairwise rounds against values worked out by hand.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "merge_plan.hpp"

using namespace sks;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

namespace {

struct El {
  int key, id;  // id tells the runs and positions apart: equal keys stay distinguishable
};
bool same(const El& x, const El& y) { return x.key == y.key && x.id == y.id; }
struct ByKey {
  bool operator()(const El& x, const El& y) const { return x.key < y.key; }
};
struct Read {
  const El* p;
  El operator()(uint32_t i) const { return p[i]; }
};

// every non-decreasing array over {0..3} of length 0..5
std::vector<std::vector<int>> sorted_arrays() {
  std::vector<std::vector<int>> all{{}};
  for (size_t at = 0, len = 0; len < 5; ++len) {
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

uint64_t check_pair(const std::vector<int>& ka, const std::vector<int>& kb) {
  std::vector<El> a, b, want;
  for (size_t i = 0; i < ka.size(); ++i) a.push_back({ka[i], (int)i});
  for (size_t j = 0; j < kb.size(); ++j) b.push_back({kb[j], 100 + (int)j});
  std::merge(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(want), ByKey{});
  const uint32_t na = (uint32_t)a.size(), nb = (uint32_t)b.size(), n = na + nb;
  const Read ra{a.data()}, rb{b.data()};
  // every diagonal: in range, monotone, and the prefix it cuts is the merge's prefix
  uint32_t before = 0;
  for (uint32_t d = 0; d <= n; ++d) {
    const uint32_t i = merge_path(ra, na, rb, nb, d, ByKey{});
    CHECK(i <= na && i <= d && d - i <= nb);
    CHECK(i >= before && (d == 0 || (d - i) >= (d - 1 - before)));
    before = i;
  }
  CHECK(merge_path(ra, na, rb, nb, 0, ByKey{}) == 0 && merge_path(ra, na, rb, nb, n, ByKey{}) == na);
  uint64_t tiles = 0;
  for (uint32_t tile : {1u, 2u, 3u, 7u}) {
    std::vector<El> got;
    for (uint32_t d0 = 0; d0 < n; d0 += tile, ++tiles) {
      const uint32_t d1 = std::min(d0 + tile, n);
      const uint32_t a0 = merge_path(ra, na, rb, nb, d0, ByKey{}), a1 = merge_path(ra, na, rb, nb, d1, ByKey{});
      const uint32_t b0 = d0 - a0, b1 = d1 - a1;
      CHECK(a0 <= a1 && b0 <= b1 && (a1 - a0) + (b1 - b0) == d1 - d0);  // the parts sum to the diagonal
      std::merge(a.begin() + a0, a.begin() + a1, b.begin() + b0, b.begin() + b1, std::back_inserter(got), ByKey{});
    }
    CHECK(got.size() == want.size());
    for (size_t k = 0; k < want.size(); ++k) CHECK(same(got[k], want[k]));
  }
  return tiles;
}

constexpr uint32_t NO = kMergeNoRun;

struct WantRound {
  std::vector<MergePair> pairs;
  std::vector<MergeRun> out;
  std::vector<uint64_t> tile_off;
};

void check_round(const MergeRound& got, const WantRound& want) {
  CHECK(got.pairs.size() == want.pairs.size() && got.out.size() == want.out.size());
  for (size_t p = 0; p < want.pairs.size(); ++p) {
    CHECK(got.pairs[p].a == want.pairs[p].a && got.pairs[p].b == want.pairs[p].b);
    CHECK(got.out[p].off == want.out[p].off && got.out[p].len == want.out[p].len);
  }
  CHECK(got.tile_off == want.tile_off);
}

void check_final(const MergeFinal& f, int round, uint32_t run, uint64_t len) {
  CHECK(f.round == round && f.run == run && f.len == len);
}

// one group of the given member lengths, tiles of 4
MergePlan one_group(const std::vector<uint32_t>& lens) { return plan_merge({0, (uint32_t)lens.size()}, lens, 4); }

void check_planner() {
  {  // 1 member: no round, the member as it is
    const MergePlan P = one_group({5});
    CHECK(P.rounds.empty() && (P.dense_off == std::vector<uint64_t>{0, 5}));
    check_final(P.final_run[0], -1, 0, 5);
  }
  {  // 2 members
    const MergePlan P = one_group({3, 6});
    CHECK(P.rounds.size() == 1);
    check_round(P.rounds[0], {{{0, 1}}, {{0, 9}}, {0, 3}});
    check_final(P.final_run[0], 0, 0, 9);
  }
  {  // 3: the third is carried in round 0
    const MergePlan P = one_group({3, 6, 2});
    CHECK(P.rounds.size() == 2);
    check_round(P.rounds[0], {{{0, 1}, {2, NO}}, {{0, 9}, {9, 2}}, {0, 3, 4}});
    check_round(P.rounds[1], {{{0, 1}}, {{0, 11}}, {0, 3}});
    check_final(P.final_run[0], 1, 0, 11);
  }
  {  // 5: carried in rounds 0 and 1
    const MergePlan P = one_group({1, 2, 3, 4, 5});
    CHECK(P.rounds.size() == 3);
    check_round(P.rounds[0], {{{0, 1}, {2, 3}, {4, NO}}, {{0, 3}, {3, 7}, {10, 5}}, {0, 1, 3, 5}});
    check_round(P.rounds[1], {{{0, 1}, {2, NO}}, {{0, 10}, {10, 5}}, {0, 3, 5}});
    check_round(P.rounds[2], {{{0, 1}}, {{0, 15}}, {0, 4}});
    check_final(P.final_run[0], 2, 0, 15);
  }
  {  // 8: a power of two, nothing carried
    const MergePlan P = one_group(std::vector<uint32_t>(8, 2));
    CHECK(P.rounds.size() == 3);
    check_round(P.rounds[0],
                {{{0, 1}, {2, 3}, {4, 5}, {6, 7}}, {{0, 4}, {4, 4}, {8, 4}, {12, 4}}, {0, 1, 2, 3, 4}});
    check_round(P.rounds[1], {{{0, 1}, {2, 3}}, {{0, 8}, {8, 8}}, {0, 2, 4}});
    check_round(P.rounds[2], {{{0, 1}}, {{0, 16}}, {0, 4}});
    check_final(P.final_run[0], 2, 0, 16);
  }
  {  // 9: the ninth is carried through rounds 0, 1 and 2
    const MergePlan P = one_group(std::vector<uint32_t>(9, 1));
    CHECK(P.rounds.size() == 4);
    check_round(P.rounds[0], {{{0, 1}, {2, 3}, {4, 5}, {6, 7}, {8, NO}},
                              {{0, 2}, {2, 2}, {4, 2}, {6, 2}, {8, 1}},
                              {0, 1, 2, 3, 4, 5}});
    check_round(P.rounds[1], {{{0, 1}, {2, 3}, {4, NO}}, {{0, 4}, {4, 4}, {8, 1}}, {0, 1, 2, 3}});
    check_round(P.rounds[2], {{{0, 1}, {2, NO}}, {{0, 8}, {8, 1}}, {0, 2, 3}});
    check_round(P.rounds[3], {{{0, 1}}, {{0, 9}}, {0, 3}});
    check_final(P.final_run[0], 3, 0, 9);
  }
  {  // 33 of length 1: 33 -> 17 -> 9 -> 5 -> 3 -> 2 -> 1 runs; round r leaves 32 / 2^(r+1) runs of
     // 2^(r+1) and, in rounds 0..4, the carried run of 1 at offset 32
    const MergePlan P = one_group(std::vector<uint32_t>(33, 1));
    CHECK(P.rounds.size() == 6);
    for (uint32_t r = 0; r < 5; ++r) {
      const MergeRound& R = P.rounds[r];
      const uint32_t full = 32u >> (r + 1), len = 2u << r;
      CHECK(R.pairs.size() == full + 1);
      for (uint32_t p = 0; p < full; ++p) {
        CHECK(R.pairs[p].a == 2 * p && R.pairs[p].b == 2 * p + 1);
        CHECK(R.out[p].off == (uint64_t)p * len && R.out[p].len == len);
        CHECK(R.tile_off[p + 1] == (uint64_t)(p + 1) * ((len + 3) / 4));
      }
      CHECK(R.pairs[full].a == 2 * full && R.pairs[full].b == NO);
      CHECK(R.out[full].off == 32 && R.out[full].len == 1);
      CHECK(R.tile_off[full + 1] == R.tile_off[full] + 1);
    }
    check_round(P.rounds[4], {{{0, 1}, {2, NO}}, {{0, 32}, {32, 1}}, {0, 8, 9}});
    check_round(P.rounds[5], {{{0, 1}}, {{0, 33}}, {0, 9}});
    check_final(P.final_run[0], 5, 0, 33);
  }
  {  // several groups: a zero-length member, no members, only empty members, one member
    const MergePlan P = plan_merge({0, 3, 3, 5, 6}, {3, 0, 2, 0, 0, 4}, 4);
    CHECK((P.dense_off == std::vector<uint64_t>{0, 5, 5, 5, 9}));
    CHECK(P.rounds.size() == 2);
    check_round(P.rounds[0], {{{0, 1}, {2, NO}, {3, 4}}, {{0, 3}, {3, 2}, {5, 0}}, {0, 1, 2, 2}});
    check_round(P.rounds[1], {{{0, 1}}, {{0, 5}}, {0, 2}});
    check_final(P.final_run[0], 1, 0, 5);
    check_final(P.final_run[1], -1, NO, 0);
    check_final(P.final_run[2], 0, 2, 0);
    check_final(P.final_run[3], -1, 5, 4);
  }
  {  // the default tile
    const MergePlan P = plan_merge({0, 2}, {1024, 1});
    check_round(P.rounds[0], {{{0, 1}}, {{0, 1025}}, {0, 2}});
    CHECK(tiles_of(0, kMergeTile) == 0 && tiles_of(1024, kMergeTile) == 1);
  }
}

void check_owner() {
  const uint64_t a[] = {0, 1, 2, 2, 5};  // owner 2 has no tile
  CHECK(tile_owner(a, 4, 0) == 0 && tile_owner(a, 4, 1) == 1);
  CHECK(tile_owner(a, 4, 2) == 3 && tile_owner(a, 4, 4) == 3);
  const uint64_t b[] = {0, 0, 0, 3};  // the first owners have none
  CHECK(tile_owner(b, 3, 0) == 2 && tile_owner(b, 3, 2) == 2);
  const uint64_t c[] = {0, 7};
  CHECK(tile_owner(c, 1, 0) == 0 && tile_owner(c, 1, 6) == 0);
}

}  // namespace

int main() {
  const std::vector<std::vector<int>> arrays = sorted_arrays();
  CHECK(arrays.size() == 1 + 4 + 10 + 20 + 35 + 56);  // multisets of {0..3} of size 0..5
  uint64_t tiles = 0;
  for (const auto& a : arrays)
    for (const auto& b : arrays) tiles += check_pair(a, b);
  check_planner();
  check_owner();
  std::printf("merge plan ok: %zu x %zu pairs, %llu tiles\n", arrays.size(), arrays.size(),
              (unsigned long long)tiles);
  return 0;
}
