// CPU check of csrc/topk_plan.hpp (no HIP, no libsks): the order is strict and
// total; the denominators, the score and eligibility; and the list update, fed
// the candidates of random inputs dense with ties in several orders and cut into
// several batches, ends for every k in 1..64 as the first k of std::sort of all
// eligible candidates, empty slots after them.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "topk_plan.hpp"

using namespace sks;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

namespace {

bool same(const TopkSlot& a, const TopkSlot& b) {
  return std::memcmp(&a.score, &b.score, sizeof(double)) == 0 && a.shared == b.shared && a.ref == b.ref;
}

void check_order() {
  // equal scores from different fractions, equal shared, neighbouring refs
  std::vector<TopkSlot> s;
  const int32_t fr[][2] = {{5, 10}, {10, 20}, {1, 2}, {1, 3}, {2, 6}, {7, 7}, {3, 3}, {1, 1000000}, {999, 1000}};
  const uint32_t refs[] = {0u, 1u, 63u, 64u, 0x7fffffffu, 0xfffffffeu};
  for (const auto& f : fr)
    for (uint32_t r : refs) s.push_back(TopkSlot{topk_score(f[0], f[1]), f[0], r});
  s.push_back(topk_empty());
  for (const TopkSlot& a : s) {
    CHECK(!topk_better(a, a));
    for (const TopkSlot& b : s) {
      const bool ab = topk_better(a, b), ba = topk_better(b, a);
      CHECK(!(ab && ba));                 // asymmetric
      CHECK(ab || ba || same(a, b));      // total over distinct slots
      for (const TopkSlot& c : s)
        if (ab && topk_better(b, c)) CHECK(topk_better(a, c));  // transitive
    }
    if (!topk_is_empty(a)) CHECK(topk_better(a, topk_empty()));  // empty is after every candidate
  }
  // the rule, field by field
  CHECK(topk_score(5, 10) == topk_score(10, 20));
  CHECK(topk_better(TopkSlot{0.5, 10, 9}, TopkSlot{0.5, 5, 3}));   // equal score: the larger shared
  CHECK(topk_better(TopkSlot{0.5, 5, 3}, TopkSlot{0.5, 5, 4}));    // then the smaller ref
  CHECK(topk_better(TopkSlot{0.6, 1, 9}, TopkSlot{0.5, 50, 0}));   // score first
  CHECK(topk_is_empty(topk_empty()) && !topk_is_empty(TopkSlot{0.0, 0, 0}));
}

void check_score() {
  CHECK(topk_denominator(kRankQuery, 10, 20) == 10 && topk_denominator(kRankQuery, 20, 10) == 20);
  CHECK(topk_denominator(kRankRef, 10, 20) == 20 && topk_denominator(kRankRef, 20, 10) == 10);
  CHECK(topk_denominator(kRankMax, 10, 20) == 10 && topk_denominator(kRankMax, 20, 10) == 10 &&
        topk_denominator(kRankMax, 7, 7) == 7);
  CHECK(topk_score(0, 0) == 0.0 && topk_score(0, 5) == 0.0 && topk_score(3, 3) == 1.0);
  CHECK(topk_score(1, 3) == 1.0 / 3.0 && topk_score(0x7fffffff, 0x7fffffff) == 1.0);
  CHECK(topk_threshold(-3) == 1 && topk_threshold(0) == 1 && topk_threshold(1) == 1 && topk_threshold(8) == 8);
  const TopkSlot c{0.25, 4, 17};
  CHECK(topk_eligible(c, 17, 1, 0.25, false) && !topk_eligible(c, 17, 1, 0.25, true) &&
        topk_eligible(c, 16, 1, 0.25, true));
  CHECK(!topk_eligible(c, 0, 5, 0.0, false) && topk_eligible(c, 0, 4, 0.0, false));
  CHECK(!topk_eligible(c, 0, 1, 0.2500001, false) && topk_eligible(c, 0, 1, -1.0, false));
}

// all candidates of one query, the model fed in `order`, cut into batches of
// `cut` (the list leaves and re-enters "scratch" between batches)
void run_model(const std::vector<TopkSlot>& cand, const std::vector<uint32_t>& order, size_t cut, uint32_t k,
               std::vector<TopkSlot>* out) {
  std::vector<TopkSlot> scratch(k, topk_empty());
  for (size_t b0 = 0; b0 < order.size(); b0 += cut) {
    TopkSlot list[kTopkMax];
    std::copy(scratch.begin(), scratch.end(), list);
    for (size_t i = b0; i < std::min(order.size(), b0 + cut); ++i) topk_list_update(list, k, cand[order[i]]);
    std::copy(list, list + k, scratch.begin());
  }
  *out = scratch;
}

void check_lists() {
  std::mt19937_64 rng(41);
  for (int round = 0; round < 10; ++round) {
    // few distinct sizes and counts: many equal scores (5/10 and 10/20), equal
    // (score, shared) with different refs, and duplicate candidates
    const uint32_t n = round < 4 ? (uint32_t)round : 1 + (uint32_t)(rng() % 120);
    const int32_t sizes[] = {10, 20, 40, 30, 60};
    std::vector<TopkSlot> cand;
    for (uint32_t i = 0; i < n; ++i) {
      const int32_t den = sizes[rng() % 5];
      const int32_t shared = 1 + (int32_t)(rng() % 4) * (den / 10) * 2;  // multiples that reduce to the same fractions
      cand.push_back(TopkSlot{topk_score(shared > den ? den : shared, den), shared > den ? den : shared,
                              (uint32_t)(rng() % (round & 1 ? 50 : 5000))});
      if (rng() % 7 == 0) cand.push_back(cand.back());                        // a duplicate
      if (rng() % 5 == 0) cand.push_back(TopkSlot{cand.back().score, cand.back().shared, cand.back().ref + 1});
    }
    std::vector<TopkSlot> sorted = cand;
    std::sort(sorted.begin(), sorted.end(), topk_better);
    std::vector<std::vector<uint32_t>> orders(4, std::vector<uint32_t>(cand.size()));
    for (auto& o : orders)
      for (uint32_t i = 0; i < o.size(); ++i) o[i] = i;
    std::reverse(orders[1].begin(), orders[1].end());
    std::shuffle(orders[2].begin(), orders[2].end(), rng);
    std::sort(orders[3].begin(), orders[3].end(),
              [&](uint32_t a, uint32_t b) { return topk_better(cand[b], cand[a]); });  // worst first: every one enters
    for (uint32_t k = 1; k <= kTopkMax; ++k)
      for (const auto& order : orders)
        for (size_t cut : {(size_t)1, (size_t)7, cand.size() + 1}) {
          std::vector<TopkSlot> got;
          run_model(cand, order, cut, k, &got);
          CHECK(got.size() == k);
          for (uint32_t j = 0; j < k; ++j) {
            if (j < sorted.size()) CHECK(same(got[j], sorted[j]));
            else CHECK(topk_is_empty(got[j]) && same(got[j], topk_empty()));
          }
        }
  }
}

// the lane form: every lane's new value from its own and the one before it
void check_lanes() {
  TopkSlot list[4] = {{0.9, 9, 1}, {0.5, 5, 2}, {0.5, 5, 7}, topk_empty()};
  const TopkSlot c{0.5, 5, 4};
  uint32_t p = 0;
  for (const TopkSlot& s : list) p += topk_better(c, s) ? 0u : 1u;
  CHECK(p == 2);
  TopkSlot next[4];
  for (uint32_t l = 0; l < 4; ++l) next[l] = topk_lane_after(list[l], list[l ? l - 1 : 0], c, l, p);
  CHECK(same(next[0], list[0]) && same(next[1], list[1]) && same(next[2], c) && same(next[3], list[2]));
  topk_list_update(list, 4, c);
  for (uint32_t l = 0; l < 4; ++l) CHECK(same(list[l], next[l]));
  // a full list drops its last slot; a candidate that is not before it changes nothing
  topk_list_update(list, 4, TopkSlot{0.5, 5, 9});
  CHECK(list[2].ref == 4 && list[3].ref == 7);
  topk_list_update(list, 4, TopkSlot{0.95, 1, 3});
  CHECK(list[0].ref == 3 && list[1].ref == 1 && list[2].ref == 2 && list[3].ref == 4);
}

}  // namespace

int main() {
  check_order();
  check_score();
  check_lists();
  check_lanes();
  std::printf("topk plan ok\n");
  return 0;
}
