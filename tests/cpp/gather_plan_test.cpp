// CPU check of csrc/gather_plan.hpp (no HIP, no libsks): the round's key orders
// candidates as a sort by (-count, index) does; the bitmap's tail mask for every
// size from 1 to 130; the bounded search against std::lower_bound on 64- and
// 128-bit arrays, with targets below, above and equal to the first and last
// element; how a candidate's list chunks map to scoring workgroups and how many
// of them arrive; and the round-group plan.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "gather_plan.hpp"

using namespace sks;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

namespace {

void check_keys() {
  std::mt19937_64 rng(11);
  std::vector<std::pair<int32_t, uint32_t>> c;  // (count, ref)
  const int32_t counts[] = {0, 1, 2, 7, 1000, 0x7ffffffe, 0x7fffffff};
  const uint32_t refs[] = {0u, 1u, 2u, 63u, 64u, 0x7fffffffu, 0x80000000u, 0xfffffffdu, 0xffffffffu - 1u};
  for (int32_t n : counts)
    for (uint32_t r : refs) c.emplace_back(n, r);
  for (int i = 0; i < 2000; ++i) c.emplace_back((int32_t)(rng() & 0x7fffffff), (uint32_t)(rng() % 0xffffffffull));
  for (const auto& x : c) {
    const unsigned long long k = gather_key(x.first, x.second);
    CHECK(gather_key_count(k) == x.first);
    CHECK(gather_key_ref(k) == x.second);
    CHECK(x.first == 0 || k != 0);  // 0 is "nothing posted"
  }
  // descending key == ascending (-count, index)
  std::vector<std::pair<int32_t, uint32_t>> by_rule = c, by_key = c;
  std::sort(by_rule.begin(), by_rule.end(), [](const auto& a, const auto& b) {
    return a.first != b.first ? a.first > b.first : a.second < b.second;
  });
  std::sort(by_key.begin(), by_key.end(), [](const auto& a, const auto& b) {
    return gather_key(a.first, a.second) > gather_key(b.first, b.second);
  });
  by_rule.erase(std::unique(by_rule.begin(), by_rule.end()), by_rule.end());
  by_key.erase(std::unique(by_key.begin(), by_key.end()), by_key.end());
  CHECK(by_rule == by_key);
  CHECK(gather_key(5, 3) > gather_key(5, 4) && gather_key(6, 4) > gather_key(5, 3));
  CHECK(gather_threshold(-4) == 1 && gather_threshold(0) == 1 && gather_threshold(1) == 1 &&
        gather_threshold(9) == 9);
}

void check_bitmap() {
  for (uint32_t n = 1; n <= 130; ++n) {
    const uint32_t words = gather_bitmap_words(n);
    CHECK(words == (n + 31) / 32 && words >= 1);
    std::vector<uint32_t> bm(words);
    for (uint32_t w = 0; w < words; ++w) bm[w] = gather_word_init(w, n);
    uint32_t set = 0;
    for (uint32_t p = 0; p < words * 32; ++p) {
      CHECK(gather_word_of(p) < words);
      const bool on = (bm[gather_word_of(p)] & gather_bit_of(p)) != 0;
      CHECK(on == (p < n));  // every element's bit, and no tail bit
      set += on;
    }
    CHECK(set == n);
    // clearing an element clears that element only
    for (uint32_t p = 0; p < n; ++p) {
      std::vector<uint32_t> b = bm;
      b[gather_word_of(p)] &= ~gather_bit_of(p);
      uint32_t left = 0;
      for (uint32_t w : b) left += (uint32_t)__builtin_popcount(w);
      CHECK(left == n - 1 && !(b[gather_word_of(p)] & gather_bit_of(p)));
    }
  }
  CHECK(gather_bitmap_words(0) == 0);
}

struct Wide {
  uint64_t lo, hi;
  bool operator<(const Wide& o) const { return hi != o.hi ? hi < o.hi : lo < o.lo; }
  bool operator==(const Wide& o) const { return lo == o.lo && hi == o.hi; }
};

template <int EW>
void check_search_on(const std::vector<Wide>& q, const std::vector<Wide>& targets, std::mt19937_64& rng) {
  std::vector<uint64_t> words;
  for (const Wide& e : q) {
    words.push_back(e.lo);
    if (EW == 2) words.push_back(e.hi);
  }
  const uint32_t n = (uint32_t)q.size();
  for (const Wide& t : targets) {
    const uint32_t want = (uint32_t)(std::lower_bound(q.begin(), q.end(), t) - q.begin());
    CHECK(gather_lower_bound<EW>(words.data(), 0, n, t.lo, t.hi) == want);
    if (want < n) CHECK(gather_equal<EW>(words.data() + (size_t)want * EW, t.lo, t.hi) == (q[want] == t));
    // restricted to ranges: the result is lower_bound clamped into [lo, hi]
    for (int rep = 0; rep < 8; ++rep) {
      uint32_t lo = (uint32_t)(rng() % (n + 1)), hi = (uint32_t)(rng() % (n + 1));
      if (lo > hi) std::swap(lo, hi);
      const uint32_t got = gather_lower_bound<EW>(words.data(), lo, hi, t.lo, t.hi);
      CHECK(got == std::min(std::max(want, lo), hi));
    }
    CHECK(gather_lower_bound<EW>(words.data(), want, want, t.lo, t.hi) == want);  // an empty range
  }
}

void check_search() {
  std::mt19937_64 rng(23);
  for (int round = 0; round < 40; ++round) {
    const uint32_t n = 1 + (uint32_t)(rng() % 300);
    // 64-bit: random values
    std::vector<Wide> q;
    for (uint32_t i = 0; i < n; ++i) q.push_back({rng() | 1ull, 0});  // never 0, so a target below exists
    std::sort(q.begin(), q.end());
    q.erase(std::unique(q.begin(), q.end()), q.end());
    if (q.back().lo == ~0ull) q.pop_back();
    if (q.empty()) continue;
    std::vector<Wide> t{{0, 0}, {~0ull, 0}, q.front(), q.back(), {q.front().lo - 1, 0}, {q.back().lo + 1, 0}};
    for (int i = 0; i < 60; ++i) t.push_back(i & 1 ? q[rng() % q.size()] : Wide{rng(), 0});
    check_search_on<1>(q, t, rng);
    // 128-bit: few distinct lo and hi values, so many pairs share lo and differ
    // in hi, and the reverse; lo's order alone would misplace them
    std::vector<Wide> p;
    const uint64_t lo_pool[] = {1, 5, 1ull << 40, ~0ull - 3, rng(), rng()};
    const uint64_t hi_pool[] = {0, 1, 2, 1ull << 63, rng(), rng()};
    for (uint32_t i = 0; i < n; ++i) p.push_back({lo_pool[rng() % 6], hi_pool[rng() % 6]});
    for (uint32_t i = 0; i < n / 4; ++i) p.push_back({rng(), rng()});
    std::sort(p.begin(), p.end());
    p.erase(std::unique(p.begin(), p.end()), p.end());
    std::vector<Wide> u{{0, 0}, {~0ull, ~0ull}, p.front(), p.back()};
    u.push_back({p.front().lo, p.front().hi + 1});  // equal lo, different hi
    u.push_back({p.back().lo + 1, p.back().hi});    // equal hi, different lo
    u.push_back({p.back().lo, p.back().hi - 1});
    for (int i = 0; i < 80; ++i) {
      const Wide a = p[rng() % p.size()], b = p[rng() % p.size()];
      u.push_back(a);
      u.push_back({a.lo, b.hi});
      u.push_back({b.lo, a.hi});
    }
    check_search_on<2>(p, u, rng);
  }
}

void check_waves() {
  // every chunk of every candidate's list is scored by exactly one workgroup, and
  // the workgroups with a chunk are the gather_blocks_of that the last arrival counts
  std::mt19937_64 rng(37);
  for (int round = 0; round < 200; ++round) {
    const uint32_t n = 1 + (uint32_t)(rng() % 9);
    std::vector<uint32_t> len(n);
    uint32_t longest = 0;
    for (uint32_t& l : len) {
      const uint32_t pick = (uint32_t)(rng() % 4);
      l = pick == 0 ? 1 + (uint32_t)(rng() % 5) : pick == 1 ? kGatherChunk * (1 + (uint32_t)(rng() % 3))
                                                            : 1 + (uint32_t)(rng() % (9 * kGatherChunk));
      longest = std::max(longest, l);
    }
    uint32_t per = gather_blocks_per_candidate(longest, n);
    CHECK(per == gather_chunks_of(longest));
    if (round & 1) per = 1 + (uint32_t)(rng() % per);  // as a capped grid would have it
    std::vector<std::vector<int>> seen(n);
    std::vector<uint32_t> arrivals(n, 0);
    for (uint32_t c = 0; c < n; ++c) seen[c].assign(gather_chunks_of(len[c]), 0);
    for (uint32_t b = 0; b < n * per; ++b) {
      const uint32_t c = gather_candidate_of(b, per), first = gather_first_chunk_of(b, per);
      CHECK(c < n && first < per);
      if (first >= gather_blocks_of(len[c], per)) continue;
      ++arrivals[c];
      for (uint64_t chunk = first; chunk * kGatherChunk < len[c]; chunk += per) ++seen[c][chunk];
    }
    for (uint32_t c = 0; c < n; ++c) {
      CHECK(arrivals[c] == gather_blocks_of(len[c], per) && arrivals[c] >= 1);
      for (int s : seen[c]) CHECK(s == 1);
    }
  }
  CHECK(gather_chunks_of(0) == 0 && gather_chunks_of(1) == 1 && gather_chunks_of(kGatherChunk) == 1 &&
        gather_chunks_of(kGatherChunk + 1) == 2);
  CHECK(gather_blocks_per_candidate(0, 5) == 1);
  // the grid stays within 2^30 workgroups
  CHECK((uint64_t)gather_blocks_per_candidate(0x7fffffffu, 3000) * 3000 <= (1ull << 30));
  CHECK(gather_blocks_per_candidate(0x7fffffffu, 1u << 30) == 1);
  // an arrival word: tickets above, counts below, no carry between them for counts that add up below 2^32
  unsigned long long word = 0;
  for (uint32_t count : {0u, 5u, 0x7ffffff0u, 10u}) word += gather_arrival(count);
  CHECK((uint32_t)(word >> 32) == 4 && (uint32_t)word == 0x7fffffffu);
}

void check_groups() {
  CHECK(gather_round_limit(10, 0) == 11 && gather_round_limit(10, 3) == 4 && gather_round_limit(10, 10) == 11 &&
        gather_round_limit(10, 50) == 11 && gather_round_limit(1, 0) == 2);
  CHECK(gather_round_limit(0x7fffffffu, 0) == 0x80000000ull);
  const uint32_t sizes[] = {0, 1, 2, 3, 7, 16, 1000};
  for (uint32_t per_wait : sizes)
    for (uint64_t limit = 1; limit <= 70; ++limit) {
      const uint32_t g = per_wait ? per_wait : kGatherDefaultRounds;
      uint64_t queued = 0, groups = 0;
      while (queued < limit) {
        const uint32_t n = gather_group_rounds(per_wait, queued, limit);
        CHECK(n >= 1 && n <= g && queued + n <= limit);
        CHECK(n == g || queued + n == limit);  // only the last group is short
        queued += n;
        ++groups;
      }
      CHECK(queued == limit && groups == (limit + g - 1) / g);
      CHECK(gather_group_rounds(per_wait, limit, limit) == 0 && gather_group_rounds(per_wait, limit + 5, limit) == 0);
    }
  CHECK(kGatherDefaultRounds >= 1);
}

}  // namespace

int main() {
  check_keys();
  check_bitmap();
  check_search();
  check_waves();
  check_groups();
  std::printf("gather plan ok\n");
  return 0;
}
