// The arithmetic of sks_sketch_set_filter (csrc/filter_plan.hpp) on the CPU: no
// HIP, no libsks.  The bracket of a chunk (the one-lane search and the 64-ary
// narrowing a wavefront runs, replayed lane by lane) against std::lower_bound /
// std::upper_bound on 64- and 128-bit arrays, and a replay of the mark and
// scatter passes built from the plan functions against std::set_difference /
// std::set_intersection.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <random>
#include <utility>
#include <vector>

#include "filter_plan.hpp"

using namespace sks;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

namespace {

// (hi, lo): std::pair's order is the elements' 128-bit order
using Val = std::pair<uint64_t, uint64_t>;

template <int EW>
std::vector<uint64_t> words_of(const std::vector<Val>& v) {
  std::vector<uint64_t> w;
  for (const Val& x : v) {
    w.push_back(x.second);
    if (EW == 2) w.push_back(x.first);
  }
  w.push_back(0);  // never empty
  return w;
}

// Ascending unique values.  Narrow: hi == 0.  Wide: few distinct hi and few
// distinct lo words, so many elements share hi and differ in lo and the reverse.
template <int EW>
std::vector<Val> random_values(std::mt19937_64& rng, size_t n, uint64_t span) {
  std::vector<Val> v;
  while (v.size() < n) {
    for (size_t i = v.size(); i < n; ++i) v.push_back({EW == 2 ? rng() % 7 : 0, rng() % span});
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
  }
  return v;
}

// one end of the bracket as a wavefront finds it: 64 probes a step
template <int EW, bool UPPER>
uint32_t wave_bound(const uint64_t* f, uint32_t n, Val v, int* steps) {
  FilterRange r{0u, n};
  for (*steps = 1;; ++*steps) {
    uint32_t n_true = 0;
    bool seen_false = false;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t i = filter_probe(r, lane);
      CHECK(i >= r.lo && i <= r.hi && r.hi <= n);
      bool t = false;
      if (i < r.hi) {
        const uint64_t* e = f + (size_t)i * EW;
        t = UPPER ? filter_not_above<EW>(e, v.second, v.first) : filter_below<EW>(e, v.second, v.first);
      }
      CHECK(!(t && seen_false));  // monotone: the ballot is a run of low lanes
      seen_false = seen_false || !t;
      n_true += t ? 1u : 0u;
    }
    bool done = false;
    const uint32_t before = r.hi - r.lo;
    r = filter_narrow(r, n_true, &done);
    CHECK(r.lo <= r.hi && r.hi <= n);
    if (done) return r.lo;
    CHECK(r.hi - r.lo < before && (uint64_t)(r.hi - r.lo) * 65 <= before + 65);
  }
}

template <int EW>
void check_bracket(const std::vector<Val>& filt, Val first, Val last) {
  const std::vector<uint64_t> w = words_of<EW>(filt);
  const uint32_t n = (uint32_t)filt.size();
  const uint32_t lb = (uint32_t)(std::lower_bound(filt.begin(), filt.end(), first) - filt.begin());
  const uint32_t ub = (uint32_t)(std::upper_bound(filt.begin(), filt.end(), last) - filt.begin());
  const FilterRange r = filter_bracket<EW>(w.data(), n, first.second, first.first, last.second, last.first);
  CHECK(r.lo == lb && r.hi == ub);
  int s0, s1;
  CHECK((wave_bound<EW, false>(w.data(), n, first, &s0)) == lb);
  CHECK((wave_bound<EW, true>(w.data(), n, last, &s1)) == ub);
  // 64 probes a step: 1 step up to 64 elements, 2 up to 65 * 65 - 1, ...
  int most = 1;
  for (uint64_t reach = 64; reach < n; reach = reach * 65 + 64) ++most;
  CHECK(s0 <= most && s1 <= most);
}

template <int EW>
void test_brackets(std::mt19937_64& rng) {
  for (size_t n : {0, 1, 2, 63, 64, 65, 66, 127, 128, 129, 1000, 4224, 4225, 4226, 70000}) {
    for (int rep = 0; rep < (n > 10000 ? 3 : 20); ++rep) {
      const uint64_t span = n < 100 ? 300 : 4 * n;
      const std::vector<Val> filt = random_values<EW>(rng, n, span);
      // chunk ends drawn from the same small space: often equal to filter elements
      for (int t = 0; t < 40; ++t) {
        Val a{EW == 2 ? rng() % 7 : 0, rng() % span}, b{EW == 2 ? rng() % 7 : 0, rng() % span};
        if (b < a) std::swap(a, b);
        if (t % 4 == 1 && n) a = filt[rng() % n];  // a duplicate of a filter element at either end
        if (t % 4 == 2 && n) b = filt[rng() % n];
        if (t % 4 == 3 && n) a = b = filt[rng() % n];
        if (b < a) std::swap(a, b);
        check_bracket<EW>(filt, a, b);
      }
      // all filter elements below the chunk, all above it, and the chunk around all of them
      const Val top{EW == 2 ? 100 : 0, ~0ull}, bottom{0, 0};
      check_bracket<EW>(filt, top, top);
      if (n && filt[0] > bottom) check_bracket<EW>(filt, bottom, bottom);
      check_bracket<EW>(filt, bottom, top);
      if (EW == 2 && n) {
        // the same lo, another hi; the same hi, another lo
        const Val x = filt[rng() % n];
        check_bracket<EW>(filt, {x.first, x.second}, {x.first + 1, x.second});
        check_bracket<EW>(filt, {x.first, 0}, {x.first, x.second});
      }
    }
  }
}

// mark + scatter of one source sketch against one filter sketch, as the kernels
// do it: chunks of kFilterChunk, strides of 256 threads, ballots of 64 lanes.
template <int EW>
std::vector<Val> replay(const std::vector<Val>& src, const std::vector<Val>& filt, int kind, bool no_stage,
                        bool copies, int* staged_chunks, int* direct_chunks) {
  const std::vector<uint64_t> fw = words_of<EW>(filt);
  const uint64_t n_chunks = (src.size() + kFilterChunk - 1) / kFilterChunk;
  std::vector<uint64_t> bitmap(filter_bitmap_words(n_chunks) + 1, ~0ull);
  std::vector<uint32_t> counts(n_chunks + 1, 0);
  for (uint64_t c = 0; c < n_chunks; ++c) {
    const size_t base = c * kFilterChunk;
    const uint32_t len = (uint32_t)std::min<size_t>(kFilterChunk, src.size() - base);
    FilterRange r{0, 0};
    if (!copies && !filt.empty())
      r = filter_bracket<EW>(fw.data(), (uint32_t)filt.size(), src[base].second, src[base].first,
                             src[base + len - 1].second, src[base + len - 1].first);
    std::vector<uint64_t> stage;
    const bool staged = r.hi != r.lo && filter_staged(r.hi - r.lo, EW, no_stage);
    if (staged) {
      CHECK((r.hi - r.lo) * 8u * EW <= kFilterStageBytes);
      stage.assign(fw.begin() + (size_t)r.lo * EW, fw.begin() + (size_t)r.hi * EW);
      ++*staged_chunks;
    } else if (r.hi != r.lo) {
      ++*direct_chunks;
    }
    for (uint32_t stride = 0; stride < kFilterChunk / 256; ++stride)
      for (uint32_t wave = 0; wave < 4; ++wave) {
        uint64_t ballot = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint32_t e = stride * 256 + wave * 64 + lane;
          if (e >= len) continue;
          const Val v = src[base + e];
          bool found = false;
          if (staged) found = filter_member<EW>(stage.data(), 0, r.hi - r.lo, v.second, v.first);
          else if (r.hi != r.lo) found = filter_member<EW>(fw.data(), r.lo, r.hi, v.second, v.first);
          if (copies || filter_keeps(found, kind)) ballot |= 1ull << lane;
          CHECK(filter_word_of(e) == filter_ballot_word(stride, wave) && filter_bit_of(e) == lane);
        }
        bitmap[c * kFilterChunkWords + filter_ballot_word(stride, wave)] = ballot;
        counts[c] += (uint32_t)__builtin_popcountll(ballot);
      }
  }
  std::vector<uint64_t> offs(n_chunks + 1, 0);
  for (uint64_t c = 0; c < n_chunks; ++c) offs[c + 1] = offs[c] + counts[c];
  std::vector<Val> out(offs[n_chunks], Val{~0ull, ~0ull});
  for (uint64_t c = 0; c < n_chunks; ++c) {
    uint32_t run = 0;
    for (uint32_t word = 0; word < kFilterChunkWords; ++word) {
      const uint64_t bits = bitmap[c * kFilterChunkWords + word];
      for (uint32_t lane = 0; lane < 64; ++lane)
        if ((bits >> lane) & 1) {
          const uint32_t rank = run + (uint32_t)__builtin_popcountll(bits & ((1ull << lane) - 1));
          CHECK(word * 64 + lane < src.size() - c * kFilterChunk);  // the tail's bits are zero
          out[offs[c] + rank] = src[c * kFilterChunk + word * 64 + lane];
        }
      run += (uint32_t)__builtin_popcountll(bits);
    }
    CHECK(run == counts[c]);
  }
  return out;
}

template <int EW>
void test_replay(std::mt19937_64& rng) {
  int staged = 0, direct = 0;
  for (size_t n : {0, 1, 255, 256, 257, 1023, 1024, 1025, 2049}) {
    // a filter about as dense as the source (short brackets), one 40 times denser
    // (brackets past the stage), a sparse one, an empty one and the source itself
    for (int shape = 0; shape < 5; ++shape) {
      const uint64_t span = 8 * std::max<size_t>(n, 16);
      const std::vector<Val> src = random_values<EW>(rng, n, span);
      std::vector<Val> filt;
      if (shape == 0) filt = random_values<EW>(rng, n, span);
      if (shape == 1) filt = random_values<EW>(rng, EW == 2 ? std::min<size_t>(40 * n, 5 * span) : 5 * n, span);
      if (shape == 2) filt = random_values<EW>(rng, n / 100, span);
      if (shape == 4) filt = src;
      for (int kind : {kFilterSubtract, kFilterIntersect})
        for (bool no_stage : {false, true}) {
          std::vector<Val> want;
          if (kind == kFilterSubtract)
            std::set_difference(src.begin(), src.end(), filt.begin(), filt.end(), std::back_inserter(want));
          else
            std::set_intersection(src.begin(), src.end(), filt.begin(), filt.end(), std::back_inserter(want));
          int s = 0, d = 0;
          CHECK(replay<EW>(src, filt, kind, no_stage, false, &s, &d) == want);
          CHECK(!no_stage || s == 0);
          staged += s, direct += no_stage ? 0 : d;
          CHECK(replay<EW>(src, filt, kind, no_stage, true, &s, &d) == src);  // no filter: a copy
        }
    }
  }
  CHECK(staged > 0 && direct > 0);  // both paths were taken by choice
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240607);
  CHECK(filter_keeps(true, kFilterIntersect) && !filter_keeps(false, kFilterIntersect));
  CHECK(!filter_keeps(true, kFilterSubtract) && filter_keeps(false, kFilterSubtract));
  CHECK(filter_stage_elems(1) == 2 * filter_stage_elems(2) && filter_stage_elems(2) * 16 == kFilterStageBytes);
  CHECK(filter_staged(filter_stage_elems(1), 1, false) && !filter_staged(filter_stage_elems(1) + 1, 1, false));
  CHECK(filter_staged(filter_stage_elems(2), 2, false) && !filter_staged(filter_stage_elems(2) + 1, 2, false));
  CHECK(!filter_staged(1, 1, true) && kFilterChunkWords == 16 && filter_bitmap_words(3) == 48);
  for (uint32_t e = 0; e < kFilterChunk; ++e) CHECK(filter_word_of(e) * 64 + filter_bit_of(e) == e);
  test_brackets<1>(rng);
  test_brackets<2>(rng);
  test_replay<1>(rng);
  test_replay<2>(rng);
  std::printf("filter plan ok\n");
  return 0;
}
