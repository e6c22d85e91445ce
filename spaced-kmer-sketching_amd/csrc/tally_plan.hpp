// The arithmetic of sks_sketch_set_tally (no HIP: tests/cpp/tally_plan_test.cpp
// runs it on any machine, and tally.hip runs the same functions on the device).
// After the merge rounds a group is one sorted run in which a value appears
// once per listed member that holds it; the functions here decide, from that
// run alone, which values are held by lo .. hi members, and by how many.
// Positions are 64-bit and every read lies in [0, size): what follows a group's
// run in memory (the next group, the next sketch of the source set) is never
// looked at, whatever it holds.
#pragma once
#include <cstdint>

#include "merge_plan.hpp"  // SKS_PLAN_HD

namespace sks {

constexpr uint32_t kTallyNoLimit = 0xffffffffu;  // a max_count entry: no upper limit

// The effective limits of group g from the caller's arrays (either may be null).
SKS_PLAN_HD inline uint32_t tally_lo(const uint32_t* min_count, uint32_t g) {
  const uint32_t v = min_count ? min_count[g] : 1u;
  return v < 1u ? 1u : v;
}
SKS_PLAN_HD inline uint32_t tally_hi(const uint32_t* max_count, uint32_t g) {
  return max_count ? max_count[g] : kTallyNoLimit;
}

// Does element i of the sorted run at(0 .. size) stay: it is the first of its
// value, and the value occurs at least lo and at most hi times (lo >= 1,
// i < size).  *v = at(i).  Two reads beyond the predecessor test: the value
// occurs at least lo times iff element i + lo - 1 exists and equals it, and at
// most hi times iff element i + hi does not exist or differs.  i + hi is a
// 64-bit sum, so hi == kTallyNoLimit lands at or past any size (< 2^32) and
// needs no case of its own.
template <class At, class Same, class V>
SKS_PLAN_HD inline bool tally_keeps(At at, Same same, uint64_t i, uint64_t size, uint32_t lo, uint32_t hi, V* v) {
  *v = at(i);
  if (i > 0 && same(*v, at(i - 1))) return false;
  if (hi < lo) return false;
  const uint64_t last_needed = i + lo - 1, first_banned = i + (uint64_t)hi;
  if (last_needed >= size) return false;
  if (lo > 1 && !same(at(last_needed), *v)) return false;
  return first_banned >= size || !same(at(first_banned), *v);
}

// How often the value v of a kept head i occurs (tally_keeps was true, so
// lo <= the answer <= hi), m the group's listed members, which no value
// exceeds.  The run of v ends in [i + lo, min(i + hi, i + m, size)]; "equals v"
// is true and then false over that range, so a bisection of at most
// log2(min(hi, m)) reads finds the end.
template <class At, class Same, class V>
SKS_PLAN_HD inline uint32_t tally_run_length(At at, Same same, const V& v, uint64_t i, uint64_t size, uint32_t lo,
                                             uint32_t hi, uint32_t m) {
  uint64_t a = i + lo, b = i + (uint64_t)(hi < m ? hi : m);
  if (b > size) b = size;
  while (a < b) {
    const uint64_t mid = a + (b - a) / 2;
    if (same(at(mid), v))
      a = mid + 1;
    else
      b = mid;
  }
  return (uint32_t)(a - i);
}

// ---- thresholds as the command line writes them (host) ---------------------------------
// "-": no limit.  Digits only: a count.  Digits with one decimal point ("0.9",
// "1.0", ".5"): a fraction num / den of each group's listed members, kept as
// the decimal written (den a power of ten), so 0.9 of 10 is 9 and not what a
// binary double makes of it.  At most 9 digits after the point, a value of at
// most 1.
struct TallyThreshold {
  enum Kind { kNone, kCount, kFraction } kind = kNone;
  uint32_t count = 0;
  uint64_t num = 0, den = 1;
};

// Null on success, else what is wrong with `s`.
inline const char* tally_parse_threshold(const char* s, TallyThreshold* out) {
  *out = TallyThreshold{};
  if (!s || !*s) return "empty";
  if (s[0] == '-' && !s[1]) return nullptr;
  uint64_t whole = 0, num = 0, den = 1;
  int digits = 0, after = 0;
  bool point = false;
  for (const char* p = s; *p; ++p) {
    if (*p == '.' && !point) {
      point = true;
      continue;
    }
    if (*p < '0' || *p > '9') return "neither a count, a fraction with a decimal point, nor -";
    ++digits;
    if (point) {
      if (++after > 9) return "more than 9 digits after the point";
      num = num * 10 + (uint64_t)(*p - '0');
      den *= 10;
    } else {
      whole = whole * 10 + (uint64_t)(*p - '0');
      if (whole > 0xffffffffull) return "a count above 2^32 - 1";
    }
  }
  if (digits == 0) return "no digits";
  if (!point) {
    out->kind = TallyThreshold::kCount;
    out->count = (uint32_t)whole;
    return nullptr;
  }
  if (whole > 1 || (whole == 1 && num != 0)) return "a fraction above 1";
  out->kind = TallyThreshold::kFraction;
  out->num = whole * den + num;
  out->den = den;
  return nullptr;
}

// The count a fraction num / den (<= 1) of m listed members stands for:
// ceil(f * m), at least 1, as a minimum; floor(f * m) as a maximum.
inline uint32_t tally_fraction_min(uint64_t num, uint64_t den, uint32_t m) {
  const uint64_t v = (num * m + den - 1) / den;
  return v < 1 ? 1u : (uint32_t)v;
}
inline uint32_t tally_fraction_max(uint64_t num, uint64_t den, uint32_t m) { return (uint32_t)(num * m / den); }

// A threshold as group g's min_count / max_count entry (m listed members).
inline uint32_t tally_min_of(const TallyThreshold& t, uint32_t m) {
  if (t.kind == TallyThreshold::kNone) return 1;
  return t.kind == TallyThreshold::kCount ? t.count : tally_fraction_min(t.num, t.den, m);
}
inline uint32_t tally_max_of(const TallyThreshold& t, uint32_t m) {
  if (t.kind == TallyThreshold::kNone) return kTallyNoLimit;
  return t.kind == TallyThreshold::kCount ? t.count : tally_fraction_max(t.num, t.den, m);
}

}  // namespace sks
