// CPU check of csrc/set_rules.hpp (no HIP, no libsks): the first differing field
// of two sets under both param rules and in both argument orders, the number of
// positions a mask selects, and the one retry after an invalid layout, with a
// fake core that records its calls.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "set_rules.hpp"
#include "sks.h"

using namespace sks;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

namespace {

bool is(const char* got, const char* want) {
  return want ? (got && std::strcmp(got, want) == 0) : got == nullptr;
}

// both argument orders give `want`
void expect(const sks_sketch_info& a, const sks_sketch_info& b, ParamRule rule, const char* want) {
  CHECK(is(set_differs_in(a, b, rule), want));
  CHECK(is(set_differs_in(b, a, rule), want));
}

sks_sketch_info base_info(int32_t kind) {
  sks_sketch_info i{};
  i.window = 31;
  i.elem_words = 1;
  i.mask[0] = 0x3ffffffffffull;
  i.mask[1] = 0;
  i.policy = sks_policy{kind, SKS_HASH_BOOST_MIX, 50, 1};
  i.n = 7;
  i.has_names = 0;
  return i;
}

struct Field {
  const char* name;
  std::function<void(sks_sketch_info&)> perturb;
};

// in the documented order
const std::vector<Field>& fields() {
  static const std::vector<Field> f = {
      {"window", [](sks_sketch_info& i) { i.window += 1; }},
      {"mask", [](sks_sketch_info& i) { i.mask[0] ^= 4; }},
      {"elem_words", [](sks_sketch_info& i) { i.elem_words = 2; }},
      {"policy kind", [](sks_sketch_info& i) { i.policy.kind ^= 1; }},
      {"hash flavour", [](sks_sketch_info& i) { i.policy.flavour ^= 1; }},
      {"nonce", [](sks_sketch_info& i) { i.policy.nonce += 1; }},
      {"policy param (FracMinHash c)", [](sks_sketch_info& i) { i.policy.param += 10; }},
  };
  return f;
}

void check_differs() {
  const sks_sketch_info frac = base_info(SKS_FRAC_MOD), bottom = base_info(SKS_BOTTOM_S);
  for (ParamRule rule : {ParamRule::kFracOnly, ParamRule::kAlways}) {
    expect(frac, frac, rule, nullptr);
    expect(bottom, bottom, rule, nullptr);
    // what a set holds is no part of how it was made
    sks_sketch_info other = frac;
    other.n = 9;
    other.has_names = 1;
    expect(frac, other, rule, nullptr);
    // one field at a time
    for (const Field& f : fields()) {
      sks_sketch_info b = frac;
      f.perturb(b);
      expect(frac, b, rule, f.name);
    }
    // the mask's high word alone
    sks_sketch_info hi = frac;
    hi.mask[1] = 1;
    expect(frac, hi, rule, "mask");
    // two fields: the earlier one in the documented order
    for (size_t x = 0; x < fields().size(); ++x)
      for (size_t y = x + 1; y < fields().size(); ++y) {
        sks_sketch_info b = frac;
        fields()[y].perturb(b);
        fields()[x].perturb(b);
        expect(frac, b, rule, fields()[x].name);
      }
  }
  // bottom-s of another s: comparable, but not one set
  sks_sketch_info s2 = bottom;
  s2.policy.param = 40;
  expect(bottom, s2, ParamRule::kFracOnly, nullptr);
  expect(bottom, s2, ParamRule::kAlways, "policy param (FracMinHash c)");
  // every other field of bottom-s sets is checked under both rules
  for (ParamRule rule : {ParamRule::kFracOnly, ParamRule::kAlways})
    for (size_t x = 0; x + 1 < fields().size(); ++x) {
      sks_sketch_info b = s2;
      fields()[x].perturb(b);
      expect(bottom, b, rule, fields()[x].name);
    }
}

void check_ones() {
  const uint64_t none[2] = {0, 0};
  CHECK(kmer_ones_of(none) == 0);
  const uint64_t one_pos[2] = {3, 0};
  CHECK(kmer_ones_of(one_pos) == 1);
  const uint64_t narrow[2] = {0x3ffffffffffull, 0};  // 21 positions
  CHECK(kmer_ones_of(narrow) == 21);
  const uint64_t full64[2] = {~0ull, 0};
  CHECK(kmer_ones_of(full64) == 32);
  const uint64_t wide[2] = {~0ull, 0xfff0ull};  // 32 + 6 positions
  CHECK(kmer_ones_of(wide) == 38);
  const uint64_t full128[2] = {~0ull, ~0ull};
  CHECK(kmer_ones_of(full128) == 64);
  const uint64_t high_only[2] = {0, 0xfull << 60};
  CHECK(kmer_ones_of(high_only) == 2);
}

struct Call {
  const std::vector<uint64_t>* bounds;
  bool has_flag;
};

void check_retry() {
  const std::vector<uint64_t> mask_bounds = {1, 2, 3};
  std::vector<Call> calls;
  // what the fake core does on its i-th call: {status, raises the flag}
  struct Step {
    int rc;
    bool invalid;
  };
  auto run = [&](std::vector<Step> steps) {
    calls.clear();
    return with_mask_bounds_retry(mask_bounds, [&](const std::vector<uint64_t>* h_bounds, bool* invalid) {
      const Step s = steps.at(calls.size());
      calls.push_back({h_bounds, invalid != nullptr});
      if (s.invalid && invalid) *invalid = true;
      return s.rc;
    });
  };
  // a success: one call, with the mask's bounds
  CHECK(run({{SKS_OK, false}}) == SKS_OK);
  CHECK(calls.size() == 1 && calls[0].bounds == &mask_bounds && calls[0].has_flag);
  // a failure that is no invalid layout: returned, not retried
  for (int rc : {SKS_E_ARG, SKS_E_HIP, SKS_E_LENGTH, SKS_E_UNSUPPORTED}) {
    CHECK(run({{rc, false}}) == rc);
    CHECK(calls.size() == 1 && calls[0].bounds == &mask_bounds);
  }
  // an invalid layout: once more with sampled bounds, the second status returned
  CHECK(run({{SKS_E_UNSUPPORTED, true}, {SKS_OK, false}}) == SKS_OK);
  CHECK(calls.size() == 2 && calls[0].bounds == &mask_bounds && calls[1].bounds == nullptr && !calls[1].has_flag);
  CHECK(run({{SKS_E_UNSUPPORTED, true}, {SKS_E_LENGTH, false}}) == SKS_E_LENGTH);
  CHECK(calls.size() == 2 && calls[1].bounds == nullptr);
  // invalid again: no third call (steps.at would throw)
  CHECK(run({{SKS_E_UNSUPPORTED, true}, {SKS_E_UNSUPPORTED, true}}) == SKS_E_UNSUPPORTED);
  CHECK(calls.size() == 2);
}

}  // namespace

int main() {
  check_differs();
  check_ones();
  check_retry();
  std::printf("set rules ok\n");
  return 0;
}
