// The decisions the set-level calls share, free of any device: which fields of
// two sketch sets must agree, how many positions a mask selects, and the one
// retry of a call whose join layout the mask's group bounds could not place.
// Only sks.h and the standard library (tests/cpp/set_rules_test.cpp builds it alone).
#pragma once
#include <cstdint>
#include <vector>

#include "sks.h"

namespace sks {

// When the policy param must match: for FracMinHash only (bottom-s of another s
// still compares: search, top-k, gather, merge), or always (concat: one policy a set).
enum class ParamRule { kFracOnly, kAlways };

// The first field two sets differ in, or null: window, mask, elem_words, policy
// kind, hash flavour, nonce, policy param.
inline const char* set_differs_in(const sks_sketch_info& a, const sks_sketch_info& b, ParamRule rule) {
  if (a.window != b.window) return "window";
  if (a.mask[0] != b.mask[0] || a.mask[1] != b.mask[1]) return "mask";
  if (a.elem_words != b.elem_words) return "elem_words";
  if (a.policy.kind != b.policy.kind) return "policy kind";
  if (a.policy.flavour != b.policy.flavour) return "hash flavour";
  if (a.policy.nonce != b.policy.nonce) return "nonce";
  if ((rule == ParamRule::kAlways || a.policy.kind == SKS_FRAC_MOD) && a.policy.param != b.policy.param)
    return "policy param (FracMinHash c)";
  return nullptr;
}

// kmer_num_ones of a mask: two mask bits a selected position.
inline int kmer_ones_of(const uint64_t mask[2]) {
  return (__builtin_popcountll(mask[0]) + __builtin_popcountll(mask[1])) / 2;
}

// core(h_bounds, invalid_layout) -> status runs a call with the given host group
// bounds (null: sampled from the data) and raises *invalid_layout (when given)
// if it failed because a layout could not be placed.  The mask's bounds need no
// sampling pass; k-mers far from uniform can overfill one of their groups, and
// then the call runs once more with sampled bounds.  No other result is retried.
template <class Core>
int with_mask_bounds_retry(const std::vector<uint64_t>& mask_bounds, Core core) {
  bool invalid = false;
  const int rc = core(&mask_bounds, &invalid);
  if (!invalid) return rc;
  return core(nullptr, nullptr);
}

}  // namespace sks
