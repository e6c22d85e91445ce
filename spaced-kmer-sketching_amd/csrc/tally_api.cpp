// C-ABI implementation (include/sks.h): sks_sketch_set_tally — per group of
// source sketches, the elements held by min_count .. max_count of the listed
// members, optionally with how many hold each.  The argument check and the merge
// rounds are sks_sketch_set_merge's (merge_rounds.cpp): they leave a group as
// one sorted run in which a value appears once per member holding it, and
// tally.hip's last pass keeps the heads of the runs of the asked lengths.
#include "sks_ctx.hpp"

using namespace sks;

namespace {

const char* const kWho = "sks_sketch_set_tally";
const char* const kFracOnly =
    "policy kind: FracMinHash sets only (whether a bottom-s sketch holds a value depends on its other values, so "
    "absence from it says nothing)";

}  // namespace

extern "C" int sks_sketch_set_tally(sks_ctx* c, const sks_sketch_set* const* sets, uint32_t n_sets,
                                    const uint32_t* group_off, const uint32_t* members, uint32_t n_groups,
                                    const uint32_t* min_count, const uint32_t* max_count, sks_sketch_set** out,
                                    uint32_t* d_counts, uint64_t counts_cap) {
  if (out) *out = nullptr;
  GroupSources S;
  SKS_TRY(group_sources(kWho, c, sets, n_sets, group_off, members, n_groups, out, kFracOnly, &S));
  const sks_sketch_set* first = sets[0];
  const int ew = S.ew;
  // per group: lo | hi << 32, listed members
  std::vector<uint64_t> limits(2 * (size_t)n_groups, 0);
  for (uint32_t g = 0; g < n_groups; ++g) {
    limits[2 * (size_t)g] = tally_lo(min_count, g) | (uint64_t)tally_hi(max_count, g) << 32;
    limits[2 * (size_t)g + 1] = S.goff[g + 1] - S.goff[g];
  }

  DeviceGuard guard(c->device);
  hipStream_t st = c->stream;
  GroupRuns R;
  SKS_TRY(queue_group_rounds(c, S, &limits, &R));
  SetPtr set;
  SKS_TRY(make_sketch_set(c->device, ew, first->window, first->mask, S.policy, std::vector<uint32_t>(n_groups, 0),
                          S.windows, {}, nullptr, st, MetaUpload::kNone, &set));
  SKS_HIP(sks::tally_count(R.d_runs, R.d_chunk_off, R.d_extra, n_groups, R.n_chunks, ew, chunk_counts(c), st));
  // the call's one wait; a tally holds no more than its members
  SKS_TRY(size_set_from_counts(c, kWho, "a tally is larger than its members", R.n_chunks, R.d_chunk_off,
                               R.run_len.data(), set.get()));
  uint64_t total = 0;
  for (uint32_t v : set->sizes) total += v;
  if (d_counts && counts_cap < total)
    return sks::fail(SKS_E_LENGTH, std::string(kWho) + ": the result holds " + std::to_string(total) +
                                       " elements, d_counts only " + std::to_string(counts_cap) +
                                       " (the sum of the listed members' sizes always suffices)");
  SKS_HIP(sks::tally_scatter(R.d_runs, R.d_chunk_off, R.d_extra, n_groups, R.n_chunks, ew, chunk_offs(c),
                             set->d_data(), d_counts, st));
  *out = set.release();
  return SKS_OK;
}
