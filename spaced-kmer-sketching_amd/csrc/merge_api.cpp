// C-ABI implementation (include/sks.h): sks_sketch_set_merge — grouped unions
// of the sketches of device sketch sets.  The host plans the pairwise merge
// rounds (merge_plan.hpp) and uploads their run tables once (merge_rounds.cpp,
// shared with sks_sketch_set_tally); merge.hip merges, drops the duplicates, and
// bottom-s sketches that grew past s are cut by downsample's selection
// (downsample_arrays).
#include "sks_ctx.hpp"

using namespace sks;

namespace {

const char* const kWho = "sks_sketch_set_merge";

}  // namespace

extern "C" int sks_sketch_set_merge(sks_ctx* c, const sks_sketch_set* const* sets, uint32_t n_sets,
                                    const uint32_t* group_off, const uint32_t* members, uint32_t n_groups,
                                    sks_sketch_set** out) {
  if (out) *out = nullptr;
  GroupSources S;
  SKS_TRY(group_sources(kWho, c, sets, n_sets, group_off, members, n_groups, out, nullptr, &S));
  const sks_sketch_set* first = sets[0];
  const sks_policy policy = S.policy;
  const bool bottom = policy.kind == SKS_BOTTOM_S;
  const int ew = S.ew;

  DeviceGuard guard(c->device);
  hipStream_t st = c->stream;
  GroupRuns R;
  SKS_TRY(queue_group_rounds(c, S, nullptr, &R));
  SetPtr set;
  SKS_TRY(make_sketch_set(c->device, ew, first->window, first->mask, policy, std::vector<uint32_t>(n_groups, 0),
                          S.windows, {}, nullptr, st, MetaUpload::kNone, &set));
  SKS_HIP(sks::merge_unique_count(R.d_runs, R.d_chunk_off, n_groups, R.n_chunks, ew, chunk_counts(c), st));
  // the first wait; a union holds no more than its members
  SKS_TRY(size_set_from_counts(c, kWho, "a union is larger than its members", R.n_chunks, R.d_chunk_off,
                               R.run_len.data(), set.get()));
  SKS_HIP(sks::merge_unique_scatter(R.d_runs, R.d_chunk_off, n_groups, R.n_chunks, ew, chunk_offs(c), set->d_data(),
                                    st));
  const auto over_s = [&](uint32_t v) { return v > policy.param; };  // bottom-s: a union holds more than s elements
  if (bottom && std::any_of(set->sizes.begin(), set->sizes.end(), over_s)) {
    // the second wait; the uncut set goes back to the block cache behind the queued filter
    SetPtr kept;
    SKS_TRY(downsample_arrays(c, kWho, set->d_data(), set->d_starts(), set->d_sizes(), set->sizes, *set, policy.param,
                              &kept));
    set = std::move(kept);
  }
  *out = set.release();
  return SKS_OK;
}
