// C-ABI implementation (include/sks.h): sks_sketch_set_merge — grouped unions
// of the sketches of device sketch sets.  The host plans the pairwise merge
// rounds (merge_plan.hpp) and uploads their run tables once; merge.hip merges,
// drops the duplicates, and bottom-s sketches that grew past s are cut by
// downsample's selection (downsample_arrays).
#include "sks_ctx.hpp"

using namespace sks;

namespace {

const char* const kWho = "sks_sketch_set_merge";

int refuse(const std::string& what) { return sks::fail(SKS_E_ARG, std::string(kWho) + ": " + what); }

}  // namespace

extern "C" int sks_sketch_set_merge(sks_ctx* c, const sks_sketch_set* const* sets, uint32_t n_sets,
                                    const uint32_t* group_off, const uint32_t* members, uint32_t n_groups,
                                    sks_sketch_set** out) {
  if (out) *out = nullptr;
  if (!c || !sets || !out) return refuse("null argument");
  if (n_sets == 0) return refuse("no sets");
  uint64_t n_src = 0;
  for (uint32_t i = 0; i < n_sets; ++i) {
    if (!sets[i]) return refuse("null set");
    n_src += sets[i]->n;
  }
  const sks_sketch_set* first = sets[0];
  sks_policy policy = first->policy;
  for (uint32_t i = 0; i < n_sets; ++i) {
    const sks_sketch_set* b = sets[i];
    if (b->device != c->device)
      return refuse("set " + std::to_string(i) + " is on device " + std::to_string(b->device) +
                    ", the context on device " + std::to_string(c->device));
    if (const char* f = set_differs_in(info_of(*first), info_of(*b), ParamRule::kFracOnly))
      return refuse("set " + std::to_string(i) + " differs from set 0 in " + f);
    policy.param = std::min(policy.param, b->policy.param);  // bottom-s: the smallest s
  }
  const bool bottom = policy.kind == SKS_BOTTOM_S;
  if (!bottom && policy.kind != SKS_FRAC_MOD) return refuse("unknown policy kind");
  if (policy.flavour != 0 && policy.flavour != 1) return refuse("unknown hash flavour");
  const int ew = first->elem_words;
  if (ew != 1 && ew != 2) return refuse("elements of 1 or 2 words only");
  if (bottom && policy.param == 0) return refuse("policy param must be > 0");
  if (n_groups && !group_off) return refuse("null group_off");
  if (n_groups && group_off[0] != 0) return refuse("group_off does not start at 0");
  for (uint32_t g = 0; g < n_groups; ++g)
    if (group_off[g + 1] < group_off[g]) return refuse("group_off decreases at group " + std::to_string(g));
  const uint32_t n_members = n_groups ? group_off[n_groups] : 0;
  if (n_members && !members) return refuse("null members");
  for (uint32_t j = 0; j < n_members; ++j)
    if (members[j] >= n_src)
      return refuse("member index " + std::to_string(members[j]) + " is out of range (" + std::to_string(n_src) +
                    " source sketches)");

  // the source sketches, numbered as sks_sketch_set_concat orders them
  std::vector<uint64_t> src_addr, src_windows;
  std::vector<uint32_t> src_len;
  src_addr.reserve(n_src), src_windows.reserve(n_src), src_len.reserve(n_src);
  for (uint32_t i = 0; i < n_sets; ++i)
    for (uint32_t k = 0; k < sets[i]->n; ++k) {
      src_addr.push_back(reinterpret_cast<uint64_t>(sets[i]->d_data() + sets[i]->starts[k] * ew));
      src_len.push_back(sets[i]->sizes[k]);
      src_windows.push_back(sets[i]->windows[k]);
    }
  std::vector<uint32_t> goff(n_groups + 1, 0), member_len(n_members);
  std::vector<uint64_t> windows(n_groups, 0);
  for (uint32_t g = 0; g < n_groups; ++g) {
    goff[g + 1] = group_off[g + 1];
    uint64_t sum = 0;
    for (uint32_t j = group_off[g]; j < group_off[g + 1]; ++j) {
      member_len[j] = src_len[members[j]];
      sum += member_len[j];
      windows[g] += src_windows[members[j]];
    }
    if (sum >> 32)
      return sks::fail(SKS_E_UNSUPPORTED, std::string(kWho) + ": the members of group " + std::to_string(g) + " hold " +
                                              std::to_string(sum) + " elements (sketch sizes are 32-bit)");
  }

  DeviceGuard guard(c->device);
  hipStream_t st = c->stream;
  const MergePlan plan = plan_merge(goff, member_len);
  const uint64_t T = plan.dense_off[n_groups];
  // round r writes column r & 1 and reads the other (round 0: the source sets)
  if (!plan.rounds.empty()) SKS_TRY(reserve_cols(c, {0, 1}, T * ew));
  auto round_addr = [&](int r, uint64_t off) {
    return reinterpret_cast<uint64_t>(col(c, r & 1) + off * ew);
  };

  MetaArena arena(c);
  struct RoundAt {
    size_t pairs, tiles;
  };
  std::vector<RoundAt> at;
  std::vector<uint64_t> table;
  for (size_t r = 0; r < plan.rounds.size(); ++r) {
    const MergeRound& R = plan.rounds[r];
    table.clear();
    for (size_t p = 0; p < R.pairs.size(); ++p) {
      auto run = [&](uint32_t i, uint64_t& addr, uint64_t& len) {
        addr = r == 0 ? src_addr[members[i]] : round_addr((int)r - 1, plan.rounds[r - 1].out[i].off);
        len = r == 0 ? member_len[i] : plan.rounds[r - 1].out[i].len;
      };
      uint64_t a_addr, a_len, b_addr, b_len = 0;
      run(R.pairs[p].a, a_addr, a_len);
      b_addr = a_addr;  // a carried run: no right run to read
      if (R.pairs[p].b != kMergeNoRun) run(R.pairs[p].b, b_addr, b_len);
      table.insert(table.end(), {a_addr, b_addr, round_addr((int)r, R.out[p].off), a_len | b_len << 32});
    }
    at.push_back({arena.add(table), arena.add(R.tile_off)});
  }
  // where every group's one run lies, and the duplicate filter's chunks
  std::vector<uint64_t> runs(2 * (size_t)n_groups, 0), chunk_off(n_groups + 1, 0);
  std::vector<uint32_t> run_len(n_groups, 0);  // a union holds no more than its members (each sum fits 32 bits)
  for (uint32_t g = 0; g < n_groups; ++g) {
    const MergeFinal& f = plan.final_run[g];
    if (f.round >= 0)
      runs[2 * g] = round_addr(f.round, plan.rounds[f.round].out[f.run].off);
    else if (f.run != kMergeNoRun)
      runs[2 * g] = src_addr[members[f.run]];
    runs[2 * g + 1] = f.len;
    run_len[g] = (uint32_t)f.len;
    chunk_off[g + 1] = chunk_off[g] + tiles_of(f.len, kDownsampleChunk);
  }
  const uint64_t n_chunks = chunk_off[n_groups];
  const size_t o_runs = arena.add(runs), o_chunk = arena.add(chunk_off);
  SKS_TRY(arena.upload());

  SetPtr set;
  SKS_TRY(make_sketch_set(c->device, ew, first->window, first->mask, policy, std::vector<uint32_t>(n_groups, 0),
                          windows, {}, nullptr, st, MetaUpload::kNone, &set));
  SKS_TRY(reserve_chunk_counters(c, n_chunks));

  for (size_t r = 0; r < plan.rounds.size(); ++r) {
    const MergeRound& R = plan.rounds[r];
    SKS_HIP(sks::merge_round(arena.ptr(at[r].pairs), arena.ptr(at[r].tiles), (uint32_t)R.pairs.size(),
                             R.tile_off.back(), ew, st));
  }
  SKS_HIP(sks::merge_unique_count(arena.ptr(o_runs), arena.ptr(o_chunk), n_groups, n_chunks, ew, chunk_counts(c),
                                  st));
  // the first wait
  SKS_TRY(size_set_from_counts(c, kWho, "a union is larger than its members", n_chunks, arena.ptr(o_chunk),
                               run_len.data(), set.get()));
  SKS_HIP(sks::merge_unique_scatter(arena.ptr(o_runs), arena.ptr(o_chunk), n_groups, n_chunks, ew, chunk_offs(c),
                                    set->d_data(), st));
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
