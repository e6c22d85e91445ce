// The part of the grouped calls (sks_sketch_set_merge, sks_sketch_set_tally)
// that does not depend on their last pass: the argument check, the source
// sketches in concat order, and the pairwise merge rounds (merge_plan.hpp plans
// them, merge.hip runs them) that leave every group as one sorted run with its
// duplicates.
#include "sks_ctx.hpp"

namespace sks {

int group_sources(const char* who, const sks_ctx* c, const sks_sketch_set* const* sets, uint32_t n_sets,
                  const uint32_t* group_off, const uint32_t* members, uint32_t n_groups, const void* out,
                  const char* frac_only, GroupSources* S) {
  const auto refuse = [who](const std::string& what) { return sks::fail(SKS_E_ARG, std::string(who) + ": " + what); };
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
  if (frac_only && policy.kind != SKS_FRAC_MOD) return refuse(frac_only);
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
  std::vector<uint64_t> src_windows;
  std::vector<uint32_t> src_len;
  S->src_addr.clear();
  S->src_addr.reserve(n_src), src_windows.reserve(n_src), src_len.reserve(n_src);
  for (uint32_t i = 0; i < n_sets; ++i)
    for (uint32_t k = 0; k < sets[i]->n; ++k) {
      S->src_addr.push_back(reinterpret_cast<uint64_t>(sets[i]->d_data() + sets[i]->starts[k] * ew));
      src_len.push_back(sets[i]->sizes[k]);
      src_windows.push_back(sets[i]->windows[k]);
    }
  S->ew = ew;
  S->policy = policy;
  S->n_groups = n_groups;
  S->n_members = n_members;
  S->members = members;
  S->goff.assign(n_groups + 1, 0);
  S->member_len.assign(n_members, 0);
  S->windows.assign(n_groups, 0);
  for (uint32_t g = 0; g < n_groups; ++g) {
    S->goff[g + 1] = group_off[g + 1];
    uint64_t sum = 0;
    for (uint32_t j = group_off[g]; j < group_off[g + 1]; ++j) {
      S->member_len[j] = src_len[members[j]];
      sum += S->member_len[j];
      S->windows[g] += src_windows[members[j]];
    }
    if (sum >> 32)
      return sks::fail(SKS_E_UNSUPPORTED, std::string(who) + ": the members of group " + std::to_string(g) + " hold " +
                                              std::to_string(sum) + " elements (sketch sizes are 32-bit)");
  }
  return SKS_OK;
}

int queue_group_rounds(sks_ctx* c, const GroupSources& S, const std::vector<uint64_t>* extra, GroupRuns* R) {
  hipStream_t st = c->stream;
  const int ew = S.ew;
  const uint32_t n_groups = S.n_groups;
  const uint32_t* members = S.members;
  const MergePlan plan = plan_merge(S.goff, S.member_len);
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
    const MergeRound& Rd = plan.rounds[r];
    table.clear();
    for (size_t p = 0; p < Rd.pairs.size(); ++p) {
      auto run = [&](uint32_t i, uint64_t& addr, uint64_t& len) {
        addr = r == 0 ? S.src_addr[members[i]] : round_addr((int)r - 1, plan.rounds[r - 1].out[i].off);
        len = r == 0 ? S.member_len[i] : plan.rounds[r - 1].out[i].len;
      };
      uint64_t a_addr, a_len, b_addr, b_len = 0;
      run(Rd.pairs[p].a, a_addr, a_len);
      b_addr = a_addr;  // a carried run: no right run to read
      if (Rd.pairs[p].b != kMergeNoRun) run(Rd.pairs[p].b, b_addr, b_len);
      table.insert(table.end(), {a_addr, b_addr, round_addr((int)r, Rd.out[p].off), a_len | b_len << 32});
    }
    at.push_back({arena.add(table), arena.add(Rd.tile_off)});
  }
  // where every group's one run lies, and the last pass's chunks
  std::vector<uint64_t> runs(2 * (size_t)n_groups, 0), chunk_off(n_groups + 1, 0);
  R->run_len.assign(n_groups, 0);  // each sum fits 32 bits (group_sources)
  for (uint32_t g = 0; g < n_groups; ++g) {
    const MergeFinal& f = plan.final_run[g];
    if (f.round >= 0)
      runs[2 * g] = round_addr(f.round, plan.rounds[f.round].out[f.run].off);
    else if (f.run != kMergeNoRun)
      runs[2 * g] = S.src_addr[members[f.run]];
    runs[2 * g + 1] = f.len;
    R->run_len[g] = (uint32_t)f.len;
    chunk_off[g + 1] = chunk_off[g] + tiles_of(f.len, kDownsampleChunk);
  }
  R->n_chunks = chunk_off[n_groups];
  const size_t o_runs = arena.add(runs), o_chunk = arena.add(chunk_off);
  const size_t o_extra = extra ? arena.add(*extra) : 0;
  SKS_TRY(arena.upload());
  R->d_runs = arena.ptr(o_runs);
  R->d_chunk_off = arena.ptr(o_chunk);
  R->d_extra = extra ? arena.ptr(o_extra) : nullptr;
  SKS_TRY(reserve_chunk_counters(c, R->n_chunks));

  for (size_t r = 0; r < plan.rounds.size(); ++r) {
    const MergeRound& Rd = plan.rounds[r];
    SKS_HIP(sks::merge_round(arena.ptr(at[r].pairs), arena.ptr(at[r].tiles), (uint32_t)Rd.pairs.size(),
                             Rd.tile_off.back(), ew, st));
  }
  return SKS_OK;
}

}  // namespace sks
