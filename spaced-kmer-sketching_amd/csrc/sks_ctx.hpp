// What the C-ABI translation units that run on a device share (ctx.cpp,
// host_mem.cpp, sketch_set.cpp, kmer_list.cpp, build.cpp, build_post.cpp,
// pairs.cpp, search_api.cpp, topk_api.cpp, cluster_api.cpp, gather_api.cpp,
// downsample_api.cpp, merge_rounds.cpp, merge_api.cpp, tally_api.cpp, filter_api.cpp,
// abund_api.cpp): the
// context, the sketch set and k-mer
// list with the device blocks they own, the error macros, the metadata arena,
// SketchSpan and the group bounds of the set-level calls (their device-free
// rules: set_rules.hpp) and small argument helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "abund.hpp"
#include "ani.hpp"
#include "cluster.hpp"
#include "code_objects.hpp"
#include "device_mem.hpp"
#include "downsample.hpp"
#include "filter.hpp"
#include "gather.hpp"
#include "ingress.hpp"
#include "intersect.hpp"
#include "join.hpp"
#include "merge.hpp"
#include "post.hpp"
#include "scan.hpp"
#include "scratch_carve.hpp"
#include "search_kernels.hpp"
#include "set_rules.hpp"
#include "sks.h"
#include "sks_api_internal.hpp"
#include "tally.hpp"
#include "topk.hpp"
#include "windows.hpp"

#define SKS_HIP(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return sks::fail(SKS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)

#define SKS_TRY(expr)              \
  do {                             \
    int rc_ = (expr);              \
    if (rc_ != SKS_OK) return rc_; \
  } while (0)

struct sks_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_s0 = nullptr, ev_s1 = nullptr;
  hipEvent_t ev_i0 = nullptr, ev_i1 = nullptr;  // device FASTA ingress
  sks::Scratch ingress;             // per-line arrays of the device FASTA parser
  sks::Scratch tmp;                 // rocPRIM temporary storage
  sks::Scratch rec[3];              // scan records (key, val, hi)
  sks::Scratch buf[10];             // dense working columns
  sks::Scratch flag, pos;
  sks::Scratch meta;                // small per-segment device arrays
  sks::Scratch iwork;               // intersection bucket tables
  sks::Scratch tdone;               // fused ANI: workgroups finished per join tile
  sks::Scratch lay;                 // one call's carve: sks_all_pairs_ani, the search walk, cluster, gather
  const uint32_t* layout_stat = nullptr;  // the last join-layout build's 2 status words (in iwork)
  std::vector<uint64_t> meta_host;  // staging for `meta`
  sks_timings last{};
  int grid_override = 0;
  int intersect_algo = 0;  // sks::kIntersect*
  bool join_check = false;  // invariant-checking join / layout kernels (sks_ctx_set_join_check)
  uint32_t layout_blocks_hint = 0;  // sks_ctx_set_layout_blocks_hint (0: every block holds sketches)
  sks::Scratch root;                // sks_ctx_ani_table: ANI by shared-element count for one set size
  sks::Scratch fstate;              // build_frac_single: bucket cursors, distinct counts, status
  bool fstate_clean = false;        // fstate is zeroed and no launch sequence was cut short
  int frac_mode = SKS_FRAC_POST_AUTO;  // sks_ctx_set_frac_post
  uint32_t frac_bucket_cap = 0;     // 0: the kernel's capacity
  uint32_t frac_buckets = 0;        // 0: chosen from the expected survivors
  int last_path = SKS_BUILD_PATH_GENERAL;  // sks_ctx_last_build_path
  uint32_t root_size = 0;
  int root_k = 0;                   // 0: no table
  sks::Scratch hits;                // sks_search: unsorted hit records, sort keys and indices
  uint32_t search_batch = 0;        // sks_ctx_set_search_batch (0: from the tile budget)
  uint32_t gather_rounds = 0;       // sks_ctx_set_gather_rounds (0: kGatherDefaultRounds)

  // every Scratch member (a new one is added here, and nowhere else)
  template <class F>
  void each_scratch(F f) {
    for (sks::Scratch* sc : {&ingress, &tmp, &flag, &pos, &meta, &iwork, &tdone, &lay, &root, &fstate, &hits}) f(*sc);
    for (auto& r : rec) f(r);
    for (auto& b : buf) f(b);
  }
  // the events created so far (with the context's device current)
  ~sks_ctx() {
    for (hipEvent_t ev : {ev_begin, ev_end, ev_s0, ev_s1, ev_i0, ev_i1})
      if (ev) (void)hipEventDestroy(ev);
  }
};

// A device-resident set of sketches (one per genome / segment).  Its arrays are
// cached device blocks: a set dropped half-built gives them back by itself.
struct sks_sketch_set {
  int device = 0;
  int elem_words = 1;
  uint32_t n = 0;
  sks::DevBlock data;     // elements (elem_words u64 each)
  sks::DevBlock dstarts;  // [n] u64 element index of each sketch
  sks::DevBlock dsizes;   // [n] u32
  sks::DevBlock abund;    // optional: [total] u32, the abundance of every element (a counted set)
  uint32_t* d_abund() const { return abund.as<uint32_t>(); }
  bool has_abund() const { return static_cast<bool>(abund); }
  uint64_t* d_data() const { return data.as<uint64_t>(); }
  uint64_t* d_starts() const { return dstarts.as<uint64_t>(); }
  uint32_t* d_sizes() const { return dsizes.as<uint32_t>(); }
  std::vector<uint32_t> sizes;
  std::vector<uint64_t> starts;
  std::vector<uint64_t> windows;
  // how the sketches were made (persisted with them)
  int window = 0;
  uint64_t mask[2] = {0, 0};
  sks_policy policy{};
  std::vector<std::string> names;  // optional, from a sketch file or sks_sketch_set_set_name
};

struct sks_kmer_list {
  int device = 0;
  uint32_t n = 0;
  uint64_t total = 0;
  sks::DevBlock pos;   // [total] u64 window start byte of each k-mer, stream order
  sks::DevBlock bits;  // [total][4] u64 kmer_bits lo, hi, masked_bits lo, hi
  std::vector<uint64_t> counts;
};

namespace sks {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// Packs small host arrays into ctx->meta with one H2D copy.
class MetaArena {
 public:
  explicit MetaArena(sks_ctx* c) : c_(c) { c_->meta_host.clear(); }
  // reserve n words; returns the word offset
  size_t add(const std::vector<uint64_t>& v) {
    size_t o = c_->meta_host.size();
    c_->meta_host.insert(c_->meta_host.end(), v.begin(), v.end());
    c_->meta_host.push_back(0);  // keep every array non-empty
    return o;
  }
  size_t add_zero(size_t n) {
    size_t o = c_->meta_host.size();
    c_->meta_host.resize(o + n + 1, 0);
    return o;
  }
  int upload() {
    size_t bytes = c_->meta_host.size() * sizeof(uint64_t);
    SKS_HIP(c_->meta.reserve(bytes));
    SKS_HIP(sks::pinned_h2d(c_->meta.ptr, c_->meta_host.data(), bytes, c_->stream));
    return SKS_OK;
  }
  uint64_t* ptr(size_t off) const { return reinterpret_cast<uint64_t*>(c_->meta.ptr) + off; }

 private:
  sks_ctx* c_;
};

inline uint64_t* col(sks_ctx* c, int i) { return reinterpret_cast<uint64_t*>(c->buf[i].ptr); }

inline int reserve_cols(sks_ctx* c, std::initializer_list<int> ids, uint64_t words) {
  for (int i : ids) SKS_HIP(c->buf[i].reserve(std::max<uint64_t>(words, 1) * sizeof(uint64_t)));
  return SKS_OK;
}

inline int end_bit_of(uint64_t max_value) {
  int b = 64 - __builtin_clzll(max_value | 1);
  return b < 1 ? 1 : b;
}

// A block of `words` u64 (at least one) from the block cache, bound to `st`.
inline int alloc_u64(DevBlock& b, uint64_t words, hipStream_t st) {
  SKS_HIP(b.alloc(std::max<uint64_t>(words, 1) * sizeof(uint64_t), st));
  return SKS_OK;
}

// ---- sketch sets (sketch_set.cpp) -------------------------------------------------------
using SetPtr = std::unique_ptr<sks_sketch_set>;
// How a new set's d_starts / d_sizes get their contents: written by the device
// later (the caller then sets the host sizes and starts), uploaded on `st`
// through the pinned ring without waiting, or with blocking copies.
enum class MetaUpload { kNone, kStream, kBlocking };
// The one place that makes a set: fills the host fields (starts from sizes),
// allocates d_starts and d_sizes and, with `data_words`, d_data of that many
// words, every block bound to `st`; uploads the metadata as `up` says.  With
// `abund` the set takes that block (one u32 per element) as its abundances.
int make_sketch_set(int device, int elem_words, int window, const uint64_t mask[2], const sks_policy& policy,
                    std::vector<uint32_t> sizes, std::vector<uint64_t> windows, std::vector<std::string> names,
                    const uint64_t* data_words, hipStream_t st, MetaUpload up, SetPtr* out,
                    DevBlock* abund = nullptr);

inline sks_sketch_info info_of(const sks_sketch_set& s) {
  return {s.window, s.elem_words, {s.mask[0], s.mask[1]}, s.policy, s.n, s.names.empty() ? 0 : 1};
}

// ---- a set's arrays as the set-level calls take them ------------------------------------
struct SketchSpan {
  const uint64_t* data;
  const uint64_t* starts;
  const uint32_t* sizes;
  uint32_t n, max_size;
  uint64_t total;
  const uint32_t* h_sizes;  // host copy of the sizes, or null (batches are then sized by max_size)
};

inline SketchSpan span_of(const sks_sketch_set* s) {
  SketchSpan S{s->d_data(), s->d_starts(), s->d_sizes(), s->n, 0, 0, s->sizes.data()};
  for (uint32_t v : s->sizes) {
    S.max_size = std::max(S.max_size, v);
    S.total += v;
  }
  return S;
}

// Element indices are 32-bit: "<who>: >= 2^32 elements <where>".
inline int check_span_totals(const char* who, const char* where, uint64_t total_a, uint64_t total_b = 0) {
  if (!((total_a | total_b) >> 32)) return SKS_OK;
  return sks::fail(SKS_E_UNSUPPORTED, std::string(who) + ": >= 2^32 elements " + where);
}

// A query and a reference set that the search, top-k and gather may compare:
// no differing field, both on the context's device, a mask that selects a
// position.  `frac_only`: a refusal between the fields and the device, the text
// after "<me>: " for sets that are not FracMinHash.  *info: the queries'.
inline int search_sets_compatible(const sks_ctx* c, const std::string& me, const sks_sketch_set* queries,
                                  const sks_sketch_set* refs, sks_sketch_info* info, int* kmer_num_ones,
                                  const char* frac_only = nullptr) {
  *info = info_of(*queries);
  if (const char* field = set_differs_in(*info, info_of(*refs), ParamRule::kFracOnly))
    return sks::fail(SKS_E_ARG, me + ": the query and reference sets differ in " + field);
  if (frac_only && info->policy.kind != SKS_FRAC_MOD) return sks::fail(SKS_E_ARG, me + ": " + frac_only);
  if (queries->device != c->device || refs->device != c->device)
    return sks::fail(SKS_E_ARG, me + ": a set lives on another device than the context");
  *kmer_num_ones = kmer_ones_of(info->mask);
  if (*kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, me + ": the sets' mask selects no position");
  return SKS_OK;
}

// The group bounds the mask fixes for sketches of at most max_size elements
// ((G + 1) * elem_words words for that size's log_b): no sampling pass.
inline int mask_group_bounds(const uint64_t mask[2], int elem_words, uint32_t max_size, std::vector<uint64_t>* out) {
  const uint32_t log_b = sks::join_log_b(std::max<uint32_t>(max_size, 1));
  out->assign((size_t)(sks::join_layout_groups(log_b) + 1) * elem_words, 0);
  return sks_join_layout_bounds_for_mask(mask, log_b, elem_words, out->data());
}

// Queues a layout's group bounds into d_bounds: the host's if given, else sampled from S.
inline int queue_group_bounds(sks_ctx* c, const SketchSpan& S, uint32_t log_b, int ew,
                              const std::vector<uint64_t>* h_bounds, uint64_t* d_bounds) {
  if (h_bounds)
    SKS_HIP(sks::pinned_h2d(d_bounds, h_bounds->data(), (size_t)(sks::join_layout_groups(log_b) + 1) * 8 * ew,
                            c->stream));
  else
    SKS_HIP(sks::join_layout_bounds(S.data, S.starts, S.sizes, S.n, log_b, ew, d_bounds, c->stream));
  return SKS_OK;
}

// A layout build raised status word 1 (*invalid_layout: for with_mask_bounds_retry).
inline int fail_invalid_layout(const std::string& me, const std::string& what, const char* nothing,
                               bool* invalid_layout) {
  if (invalid_layout) *invalid_layout = true;
  return sks::fail(SKS_E_UNSUPPORTED,
                   me + ": the join layout of " + what + " could not be placed (invalid layout); " + nothing);
}

// ---- filters over a set's arrays (downsample_api.cpp) -----------------------------------
// sks_sketch_set_downsample after its argument checks, over the CSR arrays
// (d_data, d_starts, d_sizes; src_sizes on the host) of sketches made as `like`
// says (elem_words, window, mask, policy; its windows and names are carried
// over): a new set at policy param `param`.  Waits for the stream once.
int downsample_arrays(sks_ctx* c, const char* who, const uint64_t* d_data, const uint64_t* d_starts,
                      const uint32_t* d_sizes, const std::vector<uint32_t>& src_sizes, const sks_sketch_set& like,
                      uint64_t param, SetPtr* out);
// chunk_off[g], dense_off[g]: the kDownsampleChunk-element chunks and the elements before
// sketch g of sketches of these sizes ([n + 1] each)
void chunk_prefixes(const std::vector<uint32_t>& sizes, std::vector<uint64_t>* chunk_off,
                    std::vector<uint64_t>* dense_off);
// The tail of a call whose count kernel decides the new sketches' sizes: kept
// elements per kDownsampleChunk-element chunk in chunk_counts(c), reserved with
// chunk_offs(c) before that kernel is queued.  size_set_from_counts queues
// downsample_offsets (d_chunk_off: [set->n + 1] chunks before each sketch),
// reads the sizes back (one wait), fails with "<who>: <too_large>" (SKS_E_HIP)
// if sizes[g] > bound[g], and fills the set's host starts and sizes and
// allocates its data to the exact total.  The caller's scatter follows.
inline uint32_t* chunk_counts(sks_ctx* c) { return reinterpret_cast<uint32_t*>(c->flag.ptr); }
inline uint64_t* chunk_offs(sks_ctx* c) { return reinterpret_cast<uint64_t*>(c->pos.ptr); }
int reserve_chunk_counters(sks_ctx* c, uint64_t n_chunks);
int size_set_from_counts(sks_ctx* c, const char* who, const char* too_large, uint64_t n_chunks,
                         const uint64_t* d_chunk_off, const uint32_t* bound, sks_sketch_set* set);

// ---- groups of source sketches and their merge rounds (merge_rounds.cpp) ----------------
// What sks_sketch_set_merge and sks_sketch_set_tally share.  group_sources is
// their argument check, refusing as "<who>: ..." (null ctx, sets or out before
// anything else; no sets; a null set; a set on another device or differing from
// set 0, ParamRule::kFracOnly; with `frac_only`, that text for sets that are not
// FracMinHash; unknown kind or flavour; elem_words; bottom-s param 0; group_off
// and member indices; SKS_E_UNSUPPORTED for a group of 2^32 or more elements),
// and the source sketches it leaves, numbered as sks_sketch_set_concat orders them.
struct GroupSources {
  int ew = 1;
  sks_policy policy{};               // set 0's; bottom-s: the smallest param
  uint32_t n_groups = 0, n_members = 0;
  const uint32_t* members = nullptr;  // the caller's
  std::vector<uint64_t> src_addr;     // [source sketches] device address of the first element
  std::vector<uint32_t> goff;         // [n_groups + 1]
  std::vector<uint32_t> member_len;   // [n_members] elements of each listed member
  std::vector<uint64_t> windows;      // [n_groups] sum of the listed members' windows
};
int group_sources(const char* who, const sks_ctx* c, const sks_sketch_set* const* sets, uint32_t n_sets,
                  const uint32_t* group_off, const uint32_t* members, uint32_t n_groups, const void* out,
                  const char* frac_only, GroupSources* S);
// queue_group_rounds plans the pairwise rounds (merge_plan.hpp), uploads their
// run tables, the final `runs` and `chunk_off` tables and the caller's `extra`
// table (may be null) in one arena, reserves the two scratch columns and the
// chunk counters and queues every round on the context's stream (its device
// current).  Afterwards group g is one sorted run, duplicates kept, of
// run_len[g] elements at d_runs[2g]; the last pass is the caller's.
struct GroupRuns {
  const uint64_t *d_runs = nullptr, *d_chunk_off = nullptr, *d_extra = nullptr;
  uint64_t n_chunks = 0;
  std::vector<uint32_t> run_len;  // [n_groups]; each fits 32 bits (group_sources)
};
int queue_group_rounds(sks_ctx* c, const GroupSources& S, const std::vector<uint64_t>* extra, GroupRuns* R);

// ---- argument helpers (ctx.cpp) ---------------------------------------------------------
// The opening checks of the entry points that take a join layout: a context, a
// bucket count the layout format holds, and 64- or 128-bit elements.
int check_layout_args(const char* who, const sks_ctx* c, uint32_t log_b, int elem_words);
// The fused ANI store runs in k_join: the caller's matrix must be memory the
// device can write — device memory, managed memory, or pinned host memory
// mapped into the device (sks_host_alloc), whose device-side address is
// returned.  An ordinary malloc/numpy buffer is refused (SKS_E_ARG) instead of
// being handed to the kernel, where the store would fault (XNACK is off).
int device_view_of_ani(double* ani, double** d_ani, const char* who);
// The context's table (sks_ctx_ani_table), if it was built for this k.
void attach_ani_root(const sks_ctx* c, int kmer_num_ones, JoinAni& A);

inline JoinLayout view_of(const LayoutArrays& a) { return {a.vals, a.masks, a.boff, a.bstart}; }

}  // namespace sks
