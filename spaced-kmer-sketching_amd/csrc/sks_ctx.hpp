// What the C-ABI translation units that run on a device share (ctx.cpp,
// host_mem.cpp, sketch_set.cpp, kmer_list.cpp, build.cpp, build_post.cpp,
// pairs.cpp, search_api.cpp, topk_api.cpp, cluster_api.cpp, gather_api.cpp, downsample_api.cpp, merge_api.cpp): the context, the sketch set
// and k-mer list with the device blocks they own, the error macros, the
// metadata arena and small argument helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "ani.hpp"
#include "cluster.hpp"
#include "code_objects.hpp"
#include "device_mem.hpp"
#include "downsample.hpp"
#include "gather.hpp"
#include "ingress.hpp"
#include "intersect.hpp"
#include "join.hpp"
#include "merge.hpp"
#include "post.hpp"
#include "scan.hpp"
#include "scratch_carve.hpp"
#include "search_kernels.hpp"
#include "sks.h"
#include "sks_api_internal.hpp"
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
  sks::Scratch lay;                 // sks_all_pairs_ani: the join layout, its temp and packed counts
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
// words, every block bound to `st`; uploads the metadata as `up` says.
int make_sketch_set(int device, int elem_words, int window, const uint64_t mask[2], const sks_policy& policy,
                    std::vector<uint32_t> sizes, std::vector<uint64_t> windows, std::vector<std::string> names,
                    const uint64_t* data_words, hipStream_t st, MetaUpload up, SetPtr* out);

// ---- filters over a set's arrays (downsample_api.cpp) -----------------------------------
// sks_sketch_set_downsample after its argument checks, over the CSR arrays
// (d_data, d_starts, d_sizes; src_sizes on the host) of sketches made as `like`
// says (elem_words, window, mask, policy; its windows and names are carried
// over): a new set at policy param `param`.  Waits for the stream once.
int downsample_arrays(sks_ctx* c, const char* who, const uint64_t* d_data, const uint64_t* d_starts,
                      const uint32_t* d_sizes, const std::vector<uint32_t>& src_sizes, const sks_sketch_set& like,
                      uint64_t param, SetPtr* out);

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
