// What build.cpp (the pass loop, the single-genome paths), build_post.cpp (a
// pass's post-processing) and kmer_list.cpp share.
#pragma once
#include "sks_ctx.hpp"
#include "sks_hash.hpp"

namespace sks {

inline std::vector<uint64_t> prefix(const std::vector<uint64_t>& v) {
  std::vector<uint64_t> o(v.size() + 1, 0);
  for (size_t i = 0; i < v.size(); ++i) o[i + 1] = o[i] + v[i];
  return o;
}

struct BuildState {
  sks_ctx* c;
  int w;
  bool wide;
  int ew;
  uint64_t mask_lo, mask_hi;
  sks_policy pol;
  uint64_t kconst;
  sks::DivTest dt;
  // narrow keys are packed to their mask bits for the sorts (sks::BitRuns) and
  // expanded again when the unique elements are written out; wide keys are not
  sks::BitRuns runs;
  int key_bits;
  BuildKnobs knobs;
  // sks_sketch_build_counted: the FracMinHash pipeline also counts, and keeps by these limits
  bool counted = false;
  uint32_t min_abund = 0, max_abund = 0xffffffffu;
};

// The build's environment knobs, in one place (build.cpp).  The SKS_NO_* ones
// are read on every call (tests set them at run time), SKS_SCAN_STATIC once.
BuildKnobs read_build_knobs();

inline BuildState build_state(sks_ctx* c, int window, const uint64_t mask[2], const sks_policy& policy) {
  const bool wide = window > 32;
  BuildState S{c, window, wide, wide ? 2 : 1, mask[0], mask[1], policy,
               sks::fmh_const(mask[0], mask[1], window, policy.nonce, policy.flavour), {},
               wide ? sks::BitRuns{} : sks::bit_runs(mask[0]), wide ? 64 : std::max(1, __builtin_popcountll(mask[0])),
               read_build_knobs()};
  if (policy.kind == SKS_FRAC_MOD) S.dt = sks::make_div_test(policy.param);
  return S;
}

// One completed pass: final sketches of `segs` (global segment ids) in CSR.
// The block is only used on the context's stream.
struct PassOut {
  DevBlock d;                     // elements (elem_words u64 each)
  DevBlock abund;                 // a counted build: one u32 per element
  std::vector<uint32_t> segs;
  std::vector<uint64_t> off;      // CSR in elements, size segs.size() + 1
};

// Post-process the segments `ok` (pass-local indices into the pass arrays) whose
// survivors sit in the record regions [out_off[i], out_off[i] + count[i]).
// Appends a PassOut; for bottom-s reports segments that need a larger threshold.
int post_process(BuildState& S, const std::vector<uint32_t>& seg_ids, const std::vector<uint64_t>& out_off,
                 const std::vector<uint64_t>& counts, const std::vector<uint64_t>& thresh,
                 const std::vector<uint32_t>& ok, std::vector<PassOut>& passes, std::vector<uint32_t>& retry_local,
                 std::vector<uint64_t>& final_size_local);

// Argument checks shared by sks_sketch_build and sks_kmer_list_build.
int validate_build(const char* fn, sks_ctx* c, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off,
                   uint32_t n_seg, int window, const uint64_t mask[2], const sks_policy* policy);

// The per-segment host arrays of one scan launch (launch-local segment index);
// the record regions lie back to back in segment order.
struct ScanSegs {
  std::vector<uint64_t> beg, end, thresh, cap, off;  // [m]; thresh: bottom-s pre-filter (~0: none)
  std::vector<uint64_t> tiles{0};                    // [m + 1] tiles before each segment
  uint64_t total_cap = 0;
  void push(uint64_t b, uint64_t e, uint64_t thr, uint64_t c) {
    beg.push_back(b);
    end.push_back(e);
    thresh.push_back(thr);
    cap.push_back(c);
    off.push_back(total_cap);
    tiles.push_back(tiles.back() + sks::scan_tiles_for(e - b));
    total_cap += c;
  }
  uint32_t m() const { return (uint32_t)beg.size(); }
  uint64_t n_tiles() const { return tiles.back(); }
};

// A scan's metadata on the device, laid out in this one place.  The arena holds,
// in this order: begin, end, tile prefix, threshold (not in list mode),
// capacity, record offset, the caller's `extra` words for its post kernel, the
// counters block, and the tile queue's counter (not in list mode).  The
// counters block is contiguous, so one read-back fetches it whole:
//   [0, m) survivors, 0, [m + 1, 2m + 1) windows, 0, then `result_words` words a fused post kernel writes
struct ScanMeta {
  sks::ScanParams p;
  uint64_t* extra;
  uint64_t* counters;
  uint64_t* results;
};

int scan_meta(const BuildState& S, const uint8_t* d_seq, const ScanSegs& g, bool list_mode,
              const std::vector<uint64_t>& extra, size_t result_words, ScanMeta* out);

}  // namespace sks
