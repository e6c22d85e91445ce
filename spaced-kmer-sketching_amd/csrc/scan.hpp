// The fused scan kernel's launcher (scan.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sks {

constexpr int kModeFrac = 0;
constexpr int kModeBottom = 1;
constexpr int kModeList = 2;  // FracMinHash test, emits window start positions

// Arguments of the fused scan kernel (scan.hip).  All per-segment arrays are
// device arrays indexed by the launch-local segment index.
struct ScanParams {
  const uint8_t* seq;
  const uint64_t* seg_begin;    // [n_seg] first byte of each segment
  const uint64_t* seg_end;      // [n_seg] end byte (exclusive)
  const uint64_t* tile_prefix;  // [n_seg + 1] tiles before each segment
  uint32_t n_seg;
  uint64_t n_tiles;
  int w;
  uint64_t mask_lo, mask_hi;
  uint64_t kconst;              // H(mask) ^ w ^ nonce
  // FracMinHash divisibility test (sks_hash.hpp DivTest)
  uint32_t low_mask, high_mask;  // x mod 2^s == 0 test (words)
  uint64_t dinv, dlim;           // odd part: x * d^-1 <= (2^64 - 1) / d
  // bottom-s pre-filter: keep fmh <= seg_thresh[seg]
  const uint64_t* seg_thresh;
  // output records: frac narrow key=C; frac wide key=lo val=hi;
  // bottom narrow key=C (fmh filled in by launch_fmh_narrow) val=C;
  // bottom wide key=fmh val=lo hi=hi
  uint64_t* out_key;
  uint64_t* out_val;
  uint64_t* out_hi;
  const uint64_t* seg_out_off;  // [n_seg] first record slot
  const uint64_t* seg_out_cap;  // [n_seg] record capacity
  unsigned long long* seg_count;    // [n_seg] records emitted (may exceed capacity)
  unsigned long long* seg_windows;  // [n_seg] valid windows hashed
  // dynamic tile queue (narrow scan): a zeroed counter, or null for static
  // per-workgroup tile ranges; `chunk` (set by launch_scan) tiles per grab
  unsigned long long* tile_queue;
  uint32_t chunk;
};

uint64_t scan_tiles_for(uint64_t seg_bytes);
hipError_t launch_scan(const ScanParams& p, int mode, int flavour, bool wide, int device,
                       hipStream_t stream, int grid_override);

}  // namespace sks
