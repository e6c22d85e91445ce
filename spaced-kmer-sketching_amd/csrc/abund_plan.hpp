// The arithmetic of k-mer abundances (no HIP: tests/cpp/abund_plan_test.cpp runs
// it on any machine, and abund.hip runs the same functions on the device): the
// keep rule of a counted build and of a trim, the length of a run of equal
// sorted keys from the runs' first indices and the segment's end, and the padded
// size of a sketch file's abundance section.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SKS_ABUND_HD __host__ __device__
#else
#define SKS_ABUND_HD
#endif

namespace sks {

constexpr uint32_t kAbundNoLimit = 0xffffffffu;  // max_abund: no upper limit (UINT32_MAX)

// ---- the keep rule -----------------------------------------------------------------------
// An element of abundance a (>= 1) stays iff max(min_abund, 1) <= a <= max_abund.
// max_abund == UINT32_MAX is no limit, also for a count clamped to UINT32_MAX; a
// max_abund below the minimum keeps nothing.
SKS_ABUND_HD inline uint32_t abund_floor(uint32_t min_abund) { return min_abund < 1u ? 1u : min_abund; }
SKS_ABUND_HD inline bool abund_keeps(uint32_t a, uint32_t min_abund, uint32_t max_abund) {
  return a >= abund_floor(min_abund) && a <= max_abund;
}
// whether the limits keep every element (the build then needs no trim pass)
SKS_ABUND_HD inline bool abund_keeps_all(uint32_t min_abund, uint32_t max_abund) {
  return min_abund <= 1u && max_abund == kAbundNoLimit;
}

// ---- run lengths -------------------------------------------------------------------------
// A segment's sorted records are [seg_begin, seg_end) of one array; its distinct
// values have the ranks [rank_begin, rank_end) of the array's distinct values and
// run_start[r] is the index of the first record of the run of rank r.  The run
// of rank r ends where the next run of the segment begins, or at the segment's
// end if it is the segment's last: O(1) per distinct value, whatever the length.
SKS_ABUND_HD inline uint64_t abund_run_end(const uint64_t* run_start, uint64_t r, uint64_t rank_end,
                                           uint64_t seg_end) {
  return r + 1 < rank_end ? run_start[r + 1] : seg_end;
}
SKS_ABUND_HD inline uint32_t abund_clamp(uint64_t len) {
  return len > (uint64_t)kAbundNoLimit ? kAbundNoLimit : (uint32_t)len;
}
SKS_ABUND_HD inline uint32_t abund_run_length(const uint64_t* run_start, uint64_t r, uint64_t rank_end,
                                              uint64_t seg_end) {
  return abund_clamp(abund_run_end(run_start, r, rank_end, seg_end) - run_start[r]);
}

// ---- the sketch file's section -----------------------------------------------------------
// uint32 abund[total], zero-padded to a multiple of 8 bytes
SKS_ABUND_HD inline uint64_t abund_section_bytes(uint64_t total) { return (total * 4u + 7u) & ~(uint64_t)7; }

}  // namespace sks
