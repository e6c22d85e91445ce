// Dense per-window rows of a piece (windows.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sks {

// Every window of a piece dense by start (windows.hip): rows[i] = {kmer_bits
// lo, hi, masked lo(, masked hi for w > 32)} of the window starting at
// first + i, valid[i / 64] bit i % 64 set when that window is all ACGT.
hipError_t launch_windows_dense(const uint8_t* seq, uint64_t n_bytes, uint64_t first, uint64_t n_win, int w,
                                uint64_t m_lo, uint64_t m_hi, uint64_t* rows, uint64_t* valid, hipStream_t s);

}  // namespace sks
