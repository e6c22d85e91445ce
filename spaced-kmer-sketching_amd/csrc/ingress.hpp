// Device FASTA ingress (ingress.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_mem.hpp"

namespace sks {

// strings_from_fasta on the device: writes the host parser's record stream
// (fasta.cpp) to `out` and each record's '\n' position to rec_end (optional).
// out == nullptr: size query only.  *too_small: a capacity was short (nothing
// written).  Synchronises `s` twice (sizes are read back).
hipError_t fasta_parse_device(const uint8_t* raw, uint64_t n, uint8_t* out, uint64_t out_cap,
                              uint64_t* rec_end, uint64_t rec_cap, Scratch& work, Scratch& tmp,
                              hipStream_t s, uint64_t* out_bytes, uint64_t* n_records,
                              bool* too_small);

}  // namespace sks
