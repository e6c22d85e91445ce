// Post-processing of scan records and the small utility kernels (post.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "build_plan.hpp"
#include "device_mem.hpp"

namespace sks {

// Sort each CSR segment of keys ascending (optionally carrying values).
// keys/vals are sorted in place via the alt buffers; results land in `*_out`.
hipError_t seg_sort_keys(const uint64_t* keys_in, uint64_t* keys_out, uint64_t total,
                         const std::vector<uint64_t>& host_off, const uint64_t* d_off,
                         int end_bit, Scratch& tmp, hipStream_t s);
hipError_t seg_sort_pairs(const uint64_t* keys_in, uint64_t* keys_out, const uint64_t* vals_in,
                          uint64_t* vals_out, uint64_t total, const std::vector<uint64_t>& host_off,
                          const uint64_t* d_off, int end_bit, Scratch& tmp, hipStream_t s);

// Maximal runs of set bits of a 64-bit k-mer mask. Masked k-mers only have
// mask bits set, so gathering those bits into the low popcount(mask) bits
// (a pext) is order-preserving and injective: the post-scan sorts then run
// ceil(popcount / 8) radix passes instead of ceil(top bit / 8)
// (config 3, w=31/k=21: 42 bits instead of 62, 6 passes instead of 8).
// The gather runs as Hacker's Delight's compress / expand butterfly (7-4,
// 7-5): six masks of bits moving right by 1, 2, 4, ... 32, computed on the host,
// so a pack is at most six and/xor/shift/or steps on SGPR constants (a
// 2-bit-granular k-mer mask never moves a bit by an odd amount: five).
struct BitRuns {
  uint32_t n = 0;    // runs of set bits of the mask; 0: not packed (identity)
  uint64_t mask = 0;
  uint64_t mv[6] = {0, 0, 0, 0, 0, 0};
};
BitRuns bit_runs(uint64_t mask);
hipError_t launch_bits_expand(uint64_t* keys, uint64_t n, const BitRuns& runs, hipStream_t s);
// Bottom-s post-processing per genome in one workgroup (post.hip
// k_bottom_fused): genomes of <= bottom_fused_capacity() candidates.
// d_res[g] = sketch size; ~0: fewer than s distinct candidates under a finite
// threshold (retry); kBottomOverflow: d_cnt[g] > d_cap[g] (the scan dropped
// records; d_cap may be null when the counts are known to fit).  max_cnt: a
// bound of every d_cnt[g] (or of d_cap[g]) below the capacity.  set_sizes /
// set_starts (may be null): the sketch set's device arrays, written per genome
// (size, dst_off[g]) so a build needs no host round trip before them.
constexpr uint64_t kBottomOverflow = ~1ull;
uint32_t bottom_fused_capacity();
hipError_t launch_bottom_fused(uint64_t* rec, const uint64_t* d_src_off, const uint64_t* d_cnt,
                               const uint64_t* d_retry_ok, const uint64_t* d_dst_off,
                               uint32_t n_seg, uint64_t max_cnt, uint64_t s_param, int key_bits,
                               const BitRuns& runs, uint64_t kconst, int flavour, uint64_t* out,
                               uint64_t* d_res, hipStream_t s, const uint64_t* d_cap = nullptr,
                               uint32_t* set_sizes = nullptr, uint64_t* set_starts = nullptr);

// FracMinHash post-processing of one narrow genome without a host round trip
// (post.hip k_frac_partition / k_frac_sort_unique / k_frac_gather): the
// d_cnt[0] <= d_cap[0] records at rec[0 ..) are packed, split by their top
// log_b bits into 2^log_b regions of bucket_cap keys (regions: 2^log_b *
// bucket_cap words), sorted and uniqued per bucket, and the distinct keys
// written to out[0 ..) (capacity `cap` >= d_cap[0]) with set_sizes[0],
// set_starts[0] and d_res = {distinct size, status}.  A non-zero status
// (kFracStatus*) means a capacity was short and `out` is not the sketch; the
// records are untouched.  d_cnt[0] > d_cap[0] yields size 0, status 0.
// state: frac_state_bytes() of device words, zeroed once by the caller and left
// zeroed (cursors, status) by every complete launch.
constexpr uint64_t kFracStatusBucket = 1;  // a bucket received more than bucket_cap keys
constexpr uint64_t kFracStatusCrowd = 2;   // keys crowd one sub-bucket of a bucket's sort
uint32_t frac_bucket_capacity();           // keys one bucket's workgroup sorts (largest bucket_cap)
uint32_t frac_max_log_buckets();           // largest log_b
size_t frac_state_bytes();
hipError_t launch_frac_fused(const uint64_t* rec, const uint64_t* d_cnt, const uint64_t* d_cap, uint64_t cap,
                             int key_bits, const BitRuns& runs, uint32_t log_b, uint32_t bucket_cap,
                             uint64_t* regions, uint32_t* state, uint64_t* out, uint32_t* set_sizes,
                             uint64_t* set_starts, uint64_t* d_res, hipStream_t s);

// Compact sparse survivor regions [off[g], off[g] + cnt[g]) into dense CSR,
// packing each value's mask bits when `pack` is given.  tag_shift >= 0 ORs the
// segment index in above the key bits, (g << tag_shift) | key: the segments of a
// many-genome build then sort as ONE device-wide radix sort over
// tag_shift + seg_tag_bits(n_seg) bits (each segment keeps its CSR range, as the
// counts per tag are the segment sizes) instead of a segmented sort, whose one
// workgroup per segment left most of the chip idle (64 genomes of 25k keys:
// 0.5 ms per sort).  The tag is dropped on output (seg_unique_scatter's keep
// masks; runs_expand keeps only the packed width).
hipError_t compact_regions(const uint64_t* src, uint64_t* dst, const uint64_t* d_src_off,
                           const uint64_t* d_dst_off, uint32_t n_seg, uint64_t max_len,
                           hipStream_t s, const BitRuns* pack = nullptr, int tag_shift = -1);
// out[off[g] .. off[g+1]) = g: the segment of every element (a segment tag
// that does not fit above the key rides as a sort value instead)
hipError_t launch_seg_ids(uint64_t* out, const uint64_t* d_off, uint32_t n_seg, uint64_t max_len, hipStream_t s);

// Per-segment unique of sorted keys (optionally by a (key, key2) pair):
// writes d_flag_pos (exclusive scan of "first of run" flags) and per-segment
// unique counts d_uniq[g].  Keys equal in key (and key2 when non-null) are
// one element.
// max_len: longest segment (sizes the grid; segments are grid-strided).
hipError_t seg_unique_scan(const uint64_t* keys, const uint64_t* keys2, uint64_t total,
                           uint64_t max_len, const uint64_t* d_off, uint32_t n_seg, uint32_t* d_flag,
                           uint64_t* d_pos, uint64_t* d_uniq, Scratch& tmp, hipStream_t s);
hipError_t sort_unique_u64(const uint64_t* in, uint64_t n, uint64_t* out, uint64_t* n_out,
                           Scratch& tmp, hipStream_t s);
hipError_t sort_unique_u128(const uint64_t* in, uint64_t n, uint64_t* out, uint64_t* n_out,
                            Scratch& tmp, hipStream_t s);
// Scatter the first `limit[g]` unique elements of each segment:
// out[dst_off[g] + rank] = vals[i] (and out2 from vals2 when non-null).
// limit == nullptr keeps every unique element; dst_off == nullptr places
// segment g at pos[off[g]] (the global unique rank, i.e. dense CSR output).
hipError_t seg_unique_scatter(const uint64_t* vals, const uint64_t* vals2, uint64_t total,
                              uint64_t max_len, const uint64_t* d_off, uint32_t n_seg,
                              const uint32_t* d_flag,
                              const uint64_t* d_pos, const uint64_t* d_limit,
                              const uint64_t* d_dst_off, uint64_t* out, uint64_t* out2,
                              hipStream_t s, const BitRuns* expand = nullptr, uint64_t keep = ~0ull,
                              uint64_t keep2 = ~0ull);

// ---- misc kernels -------------------------------------------------------------------------
hipError_t launch_synth(uint8_t* out, uint64_t n, uint64_t seed, uint64_t mut_seed,
                        uint64_t mut_thresh, uint64_t pos_offset, hipStream_t s);
hipError_t launch_export(const uint64_t* data, const uint64_t* starts, const uint32_t* sizes,
                         uint32_t n, int elem_words, uint64_t* dst, uint64_t stride,
                         uint32_t* dst_sizes, hipStream_t s);
// nucleotide_string_to_kmers' `kmer` for each selected window start pos[i]
// (kmer_sliding.cpp:112-186): out[4i..4i+3] = kmer_bits (lo, hi), masked_bits
// (lo, hi).  kmer_bits is the chosen strand's window register: R (2w bits), or
// F holding up to 64 bases of the run ending at the window (the reference
// never clears F's older bases).  seg_begin: [n_seg] sorted segment starts.
hipError_t launch_materialise(const uint8_t* seq, const uint64_t* seg_begin, uint32_t n_seg,
                              const uint64_t* pos, uint64_t n, int w, uint64_t mask_lo,
                              uint64_t mask_hi, uint64_t* out, hipStream_t s);
hipError_t launch_iota(uint64_t* out, uint64_t n, hipStream_t s);
// Bottom-s from C-sorted distinct candidates (uk, segment g at [uoff[g], uoff[g+1])):
// writes the min(limit[g], n_g) k-mers with the smallest (fmh, k-mer), in k-mer
// order, to out + dst[g].  Needs every n_g with limit[g] > 0 to be at most
// bottom_select_capacity().
uint32_t bottom_select_capacity();
hipError_t launch_bottom_select(const uint64_t* uk, const uint64_t* d_uoff, const uint64_t* d_dst,
                                const uint64_t* d_lim, uint32_t n_seg, uint64_t kconst,
                                int flavour, uint64_t* out, hipStream_t s);
// keys[i] = frac_min_hash of the narrow canonical k-mer keys[i] (in place).
hipError_t launch_fmh_narrow(uint64_t* keys, uint64_t n, uint64_t kconst, int flavour, hipStream_t s);
hipError_t launch_gather(const uint64_t* src, const uint64_t* idx, uint64_t n, uint64_t* out,
                         hipStream_t s);
hipError_t launch_interleave(const uint64_t* lo, const uint64_t* hi, uint64_t n, uint64_t* out,
                             hipStream_t s);

}  // namespace sks
