/*
 * sks.h — C ABI of the MI355X spaced-k-mer sketch + ANI engine (libsks.so).
 *
 * Plain pointers and sizes only.  "d_" arguments are device (HBM) pointers on
 * the context's device; everything else is host memory owned by the caller.
 * Every entry point returns an sks_status (0 = OK); the message of the last
 * failure on the calling thread is available from sks_last_error().
 *
 * Each entry point names the reference interface it replaces
 * (bensonlzl/spaced-kmer-sketching @ 2024-10-22, paths under src/).
 * The reference is a source-level C++ API with no FFI; the C++ facade in
 * spaced-kmer-sketching_amd/cpp/ re-exposes the reference names on top of
 * this ABI (see INTEGRATION.md for the binding a maintainer would add).
 */
#ifndef SKS_H
#define SKS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKS_ABI_VERSION 3  /* 3: a join layout's boff row ends with one more word, the log2 of
                              the buckets per region, which the join reads: layouts built by
                              an ABI-2 library (rows without that word) must not be joined by
                              this one (round 5); later additions within 3 (new symbols
                              only): sks_sketch_set_downsample, sks_sketch_set_merge, sks_cluster,
                              sks_cluster_set, sks_gather, sks_gather_sets,
                              sks_ctx_set_gather_rounds, sks_search_topk,
                              sks_search_topk_sets, sks_sketch_set_filter,
                              sks_sketch_set_tally, sks_sketch_build_counted,
                              sks_sketch_set_has_abund, sks_sketch_set_device_abund,
                              sks_sketch_set_abund_copy, sks_sketch_set_abund_totals,
                              sks_sketch_set_abund_trim, sks_abund_pairs.  2: deduplicated join layout (masks, region
                              ends), elem_words on the layout entry points,
                              sks_ctx_set_join_check; later additions within 2 (new symbols
                              only): sks_ani_rows, sks_intersect_layout_ani, sks_host_alloc,
                              sks_host_free, sks_join_layout_stat_copy, sks_sketches_export,
                              sks_all_pairs_ani, sks_ctx_set_layout_blocks_hint,
                              sks_ctx_ani_table */

typedef enum sks_status {
  SKS_OK = 0,
  SKS_E_ARG = 1,         /* invalid argument (the reference has UB here)        */
  SKS_E_HIP = 2,         /* HIP runtime error / no device                        */
  SKS_E_IO = 3,          /* unreadable FASTA (reference: stderr + exit(1))       */
  SKS_E_NOMEM = 4,       /* host or device allocation failed                    */
  SKS_E_UNSUPPORTED = 5, /* valid in the reference, not implemented here (yet)   */
  SKS_E_LENGTH = 6       /* pair lists of different lengths (kmer_set.cpp:147)   */
} sks_status;

/* Sketch selection policy: the device-side replacement for the reference's
 * std::function<bool(const kmer)> sketching_cond (kmer.hpp:97, kmer_sliding.cpp:183),
 * which is a host callback and cannot run in a kernel. */
typedef enum sks_policy_kind {
  SKS_FRAC_MOD = 0, /* keep iff frac_min_hash(k) % param == 0 (kmer-sketching.cpp:30-34) */
  SKS_BOTTOM_S = 1  /* the `param` distinct k-mers with the smallest frac_min_hash
                       (ties by k-mer value) — build-defined, no reference equivalent */
} sks_policy_kind;

/* boost::hash_value(dynamic_bitset) flavour used by frac_min_hash (kmer.hpp:137-146).
 * The reference does not pin its Boost version; see DESIGN.md "hash parity". */
typedef enum sks_hash_flavour {
  SKS_HASH_BOOST_MIX = 0,   /* Boost >= 1.81: hash_combine = hash_mix(seed + 0x9e3779b9 + v) */
  SKS_HASH_BOOST_LEGACY = 1 /* Boost 1.71-1.80: MurmurHash2-style hash_combine_impl          */
} sks_hash_flavour;

typedef struct sks_policy {
  int32_t kind;    /* sks_policy_kind                                   */
  int32_t flavour; /* sks_hash_flavour                                  */
  uint64_t param;  /* SKS_FRAC_MOD: c (> 0); SKS_BOTTOM_S: s (> 0)       */
  int64_t nonce;   /* frac_min_hash nonce; the reference uses fmh(1)     */
} sks_policy;

/* ---- library ---------------------------------------------------------------- */
int sks_abi_version(void);
const char* sks_last_error(void);
/* "src:<16 hex digits>": hash of the sources this library was linked from
 * (spaced-kmer-sketching_amd/srchash.py); no reference counterpart. */
const char* sks_build_info(void);

/* ---- host helpers (no device needed) ---------------------------------------------- */
/* generate_random_spaced_seed_mask(w, k, seed) — kmer_bitset.cpp:132-152.
 * mask[0] = bits 0..63, mask[1] = bits 64..127.  1 <= k <= w <= 64. */
int sks_mask_generate(int window, int k, uint64_t seed, uint64_t mask[2]);
/* contiguous_kmer(l) — kmer_bitset.cpp:50-56 (l > 64 -> SKS_E_ARG like its runtime_error). */
int sks_mask_contiguous(int length, uint64_t mask[2]);
/* frac_min_hash::operator() — kmer.hpp:144-148 (kmer = masked canonical bits). */
uint64_t sks_frac_min_hash(const uint64_t kmer[2], const uint64_t mask[2], int window,
                           int64_t nonce, int flavour);
/* containment / binomial_estimator — ani_estimation.cpp:24-28, :38-42. */
double sks_containment(int intersection, int set_size);
double sks_binomial_estimator(double containment, int kmer_num_ones);
/* Vector form of kmer-sketching.cpp:195-200: cont[i] = containment(inter[i], size_first[i]),
 * ani[i] = binomial_estimator(cont[i], kmer_num_ones).  Either output may be NULL. */
int sks_ani_from_counts(const int32_t* inter, const int32_t* size_first, uint64_t n,
                        int kmer_num_ones, double* cont, double* ani);

/* ---- FASTA ingress (host) — fasta_processing.cpp:79-211 ----------------------------- */
typedef struct sks_fasta sks_fasta;
/* strings_from_fasta(): parses the file with the reference's record rules.
 * Unreadable file -> SKS_E_IO (the reference prints to stderr and exit(1)s). */
int sks_fasta_open(const char* path, sks_fasta** out);
void sks_fasta_close(sks_fasta* f);
uint64_t sks_fasta_num_records(const sks_fasta* f);
/* Record i's raw content (the i-th string of strings_from_fasta). */
int sks_fasta_record(const sks_fasta* f, uint64_t i, const uint8_t** data, uint64_t* len);
/* The record stream handed to the device: every record followed by one '\n'
 * separator (a non-ACGT byte, so k-mers never span records). */
const uint8_t* sks_fasta_stream(const sks_fasta* f);
uint64_t sks_fasta_stream_bytes(const sks_fasta* f);
/* cut_nucleotide_strings(): ACGT runs as codes 0..3 (one byte each).  Call with
 * NULL buffers to get *n_codes / *n_runs, then again with buffers that large. */
int sks_fasta_runs(const sks_fasta* f, uint8_t* codes, uint64_t* run_lens, uint64_t* n_codes,
                   uint64_t* n_runs);

/* ---- device context ---------------------------------------------------------------- */
typedef struct sks_ctx sks_ctx;
/* stream: a hipStream_t (may be NULL = the default stream).  Creating a context
 * loads every code object of the library on its device (one empty kernel per HIP
 * translation unit; ~30 ms the first time in a process), so that the first build
 * or join does not pay it inside the caller's timing. */
int sks_ctx_create(int device, void* stream, sks_ctx** out);
int sks_ctx_destroy(sks_ctx* ctx);
int sks_ctx_set_stream(sks_ctx* ctx, void* stream);
/* The device index the context was created on (-1 for NULL). */
int sks_ctx_device(const sks_ctx* ctx);
int sks_ctx_synchronize(sks_ctx* ctx);

/* Per-phase device times of the last sketch build / intersection on this
 * context, measured with hipEvents on the context's stream. */
typedef struct sks_timings {
  float scan_ms;      /* fused extract/canonicalise/hash/select kernel(s) */
  float post_ms;      /* sort + unique + bottom-s selection               */
  float total_ms;     /* whole call, first launch to last                 */
  uint64_t windows;   /* k-mer windows hashed                             */
  uint64_t scan_launches;
  uint64_t survivors; /* records emitted by the scan kernel               */
} sks_timings;
int sks_ctx_last_timings(const sks_ctx* ctx, sks_timings* out);

/* ---- sketch build: kmer_sliding.cpp:112-238 + kmer.hpp:135-190 + kmer_set.cpp:54-133 ---
 * d_seq: n_bytes of sequence bytes in device memory.  Non-ACGT bytes split runs
 * exactly as fasta_processing.cpp:144-179 does, so an sks_fasta stream can be
 * uploaded as is.  The bytes are cut into n_seg segments (genomes) by the host
 * array seg_off[n_seg + 1]; one sketch is built per segment (the reference
 * builds one kmer_set per FASTA file, kmer_set.cpp:112-133).
 * Result: an opaque device-resident sketch set (sorted unique canonical masked
 * k-mers per segment; one u64 word per k-mer when window <= 32, two (lo, hi)
 * when 32 < window <= 64). */
typedef struct sks_sketch_set sks_sketch_set;
int sks_sketch_build(sks_ctx* ctx, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off,
                     uint32_t n_seg, int window, const uint64_t mask[2], const sks_policy* policy,
                     sks_sketch_set** out);
/* Frees the set. Like hipFree, it first waits for all work queued on the
 * device; the arrays then go to a per-process block cache for later builds. */
int sks_sketch_set_free(sks_sketch_set* set);
/* Stream-ordered free (the hipFreeAsync contract): every use of the set must
 * be ordered before the current end of `stream` (a hipStream_t, NULL = the
 * null stream). Does not wait; the arrays are reused only once that point of
 * `stream` has completed. Lets several host threads build and free
 * concurrently without the device-wide wait of sks_sketch_set_free. */
int sks_sketch_set_free_on_stream(sks_sketch_set* set, void* stream);
uint32_t sks_sketch_set_num(const sks_sketch_set* set);
int sks_sketch_set_elem_words(const sks_sketch_set* set); /* 1 or 2 */
/* Host copies of per-sketch sizes (kmer_set::kmer_set_size, kmer.hpp:186-189)
 * and windows hashed per sketch. */
int sks_sketch_set_sizes(const sks_sketch_set* set, uint32_t* sizes);
int sks_sketch_set_windows(const sks_sketch_set* set, uint64_t* windows);
/* Device layout: sketch i = d_data()[start[i]*elem_words ...], sizes[i] elements. */
const uint64_t* sks_sketch_set_device_data(const sks_sketch_set* set);
const uint64_t* sks_sketch_set_device_starts(const sks_sketch_set* set);
const uint32_t* sks_sketch_set_device_sizes(const sks_sketch_set* set);
int sks_sketch_set_starts(const sks_sketch_set* set, uint64_t* starts);
/* Copy sketch i to host (sizes[i] * elem_words u64). */
int sks_sketch_set_copy(const sks_sketch_set* set, uint32_t i, uint64_t* out);
/* Write all sketches into a caller-owned fixed-stride device layout
 * (d_dst[i * stride * elem_words ...], d_sizes[i]) — the all-gather shape. */
int sks_sketch_set_export(const sks_sketch_set* set, uint64_t* d_dst, uint64_t stride,
                          uint32_t* d_sizes);

/* ---- persisted sketches (no reference equivalent) ------------------
 * A sketch set remembers how it was made; sks_sketch_set_save writes it with
 * that description to a self-checking file (format: csrc/persist.cpp) and
 * sks_sketch_set_load brings it back onto the context's device, ready for
 * sks_intersect_*.  A missing, truncated or corrupt file -> SKS_E_IO. */
typedef struct sks_sketch_info {
  int32_t window;
  int32_t elem_words;
  uint64_t mask[2];
  sks_policy policy;
  uint32_t n;
  int32_t has_names;
} sks_sketch_info;
int sks_sketch_set_info(const sks_sketch_set* set, sks_sketch_info* info);
/* names: n strings (e.g. the FASTA file names), or NULL to clear. */
int sks_sketch_set_set_names(sks_sketch_set* set, const char* const* names);
/* Name of sketch i, or NULL when the set has no names. */
const char* sks_sketch_set_name(const sks_sketch_set* set, uint32_t i);
/* A set with abundances (below) is written as file version 3, its abundances
 * between the elements and the names; any other set as version 1, byte for byte
 * as before version 3 existed.  Load reads both; a version-3 file with a zero
 * abundance, a short section or a bad checksum is SKS_E_IO. */
int sks_sketch_set_save(const sks_sketch_set* set, const char* path);
int sks_sketch_set_load(sks_ctx* ctx, const char* path, sks_sketch_set** out);
/* One set holding the sketches of sets[0], sets[1], ... in order (e.g. shards
 * sketched on different ranks or at different times).  All sets must share
 * window, mask and policy.  Abundances are carried when all sets have them; sets
 * of which only some have them are SKS_E_ARG naming "abundance". */
int sks_sketch_set_concat(sks_ctx* ctx, const sks_sketch_set* const* sets, uint32_t n_sets,
                          sks_sketch_set** out);
/* A coarser copy of `set` on the context's device, identical to what
 * sks_sketch_build would give for the same sequences with policy.param = param:
 *  SKS_FRAC_MOD: param must be a multiple of the set's param (else SKS_E_ARG
 *    naming "policy param"); keeps x iff frac_min_hash(x) % param == 0.
 *  SKS_BOTTOM_S: 0 < param <= the set's param (else SKS_E_ARG); every sketch keeps
 *    its min(param, size) elements smallest by (frac_min_hash, k-mer value).
 * Elements stay ascending and unique; window, mask, flavour, nonce, elem_words,
 * per-sketch windows and names are carried over; info.policy.param = param.
 * param equal to the set's gives a copy.  The source set is not modified.
 * A null ctx, set or out, param == 0 and a set on another device than the
 * context's are SKS_E_ARG; *out is NULL on every failure.
 * Waits for the context's stream once (it reads the new sizes back); the
 * elements are then written by a kernel queued on that stream, like the output
 * of every queued call (sks_ctx_synchronize waits for it; the source set may be
 * freed with sks_sketch_set_free at once). */
int sks_sketch_set_downsample(sks_ctx* ctx, const sks_sketch_set* set, uint64_t param, sks_sketch_set** out);
/* Grouped unions: a new set of n_groups sketches on the context's device, sketch
 * g the union of the source sketches members[group_off[g] .. group_off[g + 1]).
 * The source sketches are numbered as sks_sketch_set_concat orders them (set
 * 0's, then set 1's, ...).  group_off has n_groups + 1 non-decreasing entries
 * from 0; a source sketch may be listed in several groups, in none, or twice in
 * one; an empty group gives an empty sketch.  Elements are ascending (wide ones
 * by the 128-bit value) and unique, whatever the order of the members.  As the
 * elements are masked canonical k-mers kept on their own hash, the union of the
 * parts' sketches is the sketch of the parts taken together: the result equals
 * sks_sketch_build of the same sequences with one segment per group (parts
 * separated so that no window spans two, or cut with (window - 1)-base halos).
 * windows[g] is the sum of the listed members' windows; a member listed twice
 * counts twice.
 *  All sets must share window, mask, elem_words, policy kind, hash flavour and
 *  nonce (else SKS_E_ARG naming "window", "mask", "policy kind", "flavour" or
 *  "nonce").
 *  SKS_FRAC_MOD: and policy.param ("policy param").
 *  SKS_BOTTOM_S: sets of different s are allowed; the result's param is the
 *    smallest, and every sketch keeps its min(param, distinct elements) smallest
 *    by (frac_min_hash, k-mer value), the rule of sks_sketch_set_downsample.
 * The result carries the common window, mask, flavour and nonce and has no
 * names (sks_sketch_set_set_names).  The source sets are not modified.
 * SKS_E_ARG, decided on the host before anything is launched: a null ctx, sets,
 * out or set (before any device is touched), n_sets == 0, a null group_off or
 * members where entries are needed, a group_off that decreases or does not
 * start at 0, a member index >= the number of source sketches (the message
 * names the index), a set on another device than the context's.  A group whose
 * members' sizes sum to 2^32 or more is SKS_E_UNSUPPORTED.  *out is NULL on
 * every failure.
 * Waits for the context's stream once, to read the new sizes back, and once
 * more when a bottom-s sketch has to be cut; the elements are then written by a
 * kernel queued on that stream (sks_ctx_synchronize waits for it; the source
 * sets may be freed with sks_sketch_set_free at once). */
int sks_sketch_set_merge(sks_ctx* ctx, const sks_sketch_set* const* sets, uint32_t n_sets,
                         const uint32_t* group_off, const uint32_t* members, uint32_t n_groups,
                         sks_sketch_set** out);
/* Subtract or intersect: a new set on the context's device with `set`'s number
 * of sketches, sketch i holding the elements of `set`'s sketch i that are absent
 * from (SKS_FILTER_SUBTRACT) or present in (SKS_FILTER_INTERSECT) sketch
 * filter_of[i] of `filters`.  The elements keep the source order, so they stay
 * ascending and unique; wide elements are compared as whole 128-bit values.  As
 * the elements are masked canonical k-mers kept on their own hash, at one
 * FracMinHash scale the result is the sketch of the difference (intersection)
 * of the two k-mer sets, and every other call takes it.
 *  filter_of: a host array of set->n entries.  UINT32_MAX: sketch i is copied
 *    unchanged, whatever the kind.  Several sketches may name the same filter.
 *    NULL: every sketch uses filter 0, allowed only when `filters` holds exactly
 *    one sketch (else SKS_E_ARG).  filters == set is allowed.
 *  Carried over from `set`: window, mask, elem_words, the whole policy, per-sketch
 *    windows and names (sks_sketch_set_info of the result equals the source's).
 *    Neither input is modified.
 *  Both sets must be SKS_FRAC_MOD (a bottom-s set on either side is SKS_E_ARG
 *    naming "policy kind": the bottom-s sketch of a difference is not a part of
 *    the bottom-s sketches) and agree in window, mask, elem_words, hash flavour,
 *    nonce and policy param (else SKS_E_ARG naming "window", "mask",
 *    "elem_words", "flavour", "nonce" or "policy param"); nothing is
 *    downsampled implicitly.
 *  An empty source sketch gives an empty sketch; an empty filter sketch makes
 *    SUBTRACT copy and INTERSECT empty; a set of no sketches gives a set of none.
 * SKS_E_ARG, decided on the host before anything is launched: a null ctx, set,
 * filters or out (before any device is touched), an unknown kind, a filter_of[i]
 * that is neither UINT32_MAX nor below the filters' number of sketches (the
 * message names i and the index), a set on another device than the context's.
 * *out is NULL on every failure.
 * Waits for the context's stream once, to read the new sizes back; the elements
 * are then written by a kernel queued on that stream (sks_ctx_synchronize waits
 * for it; both inputs may be freed with sks_sketch_set_free at once). */
typedef enum sks_filter_kind {
  SKS_FILTER_SUBTRACT = 0,  /* keep x iff x is not in the filter sketch */
  SKS_FILTER_INTERSECT = 1  /* keep x iff x is in the filter sketch     */
} sks_filter_kind;
int sks_sketch_set_filter(sks_ctx* ctx, const sks_sketch_set* set, const sks_sketch_set* filters,
                          const uint32_t* filter_of, int kind, sks_sketch_set** out);
/* Grouped tallies: how many of a group's sketches hold each k-mer.  Sets,
 * group_off, members and n_groups are exactly as sks_sketch_set_merge takes them
 * (source sketches numbered in concat order; a sketch may be listed in several
 * groups or in none; an empty group gives an empty sketch).  A new set of
 * n_groups sketches on the context's device: with cnt_g(x) the number of listed
 * members of group g that hold x, sketch g holds the values x with
 *   max(min_count[g], 1) <= cnt_g(x) <= max_count[g].
 * A member listed twice counts twice (the rule merge has for windows).  Elements
 * are ascending (wide ones by the 128-bit value) and unique, whatever the order
 * of the members.  min 1 and no maximum is the union (sks_sketch_set_merge's
 * result); min = max = the number of members is the strict core; 1 .. 1 the
 * k-mers unique to one member; ceil(0.9 m) .. none the 90 % core.
 *  min_count, max_count: host arrays of n_groups entries.  min_count NULL: 1 for
 *    every group.  max_count NULL, or an entry UINT32_MAX: no upper limit.  A
 *    max_count[g] below the effective minimum gives an empty sketch, no error.
 *  d_counts: NULL, or device memory of counts_cap u32 values.  Entry
 *    starts[g] + j of it (starts as sks_sketch_set_starts of the result) receives
 *    cnt_g of element j of sketch g, written by a kernel queued on the context's
 *    stream.  A counts_cap below the result's total number of elements is
 *    SKS_E_LENGTH (*out NULL, the contents of d_counts unspecified); the sum of
 *    the listed members' sizes, over all groups, always suffices.
 *  Carried over: window, mask, elem_words and the whole policy
 *    (sks_sketch_set_info of the result equals the sources' but for the number of
 *    sketches and the names); windows[g] is the sum of the listed members'
 *    windows.  The result has no names.  No input is modified.
 *  All sets must be SKS_FRAC_MOD (a bottom-s set is SKS_E_ARG naming "policy
 *    kind": whether a bottom-s sketch holds a value depends on that sketch's
 *    other values, so absence from it says nothing) and agree in window, mask,
 *    elem_words, hash flavour, nonce and policy param (else SKS_E_ARG naming
 *    "window", "mask", "elem_words", "policy kind", "flavour", "nonce" or "policy
 *    param"); nothing is downsampled implicitly.
 * SKS_E_ARG, decided on the host before anything is launched, as
 * sks_sketch_set_merge words them: a null ctx, sets, out or set (before any
 * device is touched), n_sets == 0, a null group_off or members where entries are
 * needed, a group_off that decreases or does not start at 0, a member index >=
 * the number of source sketches (the message names the index), a set on another
 * device than the context's.  A group whose members' sizes sum to 2^32 or more
 * is SKS_E_UNSUPPORTED.  *out is NULL on every failure.
 * Costs what the merge of the same groups costs: the same rounds, and a last
 * pass that reads two more elements per distinct value.  Waits for the
 * context's stream once, to read the new sizes back; the elements and d_counts
 * are then written by a kernel queued on that stream (sks_ctx_synchronize waits
 * for it; the source sets may be freed with sks_sketch_set_free at once). */
int sks_sketch_set_tally(sks_ctx* ctx, const sks_sketch_set* const* sets, uint32_t n_sets,
                         const uint32_t* group_off, const uint32_t* members, uint32_t n_groups,
                         const uint32_t* min_count, const uint32_t* max_count,
                         sks_sketch_set** out, uint32_t* d_counts, uint64_t counts_cap);

/* ---- k-mer abundances: counted sketch sets ---------------------------------------------
 * A sketch set may carry one more column, the abundance of every element: how
 * often its k-mer was selected in the sequence the sketch was built from.  Only
 * sks_sketch_build_counted, sks_sketch_set_abund_trim, sks_sketch_set_load (of a
 * counted set's file) and sks_sketch_set_concat (of counted sets) return a set
 * with abundances.  Every other call takes a counted set as it takes any set:
 * its results are those of the set without the column, and a set it returns
 * (downsample, merge, filter, tally) has no abundances.
 *
 * sks_sketch_build that also counts.  abund(x, g) = the number of selected windows of segment g
 * whose canonical masked k-mer is x, i.e. x's multiplicity in sks_kmer_list_build's list of
 * segment g.  Sketch g keeps x iff max(min_abund, 1) <= abund(x, g) <= max_abund
 * (max_abund == UINT32_MAX: no limit; max_abund below the minimum: empty sketches, no error).
 * Counts are clamped to UINT32_MAX.  SKS_FRAC_MOD only: SKS_BOTTOM_S is SKS_E_UNSUPPORTED
 * naming "policy kind".  With min_abund <= 1 and no limit, the elements, sizes, starts and
 * windows are bit for bit those of sks_sketch_build.  windows[g] never depends on the limits.
 * Every other argument, check and message as sks_sketch_build.  sks_ctx_last_timings filled
 * as for a build; sks_ctx_last_build_path is SKS_BUILD_PATH_GENERAL. */
int sks_sketch_build_counted(sks_ctx* ctx, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off,
                             uint32_t n_seg, int window, const uint64_t mask[2], const sks_policy* policy,
                             uint32_t min_abund, uint32_t max_abund, sks_sketch_set** out);

int sks_sketch_set_has_abund(const sks_sketch_set* set);                 /* 1 / 0 (0 for NULL) */
/* u32[total], entry starts[i] + j = abundance (>= 1) of element j of sketch i; NULL when none */
const uint32_t* sks_sketch_set_device_abund(const sks_sketch_set* set);
/* sizes[i] values to the host (SKS_E_ARG naming "abundance" for a set without them) */
int sks_sketch_set_abund_copy(const sks_sketch_set* set, uint32_t i, uint32_t* out);
/* totals[i] = the sum of sketch i's abundances (u64), n host values; waits for the device.
 * SKS_E_ARG naming "abundance" for a set without them. */
int sks_sketch_set_abund_totals(const sks_sketch_set* set, uint64_t* totals);

/* A new counted set: the elements of `set` (which must have abundances, else SKS_E_ARG naming
 * "abundance") with max(min_abund,1) <= abundance <= max_abund, order kept, abundances carried.
 * Window, mask, policy, windows and names carried over, as sks_sketch_set_filter does.
 * Identity: build_counted(.., lo, hi) == trim(build_counted(.., 1, UINT32_MAX), lo, hi).
 * SKS_E_ARG, decided on the host before any device is touched: a null ctx, set or out, a set
 * on another device than the context's.  *out is NULL on every failure.  Waits for the
 * context's stream once, to read the new sizes back; the elements and abundances are then
 * written by a kernel queued on that stream. */
int sks_sketch_set_abund_trim(sks_ctx* ctx, const sks_sketch_set* set, uint32_t min_abund, uint32_t max_abund,
                              sks_sketch_set** out);

/* Weighted overlap of n_pairs sketch pairs.  For pair p, with A = sketch d_a[p] of `samples` and
 * B = sketch d_b[p] of `refs`: d_shared[p] = |A ∩ B| and
 * d_weight[p] = sum of A's abundances over A ∩ B (u64).  d_a / d_b / outputs are device arrays,
 * queued on the context's stream, no host wait.  `samples` must have abundances.  `refs` need not,
 * and refs' own abundances are ignored.  refs == samples is allowed.  Compatibility: the checks
 * and messages of sks_gather_sets (both SKS_FRAC_MOD, same window, mask, elem_words, flavour,
 * nonce and policy param).  An index >= the set's number of sketches (or below 0) cannot be
 * seen by the host: the kernel writes shared = -1, weight = 0 for that pair and reads nothing.
 * weight / shared is the mean depth of the shared k-mers.  weight / totals[a] is the share of
 * the sample's k-mer mass inside the reference.  The result does not depend on the order in
 * which the device runs the pairs (no atomics).
 * SKS_E_ARG, decided on the host before any device is touched: a null ctx or set, n_pairs > 0
 * with a null array, a set on another device than the context's. */
int sks_abund_pairs(sks_ctx* ctx, const sks_sketch_set* samples, const sks_sketch_set* refs, const int32_t* d_a,
                    const int32_t* d_b, uint64_t n_pairs, int32_t* d_shared, uint64_t* d_weight);

/* ---- ordered k-mer lists: nucleotide_string_list_to_kmers (kmer_sliding.cpp:112-238) ---
 * Every selected window of every segment, in stream order, duplicates kept —
 * the reference's vector<kmer>.  Same inputs as sks_sketch_build; the policy
 * must be SKS_FRAC_MOD (the per-k-mer predicate; param 1 keeps every window).
 * Element i: window start byte positions[i] and bits[4i..4i+3] = kmer_bits
 * (lo, hi), masked_bits (lo, hi) of the reference's `kmer` (kmer.hpp:75-86):
 * kmer_bits is the chosen strand's window register — R (2w bits), or F, which
 * in the reference keeps up to 64 bases of the run ending at the window. */
typedef struct sks_kmer_list sks_kmer_list;
int sks_kmer_list_build(sks_ctx* ctx, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off,
                        uint32_t n_seg, int window, const uint64_t mask[2], const sks_policy* policy,
                        sks_kmer_list** out);
int sks_kmer_list_free(sks_kmer_list* list);
uint64_t sks_kmer_list_total(const sks_kmer_list* list);
/* counts[n_seg]: k-mers per segment (the list is segment 0's, then segment 1's, ...). */
int sks_kmer_list_counts(const sks_kmer_list* list, uint64_t* counts);
const uint64_t* sks_kmer_list_device_positions(const sks_kmer_list* list);
const uint64_t* sks_kmer_list_device_bits(const sks_kmer_list* list);
/* Host copies; either pointer may be NULL. */
int sks_kmer_list_copy(const sks_kmer_list* list, uint64_t* positions, uint64_t* bits);

/* Every window of a record-stream piece, dense by start position, for a HOST
 * predicate: the window sequence nucleotide_string_to_kmers hands to its
 * std::function<bool(const kmer)> (kmer_sliding.cpp:144-183), without any
 * selection.  Row i describes the window starting at byte first + i of d_seq
 * (i < n_windows): {kmer_bits lo, hi, masked_bits lo} for window <= 32 (3
 * words), {kmer_bits lo, hi, masked_bits lo, hi} for window > 32 (4 words);
 * bit i % 64 of d_valid[i / 64] is set when all its bytes are ACGT (case-
 * insensitive; any other byte ends a run, fasta_processing.cpp:144-179) — the
 * rows of invalid windows are unspecified.  kmer_bits is the canonical window
 * with the reference's 128-bit history (up to 64 bases of the run), so a caller
 * cutting a stream into pieces passes min(first_of_piece, 64 - window) bytes
 * of history before `first`.  Queued on the context stream (no host sync). */
int sks_windows_dense(sks_ctx* ctx, const uint8_t* d_seq, uint64_t n_bytes, uint64_t first, uint64_t n_windows,
                      int window, const uint64_t mask[2], uint64_t* d_rows, uint64_t* d_valid);
/* Words per row of sks_windows_dense: 3 (window <= 32) or 4. */
int sks_windows_dense_row_words(int window);

/* ---- intersection: kmer_set.cpp:23-41, :143-184 ----------------------------------
 * Sketches in device memory: sketch i = d_data[d_starts[i]*elem_words ...],
 * d_sizes[i] elements, each sorted ascending and unique (as built above). */
/* Pair list (compute_pairwise_kmer_set_intersections): d_out[p] = |S[a[p]] ∩ S[b[p]]|. */
int sks_intersect_pairs(sks_ctx* ctx, const uint64_t* d_data, const uint64_t* d_starts,
                        const uint32_t* d_sizes, int elem_words, const int32_t* d_a,
                        const int32_t* d_b, uint64_t n_pairs, int32_t* d_out);
/* All ordered pairs of a row block (generate_all_pairs_from_vector, generators.hpp:44-58):
 * d_out[(i - row_begin) * n + j] = |S[i] ∩ S[j]| for row_begin <= i < row_end, 0 <= j < n. */
int sks_intersect_all(sks_ctx* ctx, const uint64_t* d_data, const uint64_t* d_starts,
                      const uint32_t* d_sizes, int elem_words, uint32_t n, uint32_t row_begin,
                      uint32_t row_end, int32_t* d_out);

/* Symmetric all-vs-all for sharding across devices: the n x n matrix is cut
 * into 64 x 64 tiles and the upper-triangle tiles (I <= J, row-major, count
 * sks_intersect_sym_tiles(n)) in [tile_begin, tile_end) are computed; each
 * count is written to both d_out[i * n + j] and d_out[j * n + i] of the n x n
 * int32 matrix, which the call zeroes first.  Summing the matrices of calls
 * that together cover [0, sks_intersect_sym_tiles(n)) gives the full
 * generate_all_pairs_from_vector result (e.g. an all-reduce over ranks). */
uint64_t sks_intersect_sym_tiles(uint32_t n);
int sks_intersect_sym(sks_ctx* ctx, const uint64_t* d_data, const uint64_t* d_starts,
                      const uint32_t* d_sizes, int elem_words, uint32_t n, uint64_t tile_begin,
                      uint64_t tile_end, int32_t* d_out);

/* ---- sketch union (no reference equivalent) --------------------------------------------
 * Sorted unique union of n u64 k-mers (any order, duplicates allowed): e.g. the
 * FracMinHash sketches of chunks of one genome cut with (w-1)-base halos, whose
 * union is the genome's sketch (FracMinHash keeps a k-mer on its own hash).
 * d_out holds n values; *n_out (host) = distinct values.  Narrow (w <= 32) only. */
int sks_sketch_union(sks_ctx* ctx, const uint64_t* d_in, uint64_t n, uint64_t* d_out,
                     uint64_t* n_out);
/* The same for 32 < w <= 64: n 128-bit k-mers as (lo, hi) word pairs (2n words),
 * ordered by the 128-bit value like the reference's operator< on kmer_bitset.
 * d_in / d_out 16-byte aligned (SKS_E_ARG otherwise). */
int sks_sketch_union_wide(sks_ctx* ctx, const uint64_t* d_in, uint64_t n, uint64_t* d_out,
                          uint64_t* n_out);

/* ---- join layout: all-vs-all across GPUs ------------------------------------------------
 * The all-pairs join kernel (sks_intersect_all / _sym, SKS_INTERSECT_JOIN) reads
 * a "join layout": blocks of 64 consecutive sketches, each DISTINCT value of a
 * block stored once with a 64-bit mask of the block's sketches holding it
 * (bit s = sketch 64 * block + s).  Buckets are two-level: G =
 * sks_join_layout_groups(log_b) value groups cut by bounds (G + 1 values of
 * elem_words words each, non-decreasing, bounds[0] = 0, bounds[G] = the
 * largest value), each split into 8 (or 2^log_b when log_b < 3) hash buckets;
 * 2^rg consecutive groups form a region (NR = regions per block; the build
 * picks rg in 1..3 by its size: 8-group regions when the blocks give >= 1024
 * of them, smaller ones for small builds).  A region's entries start at its
 * raw offset in the block (the block's sketch elements in earlier regions),
 * so its tail up to the next region is unused.  Exposing the
 * layout lets a multi-GPU caller build the layout of its own sketches only and
 * all-gather layouts instead of raw sketches (no replicated build):
 *   vals   u64[total * elem_words]  entry values, block-major (total = sum of sizes)
 *   masks  u64[total]               sketch mask of each entry
 *   boff   u32[nb * sks_join_layout_boff_words(log_b)]  per block (nb = ceil(n/64)):
 *          2^log_b bucket starts, then NR region ends, relative to bstart[block]
 *          (room for G), and in the row's last word log2 of the buckets per region
 *   bstart u64[nb + 1]              raw block starts (prefix of the sizes); [nb] = total
 * Layouts of consecutive sketch ranges that each start at a multiple of 64 can
 * be concatenated (append vals/masks/boff and add the data offset to bstart)
 * when they were built with the same bounds.  elem_words: 1 (u64 k-mers,
 * w <= 32) or 2 ((lo, hi) k-mers, 32 < w <= 64). */
/* log_b for a largest sketch of max_sketch_size elements (all ranks must agree). */
uint32_t sks_join_layout_log_b(uint32_t max_sketch_size);
/* Block-bucket population (entries) one join chunk holds; larger buckets are
 * joined in sub-chunks (exact, slower). */
uint32_t sks_join_layout_capacity(void);
/* log2 of the value groups per region that a layout build of n_blocks blocks
 * (of 64 sketches) with 2^log_b buckets takes in this process (0..3; a region's
 * buckets: min(2^log_b, 8 groups' worth)).  Read-only; for tests and diagnostics. */
uint32_t sks_join_layout_region_log(uint32_t n_blocks, uint32_t log_b);
/* How this process cuts a join call of `tiles` tiles over a layout of 2^log_b
 * buckets: workgroups per tile and whole tiles per launch (either may be NULL).
 * Read-only; for tests and diagnostics.  Returns SKS_E_ARG for log_b > 14. */
int sks_join_launch_plan(uint64_t tiles, uint32_t log_b, uint32_t* n_groups, uint64_t* tiles_per_launch);
/* Value groups of a layout with 2^log_b buckets (bounds hold groups + 1 values). */
uint32_t sks_join_layout_groups(uint32_t log_b);
/* Words of one block's boff row: 2^log_b bucket starts + room for the region
 * ends + the region size word (the row's last word, log2 of the buckets per
 * region; added in ABI 3 — rows of ABI-2 layouts are one word shorter). */
uint32_t sks_join_layout_boff_words(uint32_t log_b);
/* Group bounds fixed by the mask alone (host array of (groups + 1) * elem_words
 * words): the quantiles of min(F & M, R & M) for random sequence, so every rank
 * of a multi-GPU all-vs-all uses the same bounds without sampling or
 * exchanging anything.  Any bounds give exact counts; these balance groups for
 * genome-like (near-uniform) k-mers. */
int sks_join_layout_bounds_for_mask(const uint64_t mask[2], uint32_t log_b, int elem_words, uint64_t* bounds);
/* Group bounds balanced for the set (quantiles averaged over up to 64 sample
 * sketches), queued on the context stream.  Any bounds give exact counts. */
int sks_join_layout_bounds(sks_ctx* ctx, const uint64_t* d_data, const uint64_t* d_starts,
                           const uint32_t* d_sizes, int elem_words, uint32_t n, uint32_t log_b,
                           uint64_t* d_bounds);
/* Builds the layout of sketches (d_data, d_starts, d_sizes)[0, n) into caller
 * buffers (three launches: bounds + block starts, group positions, placement).
 * d_bounds: the group bounds (NULL: the set's own, sks_join_layout_bounds).
 * *max_block_bucket (host) receives the largest block-bucket population in
 * entries, or UINT32_MAX when the build could not place a group (only for
 * adversarial 128-bit values; the layout is then invalid) — it waits for the
 * build; NULL skips that read-back.  total_hint: the n sizes' sum when the
 * caller knows it (the build then never waits for the stream), UINT64_MAX to
 * have the sizes read back. */
int sks_join_layout_build(sks_ctx* ctx, const uint64_t* d_data, const uint64_t* d_starts,
                          const uint32_t* d_sizes, int elem_words, uint32_t n, uint64_t total_hint,
                          uint32_t log_b, const uint64_t* d_bounds, uint64_t* d_out_vals,
                          uint64_t* d_out_masks, uint32_t* d_out_boff, uint64_t* d_out_bstart,
                          uint32_t* max_block_bucket);
/* Queues a copy of the last sks_join_layout_build's two status words on this
 * context — [0] the largest block-bucket population, [1] non-zero when the
 * layout is invalid (see max_block_bucket) — into d_dst (2 x u32, device), so
 * a caller that skips the read-back can check the layout after the join
 * without a stream round trip.  Call it right after the build. */
/* Region-size hint for the next sks_join_layout_build calls on this context:
 * the number of 64-sketch blocks that actually hold sketches (0, the default:
 * every block does).  A build over a buffer with many empty rows — a rank's
 * exchange buffer, a slot per rank — then picks the region size (workgroups
 * per block) for its real work.  The layout's content does not depend on it. */
int sks_ctx_set_layout_blocks_hint(sks_ctx* ctx, uint32_t blocks);
int sks_join_layout_stat_copy(sks_ctx* ctx, uint32_t* d_dst);
/* sks_intersect_sym over a join layout of n sketches: upper-triangle 64x64 tiles
 * [tile_begin, tile_end) into the n x n int32 matrix d_out (zeroed first). */
int sks_intersect_sym_layout(sks_ctx* ctx, uint32_t n, uint32_t log_b, int elem_words, const uint64_t* d_vals,
                             const uint64_t* d_masks, const uint32_t* d_boff, const uint64_t* d_bstart,
                             uint64_t tile_begin, uint64_t tile_end, int32_t* d_out);

/* Tiles of the n x n matrix over a join layout whose block 0 is global block
 * blk0 (a rank's own blocks, or a gathered layout with blk0 = 0); every tile's
 * two blocks must lie in the layout.  Tiles: d_tiles == NULL -> upper-triangle
 * tiles [tile_begin, tile_end) (row-major, sks_intersect_sym_tiles; blk0 must
 * be 0, else SKS_E_ARG); else the list d_tiles[2t] = I, d_tiles[2t + 1] = J
 * (I <= J, global block indices) for t in [tile_begin, tile_end).  packed == 0:
 * counts are ADDED to the n x n int32 matrix d_out at (i, j) and (j, i);
 * packed != 0: to d_out[(t - tile_begin) * 4096 + r * 64 + c] for row I*64 + r,
 * column J*64 + c (a diagonal tile holds both triangles).  The caller zeroes
 * d_out.  A multi-GPU caller counts the tiles of its own blocks on its own
 * layout while the others' layouts are still being gathered. */
int sks_intersect_layout_tiles(sks_ctx* ctx, uint32_t n, uint32_t log_b, int elem_words, const uint64_t* d_vals,
                               const uint64_t* d_masks, const uint32_t* d_boff, const uint64_t* d_bstart,
                               uint32_t blk0, const uint32_t* d_tiles, uint64_t tile_begin,
                               uint64_t tile_end, int packed, int32_t* d_out);

/* sks_intersect_layout_tiles with the row blocks and the column blocks in two
 * layouts (built with the same bounds): tile (I, J) of the list joins row block
 * I of the row layout (whose block 0 is global block r_blk0) with column block
 * J of the column layout (block 0 = c_blk0).  A multi-GPU caller joins its own
 * layout with each peer's as the peer's sketches arrive. */
int sks_intersect_layout_pair_tiles(sks_ctx* ctx, uint32_t n, uint32_t log_b, int elem_words,
                                    const uint64_t* d_rvals, const uint64_t* d_rmasks, const uint32_t* d_rboff,
                                    const uint64_t* d_rbstart, uint32_t r_blk0, const uint64_t* d_cvals,
                                    const uint64_t* d_cmasks, const uint32_t* d_cboff, const uint64_t* d_cbstart,
                                    uint32_t c_blk0, const uint32_t* d_tiles, uint64_t tile_begin,
                                    uint64_t tile_end, int packed, int32_t* d_out);
/* sks_intersect_layout_pair_tiles fused with containment / ANI — the count
 * loop, the containment / binomial_estimator loop and the host result vector of
 * kmer-sketching.cpp:185-200 (ani_estimation.cpp:24-42) in one launch: counts
 * are added to d_out as there (packed or both halves of the n x n matrix; the
 * caller zeroes d_out), and as each tile's last workgroup finishes, it writes
 *   ani[i * n + j] = binomial_estimator(containment(|S_i ∩ S_j|, d_sizes[i]), kmer_num_ones)
 * for both orientations (i, j) and (j, i) of every pair of the tile (the
 * diagonal tile's own pairs once).  d_sizes[i] = |S_i| (int32, n entries, by
 * global genome index).  ani: n * n doubles in device memory, or pinned host
 * memory (sks_host_alloc, or any hipHostMalloc'd buffer): the kernel then
 * writes the host matrix itself, so the transfer runs while later tiles are
 * counted.  Cells of tiles not in the list are left untouched.  d_tiles ==
 * NULL: the upper-triangle tiles [tile_begin, tile_end) of ONE layout
 * (rows == cols, r_blk0 = c_blk0 = 0). */
int sks_intersect_layout_ani(sks_ctx* ctx, uint32_t n, uint32_t log_b, int elem_words,
                             const uint64_t* d_rvals, const uint64_t* d_rmasks, const uint32_t* d_rboff,
                             const uint64_t* d_rbstart, uint32_t r_blk0, const uint64_t* d_cvals,
                             const uint64_t* d_cmasks, const uint32_t* d_cboff, const uint64_t* d_cbstart,
                             uint32_t c_blk0, const uint32_t* d_tiles, uint64_t tile_begin, uint64_t tile_end,
                             int packed, int32_t* d_out, const int32_t* d_sizes, int kmer_num_ones, double* ani);
/* sks_sketch_set_export for sketches given as device arrays (e.g. a received
 * shard): d_dst[i * stride * elem_words ...] = sketch i padded with ~0 words,
 * d_dst_sizes[i] = d_sizes[i]; queued on the context stream, no wait.  Every
 * d_sizes[i] must be <= stride (the caller's bound; larger sketches are cut). */
int sks_sketches_export(sks_ctx* ctx, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                        int elem_words, uint32_t n, uint64_t* d_dst, uint64_t stride, uint32_t* d_dst_sizes);
/* The whole "comparison" of kmer-sketching.cpp:185-200 in one call, for one
 * process and one device: every ordered pair of the n sketches (d_data,
 * d_starts, d_sizes — e.g. a set's device arrays) counted over a join layout
 * of all of them (built in context scratch), and, when ani != NULL, their
 * containment / ANI written by the join as in sks_intersect_layout_ani
 * (ani[i * n + j], n * n doubles in device or pinned host memory).
 * d_counts: the packed upper-triangle tiles [sks_intersect_sym_tiles(n)][64][64]
 * int32 (sks_intersect_layout_tiles' packed format; the call clears them, the
 * caller need not), or NULL to keep them in scratch.  max_size: the largest sketch (sizes the buckets); total: the sizes'
 * sum (or an upper bound).  d_status (device, 2 x u32, may be NULL) receives the
 * layout's status words (sks_join_layout_stat_copy).  Queued on the context
 * stream; nothing waits.  sks_ctx_last_intersect_ms then times the join launch
 * alone. */
int sks_all_pairs_ani(sks_ctx* ctx, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                      int elem_words, uint32_t n, uint32_t max_size, uint64_t total, int kmer_num_ones,
                      double* ani, int32_t* d_counts, uint32_t* d_status);
/* One rank's step of a multi-GPU all-vs-all (sks_dist.all_vs_all_join) in one
 * call: the join layout of the n sketches (context scratch; group bounds
 * d_bounds, or sampled when NULL; blocks_hint as sks_ctx_set_layout_blocks_hint)
 * whose block 0 is global block blk0, then the join of the n_tiles global
 * (I, J) tiles of d_tiles (u32 pairs, both blocks in this set) into the packed
 * d_counts[n_tiles][64][64], and — ani non-NULL — containment / ANI of both
 * orientations written into the n_global x n_global matrix ani (device or
 * mapped pinned host memory), with |S_g| = d_sizes_global[g] for global genome
 * g.  The counts, the tiles' finisher counters and the two status words
 * (d_status, as sks_join_layout_build's: max block bucket, invalid) are
 * cleared by the build itself: four launches, no memset, no host sync.
 * Replaces per tile kmer_set.cpp:23-41 over kmer_set.cpp:167-184's pairs. */
int sks_layout_tiles_ani(sks_ctx* ctx, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                         int elem_words, uint32_t n, uint64_t total, uint32_t log_b, const uint64_t* d_bounds,
                         uint32_t blocks_hint, uint32_t blk0, const uint32_t* d_tiles, uint64_t n_tiles,
                         uint32_t n_global, const int32_t* d_sizes_global, int kmer_num_ones, double* ani,
                         int32_t* d_counts, uint32_t* d_status);
/* ---- query-vs-reference search (no reference equivalent) -------------------------------
 * "Which of these stored sketches contain my queries?": every query sketch
 * against every reference sketch, with only the pairs that pass the thresholds
 * coming back, as a compact list instead of a dense matrix.  The query set's
 * join layout is built once (context scratch); the references are taken in
 * batches of whole 64-sketch blocks, each batch's layout built with the query
 * layout's log_b and group bounds and joined with it into packed count tiles
 * (scratch), which a filter kernel turns into hit records on the device.
 * Scratch is bounded by the query layout, one batch's layout and tiles, and
 * the hit buffers, whatever the size of the reference set. */
typedef struct sks_hit {       /* 32 bytes */
  uint32_t query, ref;         /* indices into the two sets                       */
  int32_t  shared;             /* |Q_query ∩ R_ref|                               */
  int32_t  query_size;         /* |Q_query|                                       */
  double   containment;        /* containment(shared, query_size)                 */
  double   ani;                /* binomial_estimator(containment, kmer_num_ones)  */
} sks_hit;
/* Device-array form: queries (d_q_*) and references (d_r_*) as in the
 * intersection entry points, with n sketches, the largest sketch (max_size) and
 * the sizes' sum (total, or an upper bound) of each side.  (q, r) is a hit iff
 * shared >= max(min_shared, 1) and containment(shared, |Q_q|) >= min_containment
 * (the query is the first set of the pair, kmer-sketching.cpp:195-200; pairs
 * sharing nothing are never hits).  Hits are written to d_hits (device, hit_cap
 * records) in ascending (query, ref) order, each pair once; *n_hits (host)
 * always receives the exact number of hits.  d_hits == NULL is a size query;
 * *n_hits > hit_cap -> SKS_E_LENGTH, the contents of d_hits then unspecified.
 * The call waits for the stream (it reads the count back); the final sort into
 * d_hits is queued on it.  >= 2^32 elements on a side -> SKS_E_UNSUPPORTED, and
 * so is a layout the build could not place (adversarial 128-bit values): no
 * hit is reported from an invalid layout. */
int sks_search(sks_ctx* ctx, const uint64_t* d_q_data, const uint64_t* d_q_starts, const uint32_t* d_q_sizes,
               uint32_t q_n, uint32_t q_max_size, uint64_t q_total, const uint64_t* d_r_data,
               const uint64_t* d_r_starts, const uint32_t* d_r_sizes, uint32_t r_n, uint32_t r_max_size,
               uint64_t r_total, int elem_words, int kmer_num_ones, double min_containment, int32_t min_shared,
               sks_hit* d_hits, uint64_t hit_cap, uint64_t* n_hits);
/* The same for two sketch sets (queries == refs is allowed).  Both must share
 * window, mask, elem_words, policy kind, hash flavour and nonce, and for
 * SKS_FRAC_MOD the policy param (bottom-s sets of different s may be compared);
 * a mismatch is SKS_E_ARG naming the field.  kmer_num_ones = popcount(mask) / 2;
 * the group bounds are the mask-derived ones (sks_join_layout_bounds_for_mask);
 * if a layout cannot be placed with them, the search runs once more with
 * bounds sampled from the references before giving up. */
int sks_search_sets(sks_ctx* ctx, const sks_sketch_set* queries, const sks_sketch_set* refs,
                    double min_containment, int32_t min_shared, sks_hit* d_hits, uint64_t hit_cap,
                    uint64_t* n_hits);
/* Diagnostics: 64-sketch reference blocks per batch of sks_search (0, the
 * default: the engine's choice, which keeps a batch's count tiles within 256 MiB). */
int sks_ctx_set_search_batch(sks_ctx* ctx, uint32_t ref_blocks);

/* ---- the k best references per query (no reference equivalent) --------------------------
 * "For each of my sketches, which k references are closest, best first?"  The
 * output has a fixed size, q_n * k records, so there is no size query, no sort
 * of hits and no second pass: the layouts, the reference batches and the joins
 * into count tiles are those of sks_search, and a selection kernel keeps, per
 * query, a sorted list of k slots across the batches (q_n * k * 16 bytes of
 * context scratch), which a last kernel expands into records.
 * score(q, r) is containment(shared, denominator), shared = |Q_q ∩ R_r|, with
 * the denominator rank_kind names: the query's size (what sks_search thresholds
 * on), the reference's (a reference inside a metagenome), or the smaller of the
 * two (what sks_cluster links on).
 * Eligibility: reference r is listed for query q only if shared >=
 * max(min_shared, 1), score >= min_score, and, with skip_same_index set, r != q
 * (the k-NN graph of one set passed as both sides).  A pair sharing nothing is
 * never listed; an empty sketch has an empty list and is in nobody's list.
 * Order: strict and total — the larger score first (compared as the doubles
 * containment returns), ties to the larger shared, then to the smaller ref.
 * The k best of a strict total order are unique: the result does not depend on
 * the batch size, on the order in which tiles arrive or on anything else about
 * the run.
 * Output: d_hits[q * k + j] (device, q_n * k records) is the j-th best of query
 * q for j < d_counts[q]; the remaining slots hold {query = q, ref = UINT32_MAX,
 * rank = j, everything else 0}.  d_counts[q] (device, q_n x u32, may be NULL) is
 * the number of filled slots.  Every slot of every query is written on success,
 * also when r_n == 0; q_n == 0 writes nothing and returns SKS_OK.
 * ani is ani_of(shared, denominator), the function the search's hit filter
 * uses: with SKS_RANK_QUERY, (shared, query_size, score, ani) of a record are
 * the same bits as (shared, query_size, containment, ani) of the sks_hit that
 * sks_search_sets reports for that pair.
 * Checked on the host before anything is launched: null ctx (before any device
 * is touched), null d_hits with q_n > 0, k == 0, NaN min_score, unknown
 * rank_kind, elem_words not 1 or 2, kmer_num_ones <= 0, null arrays where
 * entries are needed -> SKS_E_ARG; k > SKS_TOPK_MAX -> SKS_E_UNSUPPORTED
 * (naming "k"); the limits on elements and blocks are those of sks_search.  A
 * layout the build could not place -> SKS_E_UNSUPPORTED ("invalid layout"), the
 * contents of d_hits and d_counts then unspecified.
 * Everything is queued on the context's stream; the call waits once, at the
 * end, to read the layouts' status words.  Reference batches follow
 * sks_ctx_set_search_batch and the 256 MiB tile budget, as in sks_search.
 * sks_ctx_last_intersect_ms then times the whole call. */
typedef enum sks_rank_kind {
  SKS_RANK_QUERY = 0,  /* score = containment(shared, |Q_q|)               */
  SKS_RANK_REF   = 1,  /* score = containment(shared, |R_r|)               */
  SKS_RANK_MAX   = 2   /* score = containment(shared, min(|Q_q|, |R_r|))   */
} sks_rank_kind;
#define SKS_TOPK_MAX 64
typedef struct sks_top_hit {   /* 40 bytes */
  uint32_t query, ref;         /* ref == UINT32_MAX: an empty slot                    */
  int32_t  shared;             /* |Q_query ∩ R_ref|                                   */
  int32_t  query_size, ref_size;
  uint32_t rank;               /* position in the query's list, 0 = best              */
  double   score;              /* as rank_kind says                                   */
  double   ani;                /* binomial_estimator(score, kmer_num_ones)            */
} sks_top_hit;
/* Device-array form: queries and references exactly as sks_search takes them
 * (group bounds sampled from the references). */
int sks_search_topk(sks_ctx* ctx, const uint64_t* d_q_data, const uint64_t* d_q_starts, const uint32_t* d_q_sizes,
                    uint32_t q_n, uint32_t q_max_size, uint64_t q_total, const uint64_t* d_r_data,
                    const uint64_t* d_r_starts, const uint32_t* d_r_sizes, uint32_t r_n, uint32_t r_max_size,
                    uint64_t r_total, int elem_words, int kmer_num_ones, int rank_kind, uint32_t k,
                    double min_score, int32_t min_shared, int skip_same_index, sks_top_hit* d_hits,
                    uint32_t* d_counts);
/* The same for two sketch sets (queries == refs is allowed), with the
 * compatibility rules and messages of sks_search_sets (bottom-s sets of
 * different s may be compared) and its bounds: the mask-derived ones first,
 * once more with bounds sampled from the references if a layout cannot be
 * placed with them. */
int sks_search_topk_sets(sks_ctx* ctx, const sks_sketch_set* queries, const sks_sketch_set* refs, int rank_kind,
                         uint32_t k, double min_score, int32_t min_shared, int skip_same_index,
                         sks_top_hit* d_hits, uint32_t* d_counts);

/* ---- single-linkage clusters (no reference equivalent) ---------------------------------
 * "Which of these sketches are the same thing?": the connected components of the
 * graph that links two sketches i != j of one set iff, with shared = |S_i ∩ S_j|,
 *   shared >= max(min_shared, 1)  and
 *   max(containment(shared, |S_i|), containment(shared, |S_j|)) >= min_containment
 * (containment as everywhere else: a double division), which is to say iff
 * sks_search_sets(set, set, min_containment, min_shared) reports (i, j) or
 * (j, i).  An empty sketch shares nothing and is a cluster of its own;
 * min_containment <= 0 links every pair sharing max(min_shared, 1) k-mers; a
 * min_containment no pair can meet gives n clusters of one.
 * The result is canonical, whatever the order in which links are found:
 * clusters are numbered 0 .. C-1 by ascending smallest member, so sketch 0 is in
 * cluster 0.  d_cluster[i] (device, n x u32) is the cluster of sketch i;
 * d_rep[c] (device, room for n x u32, C written) the representative of cluster
 * c, its member with the most elements, ties to the smallest index; either may
 * be NULL.  *n_clusters (host) receives C.
 * The set's join layout is built once (context scratch) and joined with itself,
 * the tiles on or above the diagonal only, in batches of whole columns of
 * 64-sketch blocks (sks_ctx_set_search_batch; by default a batch's count tiles
 * stay within 256 MiB); a kernel turns each batch's tiles into unions in a
 * parent array.  Scratch depends on n and on one batch, never on the number of
 * linked pairs, and only the labels leave the device.
 * Device-array form: the set as in the intersection entry points, with the
 * largest sketch (max_size) and the sizes' sum (total, or an upper bound); group
 * bounds are sampled from the set.  kmer_num_ones is taken for symmetry with
 * sks_search only: the rule is on containment.  Checked on the host, leaving
 * *n_clusters = 0: null ctx (before any device is touched), null n_clusters,
 * NaN min_containment, elem_words not 1 or 2, kmer_num_ones <= 0 -> SKS_E_ARG;
 * total >= 2^32 -> SKS_E_UNSUPPORTED; n == 0 -> SKS_OK and 0 clusters.  A layout
 * the build could not place (adversarial 128-bit values) -> SKS_E_UNSUPPORTED
 * ("invalid layout"), 0 clusters: nothing is linked from such a layout.
 * The call waits for the stream once, to read C back; the labels and
 * representatives are written by kernels queued before that wait.
 * sks_ctx_last_intersect_ms then times the whole call. */
int sks_cluster(sks_ctx* ctx, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                uint32_t n, uint32_t max_size, uint64_t total, int elem_words, int kmer_num_ones,
                double min_containment, int32_t min_shared, uint32_t* d_cluster, uint32_t* d_rep,
                uint32_t* n_clusters);
/* The same for a sketch set (null set, or a set on another device than the
 * context -> SKS_E_ARG).  The group bounds are the mask-derived ones
 * (sks_join_layout_bounds_for_mask); if the layout cannot be placed with them,
 * the call runs once more with bounds sampled from the set before giving up. */
int sks_cluster_set(sks_ctx* ctx, const sks_sketch_set* set, double min_containment, int32_t min_shared,
                    uint32_t* d_cluster, uint32_t* d_rep, uint32_t* n_clusters);

/* ---- gather: greedy min-set cover of a query (no reference equivalent) ------------------
 * "This sample is a mixture: which references does it contain, each counted only
 * for what the earlier ones did not explain?"  Q is one query sketch, R_0 ..
 * R_{n-1} reference sketches over the same k-mer space (ascending, unique
 * elements; with elem_words 2 ordered by the 128-bit value, hi first).  With
 * thr = max(min_shared, 1) and Q_rem = Q, every round computes
 * new_r = |Q_rem ∩ R_r| for every r and picks the r with the largest new_r, ties
 * to the smallest index.  If that new_r < thr, or max_rounds rounds have been
 * reported (0: no limit), the call stops; otherwise r is reported and
 * Q_rem <- Q_rem \ R_r.  Hits come out in round order; no reference is reported
 * twice.  Every value is an integer or one double division of integers, so the
 * result is exact and deterministic.
 * Near-identical references all pass a containment threshold of sks_search;
 * gather reports one of them and the rest drop out, nothing of theirs being
 * left to explain.
 * The call finds, once, the position in Q of every reference element (scratch
 * of O(q_size + r_total) words on the context), then runs the rounds on the
 * device over a bitmap of Q's unexplained elements, queued in groups
 * (sks_ctx_set_gather_rounds) with one host wait per group and one after the
 * membership pass.  sks_ctx_last_intersect_ms then times the whole call. */
typedef struct sks_gather_hit {  /* 32 bytes */
  uint32_t ref;         /* index into the references                                          */
  int32_t  shared;      /* |Q ∩ R_ref|, with the whole query                                  */
  int32_t  shared_new;  /* |Q_rem ∩ R_ref| when chosen: the elements this round explains       */
  int32_t  ref_size;    /* |R_ref|                                                            */
  double   f_query_new; /* containment(shared_new, |Q|)                                       */
  double   ani;         /* binomial_estimator(containment(shared, ref_size), kmer_num_ones)   */
} sks_gather_hit;
/* Device-array form: the query's q_size elements at d_q (device), the references
 * as in sks_search (r_max_size is taken for symmetry with it; r_total is the
 * sizes' sum or an upper bound; sizes adding up to more -> SKS_E_ARG).
 * *n_hits (host) always receives the exact number of rounds, *n_unexplained
 * (host, may be NULL) |Q_rem| at the end.  d_hits (device, hit_cap records) may be
 * NULL: a size query.  *n_hits > hit_cap -> SKS_E_LENGTH, the contents of d_hits
 * then unspecified.  min(r_n, q_size) records always suffice.
 * Checked on the host, leaving *n_hits = 0: null ctx (before any device is
 * touched), null n_hits, elem_words not 1 or 2, kmer_num_ones <= 0, null arrays
 * where entries are needed -> SKS_E_ARG; r_total >= 2^32 (or 2^31 query elements
 * or references) -> SKS_E_UNSUPPORTED; q_size == 0 or r_n == 0 -> SKS_OK, 0 hits. */
int sks_gather(sks_ctx* ctx, const uint64_t* d_q, uint32_t q_size, const uint64_t* d_r_data,
               const uint64_t* d_r_starts, const uint32_t* d_r_sizes, uint32_t r_n, uint32_t r_max_size,
               uint64_t r_total, int elem_words, int kmer_num_ones, int32_t min_shared, uint32_t max_rounds,
               sks_gather_hit* d_hits, uint64_t hit_cap, uint64_t* n_hits, uint32_t* n_unexplained);
/* The same for sketch `q` of `queries` (q >= its number -> SKS_E_ARG) against the
 * set `refs`.  Both sets must share window, mask, elem_words, policy kind, hash
 * flavour, nonce and policy param (the checks and messages of sks_search_sets),
 * and both must be SKS_FRAC_MOD: a bottom-s set is SKS_E_ARG naming "policy
 * kind", because subtraction only means something when every sketch samples the
 * same hash space.  Both sets must live on the context's device.
 * kmer_num_ones = popcount(mask) / 2. */
int sks_gather_sets(sks_ctx* ctx, const sks_sketch_set* queries, uint32_t q, const sks_sketch_set* refs,
                    int32_t min_shared, uint32_t max_rounds, sks_gather_hit* d_hits, uint64_t hit_cap,
                    uint64_t* n_hits, uint32_t* n_unexplained);
/* Diagnostics: rounds of sks_gather queued per host wait (0, the default: the
 * engine's choice, gather_plan.hpp). */
int sks_ctx_set_gather_rounds(sks_ctx* ctx, uint32_t rounds_per_wait);

/* Pinned host memory the device reads and writes directly (mapped into every
 * device's address space): the destination of a fused ANI matrix.  coherent:
 * fine-grained (every device store goes to the host as issued); 0: coarse-
 * grained (device stores are cached and written back by the end of the kernel,
 * in whole lines).  No reference counterpart (the reference's result vectors
 * are plain host vectors, kmer-sketching.cpp:193). */
int sks_host_alloc(uint64_t bytes, int coherent, void** out);
/* ANI by shared-element count for sets of `size` elements, kept on the context:
 * table[x] = binomial_estimator(containment(x, size), kmer_num_ones) for x in
 * [0, size] (the same device function as the fused conversion, so the same
 * doubles).  The fused ANI of sks_intersect_layout_ani / sks_all_pairs_ani then
 * reads a row whose set holds `size` elements from the table instead of
 * evaluating pow (bottom-s sets: every row).  Queued on the context stream;
 * rebuilt only when (size, kmer_num_ones) changes; sizes above
 * SKS_ANI_TABLE_MAX (or 0) drop the table.  sks_all_pairs_ani calls it with its
 * max_size. */
#define SKS_ANI_TABLE_MAX (1u << 20)
int sks_ctx_ani_table(sks_ctx* ctx, uint32_t size, int kmer_num_ones);
int sks_host_free(void* p);
/* The set's sketches back to back (sizes[i] * elem_words words each, in order)
 * and its sizes, copied into caller device buffers (a send buffer). */
int sks_sketch_set_export_csr(const sks_sketch_set* set, uint64_t* d_data, uint32_t* d_sizes);

/* ---- containment / ANI on the device: kmer-sketching.cpp:195-200 + ani_estimation.cpp:24-42 ----
 * d_ani[i * n + j] = binomial_estimator(containment(counts[i][j], |S_i|), kmer_num_ones)
 * for the n x n count matrix (|S_i| = counts[i][i]); d_cont (may be NULL) the
 * containments.  Queued on the context stream. */
int sks_ani_matrix(sks_ctx* ctx, const int32_t* d_counts, uint32_t n, int kmer_num_ones, double* d_cont,
                   double* d_ani);
/* Rows [row_begin, row_end) of sks_ani_matrix (same addressing: d_ani[i * n + j]),
 * so a caller can convert and copy out the rows an all-pairs call has finished
 * (rows of tile rows [0, I) are final once those tile rows are counted) while
 * later tiles are still being counted. */
int sks_ani_rows(sks_ctx* ctx, const int32_t* d_counts, uint32_t n, uint32_t row_begin, uint32_t row_end,
                 int kmer_num_ones, double* d_cont, double* d_ani);
/* Packed tiles (d_packed [n_tiles][64][64] of tiles d_tiles[2t] = I,
 * d_tiles[2t + 1] = J, as sks_intersect_layout_tiles writes them):
 * d_ani[t][0][r][c] = ANI of (64 I + r, 64 J + c), d_ani[t][1][c][r] = ANI of
 * (64 J + c, 64 I + r); d_sizes[i] = |S_i| (int32). */
int sks_ani_tiles(sks_ctx* ctx, const int32_t* d_packed, const uint32_t* d_tiles, uint64_t n_tiles, uint32_t n,
                  const int32_t* d_sizes, int kmer_num_ones, double* d_ani);

/* ---- FASTA ingress (device) — fasta_processing.cpp:79-133 on the GPU ------------------
 * d_raw: the n_raw bytes of one FASTA file in device memory (the host only reads
 * the file).  Writes to d_stream exactly the bytes sks_fasta_stream() holds for
 * the same file (records in order, each followed by one '\n'), and, when
 * d_rec_end is non-NULL, the stream position of record i's '\n' to d_rec_end[i].
 * *stream_bytes / *n_records always receive the sizes; d_stream == NULL is a
 * size query.  Capacity too small -> SKS_E_LENGTH, nothing written.  Output is
 * at most n_raw + 1 bytes.  Returns after the sizes are known; the copy kernels
 * are queued on the context stream. */
int sks_fasta_parse_device(sks_ctx* ctx, const uint8_t* d_raw, uint64_t n_raw, uint8_t* d_stream,
                           uint64_t stream_cap, uint64_t* d_rec_end, uint64_t rec_cap,
                           uint64_t* stream_bytes, uint64_t* n_records);
/* Device time (ms) of the last sks_fasta_parse_device call (waits for it). */
int sks_ctx_last_ingress_ms(sks_ctx* ctx, float* ms);

/* ---- diagnostics / tuning ------------------------------------------------------------- */
/* Device time (ms) between the first and last launch of the last
 * sks_intersect_* call on this context (waits for it to finish). */
int sks_ctx_last_intersect_ms(sks_ctx* ctx, float* ms);
/* Fix the scan kernel's persistent grid size (0 = derive from occupancy). */
int sks_ctx_set_scan_grid(sks_ctx* ctx, int grid);
/* Post-processing of a build of ONE FracMinHash genome with window <= 32.  By
 * default such a build takes the fused path when the expected survivors fit
 * its buckets: the survivors are split by their top key bits into `buckets`
 * regions of `bucket_capacity` keys, sorted and uniqued per bucket and gathered
 * on the device, with one host round trip per build.  GENERAL forces the
 * device-wide sort + unique every other build uses, FUSED takes the fused path
 * even when the SKS_NO_FRAC_FUSED environment variable is set.  For tests,
 * bucket_capacity and buckets (a power of two) lower the path's own choices
 * (0: keep them; larger values are clamped): a bucket that receives more keys
 * than its capacity is a status, after which the general post-processing runs
 * on the same scan records.  Every path gives identical sketches. */
enum {
  SKS_FRAC_POST_AUTO = 0,
  SKS_FRAC_POST_GENERAL = 1,
  SKS_FRAC_POST_FUSED = 2
};
int sks_ctx_set_frac_post(sks_ctx* ctx, int mode, uint32_t bucket_capacity, uint32_t buckets);
/* The path the context's last sks_sketch_build took (-1 for NULL). */
enum {
  SKS_BUILD_PATH_GENERAL = 0,
  SKS_BUILD_PATH_FUSED = 1,                   /* fused FracMinHash post-processing */
  SKS_BUILD_PATH_FUSED_THEN_GENERAL_POST = 2  /* its status was raised: general post-processing, same scan */
};
int sks_ctx_last_build_path(const sks_ctx* ctx);
/* Kernel used by sks_intersect_all / sks_intersect_sym for u64 sketches.  All
 * give identical counts; AUTO (default) = the LDS hash join when the bucket
 * sizes allow it, else the LDS merge tiles, else one wavefront per pair.
 * (Round 3's block-postings and range-join kernels were measured slower than
 * the hash join on every workload and removed) */
enum {
  SKS_INTERSECT_AUTO = 0,
  SKS_INTERSECT_MERGE = 1,    /* 64x64 tiles of pairwise LDS merges */
  SKS_INTERSECT_JOIN = 2,     /* 64x64 tiles, LDS hash join of the two blocks */
  SKS_INTERSECT_GLOBAL = 3    /* one wavefront per pair, straight from HBM */
};
int sks_ctx_set_intersect_kernel(sks_ctx* ctx, int kind);
/* Diagnostics: on != 0 switches the context's join-layout builds and join
 * launches to instrumented kernels that check, per element, the invariants the
 * counts rest on (the layout's deduplication: every element's representative
 * holds its value; the join table: every inserted value is found naming its
 * own entry).  sks_ctx_join_check_violations waits for the context's stream
 * and returns (and resets) the violations counted on the device since the
 * last call; a correct build counts 0. */
int sks_ctx_set_join_check(sks_ctx* ctx, int on);
int sks_ctx_join_check_violations(sks_ctx* ctx, uint64_t* violations);

/* ---- synthetic genomes (bench / test utility; no reference equivalent) ----------------- */
/* Fills d_out[0..n) with ACGT bytes: base(p) = splitmix64(seed ^ (p * golden)) >> 62;
 * if mut_rate > 0 a position mutates with probability mut_rate. */
int sks_synth_bases(sks_ctx* ctx, uint8_t* d_out, uint64_t n, uint64_t seed, uint64_t mut_seed,
                    double mut_rate, uint64_t pos_offset);

#ifdef __cplusplus
}
#endif
#endif /* SKS_H */
