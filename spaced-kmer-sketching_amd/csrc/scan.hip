// Kernel 1 — fused spaced-seed sketch scan for gfx950.
//
// One pass over the sequence bytes computes, for every window start, exactly
// what the reference's hot loop computes (kmer_sliding.cpp:112-186):
//   forward window F  (kmer_sliding.cpp:26-31:  F <<= 2; F[0..1] = base)
//   reverse-complement window R (:42-47: R >>= 2; R[2w-2..2w-1] = base ^ 3)
//   canonical C = min(F & M, R & M), ties -> R & M (same value)   (:159-175)
//   fmh = H(C) ^ H(M) ^ w ^ nonce   (kmer.hpp:141-148, boost hash flavour)
// and applies the selection policy (FracMinHash `fmh % c == 0`, or the
// bottom-s pre-filter `fmh <= threshold`) in the same kernel.  List mode
// (nucleotide_string_list_to_kmers) applies the FracMinHash test and emits the
// window's start position instead of the k-mer (materialised later in order).  Bytes that are
// not A/C/G/T (either case) split runs exactly like
// fasta_processing.cpp:144-179; a window is valid iff all its w bytes are
// ACGT and lie inside its segment, so k-mers never span runs or genomes.
//
// Structure (MI355X): persistent grid, each workgroup streams a contiguous
// range of 4096-window tiles.  A tile's bytes arrive with 16-B coalesced
// loads (prefetched one tile ahead into registers), are packed once into
// 2-bit words in LDS (a big-endian stream for F, a complemented little-endian
// stream for R, a 1-bit invalid map).  The narrow kernel's lane (g, r) — r the
// low 4 bits of the thread index, g the rest — then owns the 16 window starts
// 16 (16 g + m) + r, m = 0..15: 16 bases apart, so consecutive windows of a
// lane share a 32-bit word of F and of R and each window costs one new funnel
// shift (v_alignbit_b32) per strand, by a per-lane constant amount.  (The wide
// kernel's lanes own 16 consecutive starts.)  The narrow kernel keeps its segment
// cursor and the segment's geometry in scalar registers (SegCursor), read from
// memory only when the cursor moves, and prefetches a tile that lies whole
// inside its segment from a scalar base plus the lane's constant offset.
// Survivors (~1/c of windows) go to an LDS queue flushed with one global
// atomic per flush, so the global counters see a few thousand atomics per
// launch instead of one per survivor; a survivor that finds the queue full is
// written directly, its slot taken with one global atomic per wave
// (wave_aggregated_inc).  The pre-filter kernel first queues its candidates
// (1 window in 2^min(s,4)) per wave: a passing lane takes its 16-byte slot with
// a returning LDS atomic on the wave's cursor word, which holds the next free
// slot's LDS address; a scalar count follows the cursor and the list is
// finished 64 candidates at a time.
// For w <= 31 the canonical minimum of the narrow FracMinHash and bottom-s
// kernels is one v_min_f64 on the bit patterns (min_below_2_62).
// This unit is compiled without LLVM's AMDGPU atomic optimizer (Makefile), so
// every atomicAdd below is the instruction it names, per active lane: an
// atomic that should be one per wave is issued by one lane or aggregated in
// source.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <cstdint>
#include <type_traits>

#include "code_objects.hpp"
#include "scan.hpp"
#include "sks_hash.hpp"

namespace sks {

namespace {

constexpr int kBlock = 256;
constexpr int kWPT = 16;                  // windows per lane
constexpr int kTile = kBlock * kWPT;      // 4096 window starts per tile
constexpr int kHaloWords = 4;             // 64 extra bases (>= w - 1 for w <= 64)
constexpr int kWords = kBlock + kHaloWords;            // 2-bit words per tile (16 bases each)
constexpr int kLoadVecs = (kWords * 16 + 16) / 16;      // 16-B loads per tile (+1 for alignment)
constexpr int kQCap = 2048;               // LDS survivor queue entries (list mode, wide path)
#ifndef SKS_SCAN_QCAP
#define SKS_SCAN_QCAP 512
#endif
// FracMinHash keeps ~1/c of the windows and bottom-s ~s/L (a few per tile), so a
// small queue suffices there and leaves LDS for more workgroups per CU; list
// mode (every selected window, c = 1 keeps all) keeps the large one.
template <int MODE>
constexpr int qcap() { return MODE == kModeList ? kQCap : SKS_SCAN_QCAP; }
constexpr unsigned char kSep = '\n';      // any non-ACGT byte

struct Geom {
  uint64_t win0;    // byte index of the tile's first window start
  uint64_t seg_end; // end byte of the segment
  uint32_t seg;
};

// Scalar (wave-uniform) segment cursor: advance `seg` until tile is inside it.
__device__ __forceinline__ Geom tile_geom(const ScanParams& p, uint64_t tile, uint32_t& seg) {
  while (seg + 1 < p.n_seg && tile >= p.tile_prefix[seg + 1]) ++seg;
  Geom g;
  g.seg = seg;
  g.win0 = p.seg_begin[seg] + (tile - p.tile_prefix[seg]) * (uint64_t)kTile;
  g.seg_end = p.seg_end[seg];
  return g;
}

// A value every lane of the wave holds alike, moved to the scalar registers:
// what is computed from it (tile geometry, 64-bit compares, a load's base) then
// runs on the scalar unit, once per wave.
// (The builtin returns int: each half goes through uint32_t, or widening the
// low one would sign-extend bit 31 over the high one.)
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

// A wave-uniform 64-bit value given a scalar register pair of its own (no
// instruction beyond a possible copy).  The compiler then neither spills it as
// part of the block of kernel arguments it arrived in (a spilled SGPR costs a
// v_readlane, a VALU op, at every use) nor folds it into per-lane address
// arithmetic: a load from such a base plus a 32-bit lane offset takes the
// SGPR-base form of global_load.
__device__ __forceinline__ uint64_t own_sgprs(uint64_t v) {
  asm("" : "+s"(v));
  return v;
}

// a < b for wave-uniform 64-bit values, on the scalar unit, as the borrow of
// a - b.  The scalar unit has no ordered 64-bit compare: the compiler moves one
// side to VGPRs for a v_cmp (two VALU ops per wave and test), also when the
// source asks for the borrow.
__device__ __forceinline__ bool uniform_less(uint64_t a, uint64_t b) {
  uint32_t diff, borrow;
  asm("s_sub_u32 %0, %2, %4\n\ts_subb_u32 %0, %3, %5\n\ts_cselect_b32 %1, 1, 0"
      : "=&s"(diff), "=s"(borrow)
      : "s"((uint32_t)a), "s"((uint32_t)(a >> 32)), "s"((uint32_t)b), "s"((uint32_t)(b >> 32))
      : "scc");
  return borrow != 0;
}

// The narrow kernel's segment cursor with the segment's geometry beside it, all
// wave-uniform (SGPRs).  The arrays are read when the cursor moves (and once at
// the start), not per tile: the kernel also stores to global memory, so the
// compiler cannot hoist such loads itself and each one costs a vector load, a
// full wait and 64-bit per-lane arithmetic behind it.
template <int MODE>
struct SegCursor {
  uint32_t seg;
  uint64_t next_prefix;  // tile_prefix[seg + 1]: the first tile past the segment
  uint64_t win_off;      // seg_begin[seg] - kTile * tile_prefix[seg]: win0 = win_off + kTile * tile
  int64_t end;           // seg_end[seg]
  uint64_t thresh;       // seg_thresh[seg] (bottom-s only)

  // the segment's own figures; prefix = tile_prefix[seg]
  __device__ __forceinline__ void load(const ScanParams& p, uint64_t prefix) {
    win_off = uniform64(p.seg_begin[seg]) - prefix * (uint64_t)kTile;
    end = (int64_t)uniform64(p.seg_end[seg]);
    if constexpr (MODE == kModeBottom) thresh = uniform64(p.seg_thresh[seg]);
  }
  __device__ __forceinline__ void start(const ScanParams& p, uint32_t s) {
    seg = __builtin_amdgcn_readfirstlane(s);
    next_prefix = uniform64(p.tile_prefix[seg + 1]);
    load(p, uniform64(p.tile_prefix[seg]));
  }
  // advance until `tile` is inside the segment (tile_geom's walk: tiles only grow)
  __device__ __forceinline__ void seek(const ScanParams& p, uint64_t tile) {
    if (seg + 1 < p.n_seg && !uniform_less(tile, next_prefix)) {
      uint64_t prefix;
      do {  // segments without a tile are stepped over reading their prefix alone
        ++seg;
        prefix = next_prefix;
        next_prefix = uniform64(p.tile_prefix[seg + 1]);
      } while (seg + 1 < p.n_seg && !uniform_less(tile, next_prefix));
      load(p, prefix);
    }
  }
};

// What the window phase needs of a tile, fixed when the tile is prefetched
// (wave-uniform).
struct TileGeom {
  uint64_t win0;    // byte index of the tile's first window start
  uint64_t thresh;  // bottom-s: the segment's threshold
  uint32_t seg;
  uint32_t shift;   // align_shift of win0
};

// The sequence as a pointer that names the global address space: a pointer
// rebuilt from own_sgprs' integer would otherwise be a generic one (flat loads).
typedef const __attribute__((address_space(1))) uint8_t* GlobalBytes;
__device__ __forceinline__ GlobalBytes global_bytes(uint64_t address) {
  return reinterpret_cast<GlobalBytes>((uintptr_t)address);
}

__device__ __forceinline__ uint4 load16(const uint8_t* at) { return *reinterpret_cast<const uint4*>(at); }
__device__ __forceinline__ uint4 load16(GlobalBytes at) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = *reinterpret_cast<const __attribute__((address_space(1))) u32x4*>(at);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// Load the 16-B vector #k of a tile: bytes [base + 16k, base + 16k + 16) where
// `base` (relative to seq, possibly negative) is 16-B aligned in absolute
// address terms, so every vector load is aligned even when the caller's
// sequence pointer is not.  Bytes at or past seg_end read as a separator.
template <class Bytes>
__device__ __forceinline__ uint4 load_vec(Bytes seq, int64_t base, int k, int64_t seg_end) {
  int64_t a = base + 16 * (int64_t)k;
  if (a + 16 <= seg_end) return load16(seq + a);
  uint32_t wv[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      int64_t pos = a + 4 * q + b;
      uint32_t ch = pos < seg_end ? seq[pos] : kSep;
      v |= ch << (8 * b);
    }
    wv[q] = v;
  }
  return make_uint4(wv[0], wv[1], wv[2], wv[3]);
}

// Offset of win0 inside its absolutely aligned 16-B chunk.
template <class Bytes>
__device__ __forceinline__ uint32_t align_shift(Bytes seq, uint64_t win0) {
  return (uint32_t)(((uint64_t)(uintptr_t)seq + win0) & 15u);
}

// 4 ASCII bytes -> 8 bits of little-endian 2-bit codes + 4 invalid bits.
// code = ((c >> 1) ^ (c >> 2)) & 3 maps A/a C/c G/g T/t to 0 1 2 3
// (fasta_processing.cpp:35-69); a byte is valid iff it equals "acgt"[code]
// after lower-casing.
__device__ __forceinline__ void encode4(uint32_t x, uint32_t& le8, uint32_t& inv4) {
  uint32_t low = x | 0x20202020u;
  uint32_t code = ((low >> 1) ^ (low >> 2)) & 0x03030303u;
  uint32_t expect = __builtin_amdgcn_perm(0u, 0x74676361u, code);  // bytes 'a','c','g','t'
  uint32_t eq = expect ^ low;
  uint32_t t = (eq & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  t = ~(t | eq | 0x7F7F7F7Fu);             // 0x80 in every byte where eq == 0
  uint32_t bad = (~t) & 0x80808080u;       // 0x80 in every invalid byte
  inv4 = (bad * 0x00204081u) >> 28;        // gather bits 7,15,23,31 -> 0..3
  uint32_t y = code | (code >> 6);
  le8 = (y | (y >> 12)) & 0xFFu;
}

__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t s) {
  return __builtin_amdgcn_alignbit(hi, lo, s);
}

// 16 ASCII bytes (x[0..4] funnel-shifted by sb bits) -> 32 bits of
// little-endian 2-bit codes (base k at bits 2k) and a 16-bit invalid map.
// Fast path: per dword, the 4 codes are gathered into bits 24..31 by one
// multiply (c0 + c1<<2 + c2<<4 + c3<<6: the cross products land below bit 24
// without overlapping), and validity of all 4 bytes is one v_sad_u8 against
// the expected lower-case letters.  Only a 16-base word holding a non-ACGT
// byte pays for the exact per-byte invalid bits (encode4).
// ALIGNED: x[0..3] are the word's dwords as they are (the pack from the
// prefetch registers of a tile that starts on a 16-byte boundary, e.g. config
// 3), so the four alignbits go.
template <bool ALIGNED>
__device__ __forceinline__ void pack16(const uint32_t (&x)[5], uint32_t sb, uint32_t& le,
                                       uint32_t& inv) {
  uint32_t w[4], g[4], sad = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[k] = ALIGNED ? x[k] : funnel(x[k + 1], x[k], sb);
    const uint32_t low = w[k] | 0x20202020u;
    const uint32_t code = ((low >> 1) ^ (low >> 2)) & 0x03030303u;
    const uint32_t expect = __builtin_amdgcn_perm(0u, 0x74676361u, code);
    sad = __builtin_amdgcn_sad_u8(low, expect, sad);
    g[k] = code * 0x01041040u;  // gathered codes in bits 24..31
  }
  // bytes 3 of g[0..3] -> bytes 0..3 of le
  const uint32_t g01 = __builtin_amdgcn_perm(g[1], g[0], 0x0c0c0703u);
  const uint32_t g23 = __builtin_amdgcn_perm(g[3], g[2], 0x0c0c0703u);
  le = __builtin_amdgcn_perm(g23, g01, 0x05040100u);
  inv = 0;
  if (sad) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t le8, inv4;
      encode4(w[k], le8, inv4);
      inv |= inv4 << (4 * k);
    }
  }
}

__device__ __forceinline__ uint32_t rev_pairs(uint32_t x) {
  uint32_t r = __builtin_bitreverse32(x);
  return ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
}


// atomicAdd(counter, 1) from every active lane of the wave as ONE atomic: the
// lowest active lane adds their number, its return is broadcast and each lane
// adds its rank among the active ones (the slots a per-lane atomic would have
// handed out, in lane order).  `counter` must be wave-uniform.  Call it inside
// the divergent branch: the ballot of `true` is that branch's lane mask.  The
// compiler's atomic optimizer does this by itself; this unit is built without
// it, and 64 atomics per wave on one word would meet the ~88 per microsecond
// one counter word takes (MI355X_MICROARCH.md "dequeue").  (Here and not in
// wave_prims.hpp: the scan does not include the join's primitives.)
__device__ __forceinline__ unsigned long long wave_aggregated_inc(unsigned long long* counter) {
  const uint64_t act = __ballot(true);
  const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
  unsigned long long base = 0;
  if (rank == 0) base = atomicAdd(counter, (unsigned long long)__popcll(act));
  // readfirstlane reads the lowest active lane: the one that did the add
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
  return (((unsigned long long)hi << 32) | lo) + rank;
}

template <int MODE>
struct Queue {
  uint64_t key[qcap<MODE>()];
  uint64_t val[MODE == kModeBottom ? qcap<MODE>() : 1];
  uint32_t n;
  unsigned long long base;
  unsigned long long wins;  // windows of the current segment not yet published
};

template <int MODE>
__device__ __forceinline__ void emit(const ScanParams& p, Queue<MODE>& q, uint32_t seg,
                                     uint64_t key, uint64_t val) {
  uint32_t slot = atomicAdd(&q.n, 1u);
  if (slot < (uint32_t)qcap<MODE>()) {
    q.key[slot] = key;
    if constexpr (MODE == kModeBottom) q.val[slot] = val;
  } else {  // queue full: the direct path, one global atomic per wave
    unsigned long long g = wave_aggregated_inc(&p.seg_count[seg]);
    if (g < p.seg_out_cap[seg]) {
      uint64_t o = p.seg_out_off[seg] + g;
      p.out_key[o] = key;
      if constexpr (MODE == kModeBottom) p.out_val[o] = val;
    }
  }
}

// Block-wide flush of the LDS queue to segment `seg` (call from all threads).
template <int MODE>
__device__ __forceinline__ void flush(const ScanParams& p, Queue<MODE>& q, uint32_t seg) {
  __syncthreads();
  // the workgroup's window count: one global atomic per flush, not one per
  // wave — when a small input gives every workgroup one tile, all of them
  // finish together and the segment's counter word serialises the atomics
  // (one word takes ~88 per microsecond, MI355X_MICROARCH.md "dequeue")
  if (threadIdx.x == 0 && q.wins) atomicAdd(&p.seg_windows[seg], q.wins);
  constexpr uint32_t cap = qcap<MODE>();
  uint32_t n = q.n < cap ? q.n : cap;
  if (n) {
    if (threadIdx.x == 0) q.base = atomicAdd(&p.seg_count[seg], (unsigned long long)n);
    __syncthreads();
    uint64_t base = q.base;
    uint64_t cap = p.seg_out_cap[seg];
    uint64_t off = p.seg_out_off[seg];
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
      if (base + i < cap) {
        p.out_key[off + base + i] = q.key[i];
        if constexpr (MODE == kModeBottom) p.out_val[off + base + i] = q.val[i];
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    q.n = 0;
    q.wins = 0;
  }
  __syncthreads();
}

// Windows hashed by this thread for the current segment -> the workgroup's
// LDS total (published by the next flush of that segment).
__device__ __forceinline__ void add_windows(unsigned long long& wins, uint32_t cnt) {
  uint32_t v = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(&wins, (unsigned long long)v);
}

// frac_min_hash of a canonical k-mer (w <= 32, so the high block is 0).
template <int FLAVOUR>
__device__ __forceinline__ uint64_t fmh_narrow(const ScanParams& p, uint64_t c) {
  uint64_t h;
  if constexpr (FLAVOUR == 0) {
    h = hash_mix(c + kGolden32);                // combine(0, lo)
    h = hash_mix(h + kGolden32);                // combine(h, hi = 0)
    h = hash_mix(h + (128 + kGolden32));        // combine(num_bits = 128, h)
  } else {
    h = hash_bitset128<1>(c, 0);
  }
  return h ^ p.kconst;
}

// Flavour B up to the third hash_mix's second multiply: h = mix(mix(c+K)+K);
// x = h + 128 + K; x ^= x >> 32; x *= M; x ^= x >> 32. The rest of the hash
// is H = y ^ (y >> 28) with y = x * M, and fmh = H ^ kconst. The low 4 bits
// of H need only the low 32 bits of y, i.e. one v_mul_lo_u32 (low-bits
// pre-filter of the FracMinHash test, scan_kernel<..., PRE = 1>).
__device__ __forceinline__ uint64_t mix3_head(uint64_t c) {
  uint64_t h = hash_mix(c + kGolden32);
  h = hash_mix(h + kGolden32);
  uint64_t x = h + (128 + kGolden32);
  x ^= x >> 32;
  x = mul_const<kMixMul>(x);
  return x ^ (x >> 32);
}

template <int MODE>
__device__ __forceinline__ bool keep_fmh(const ScanParams& p, uint64_t f, uint64_t thresh) {
  if constexpr (MODE != kModeBottom) return div_test(f, p.low_mask, p.high_mask, p.dinv, p.dlim);
  else return f <= thresh;
}

constexpr int kBeOff = 2;  // s_be[kBeOff + i] = word i; two zero words in front

// Waves per SIMD the compiler must leave room for (its register budget is
// 512 / waves): 7 for the pre-filter kernel (what its ~100 SGPRs allow, and
// what the runtime's occupancy query answers), 4 for list mode with its large
// queue, 6 for bottom-s with the one-op minimum (79 VGPRs when left alone in
// round 10; asked for since round 11, whose scalar tile geometry otherwise
// tempts the compiler to 85), 5 for the rest.  Without it the compiler spends
// registers on hoisted addresses and a whole wave per SIMD goes.
template <int MODE, int PRE, int FMIN>
constexpr int min_waves() {
#ifdef SKS_SCAN_MIN_WAVES
  return SKS_SCAN_MIN_WAVES;
#else
  return PRE ? 7 : MODE == kModeList ? 4 : (MODE == kModeBottom && FMIN) ? 6 : 5;
#endif
}

constexpr uint32_t kCandCap = 128;  // pre-filter candidates per wave (< 64 + 64)

// Unsigned minimum of two values below 2^62 in one VALU op.  Read as IEEE
// doubles such bit patterns are non-negative and finite (bit 62 clear: the
// exponent field is never all ones, so no NaN and no infinity), and finite
// non-negative doubles order exactly as their bit patterns do; zero and the
// denormal patterns (values below 2^52) included, since the kernels keep f64
// denormals (the compiler's default float mode) and a minimum returns one of
// its operands unchanged.  The masked windows of w <= 31 use at most 62 bits.
// The builtin fmin would add a canonicalising v_max_f64 per operand, hence the asm.
constexpr int kFminMaxW = 31;
__device__ __forceinline__ uint64_t min_below_2_62(uint64_t a, uint64_t b) {
  uint64_t r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// FMIN: the canonical minimum is min_below_2_62 (launch_scan picks it for
// w <= kFminMaxW); otherwise the 64-bit compare and select, which w = 32 needs.
template <int MODE, int FLAVOUR, int PRE = 0, int FMIN = 0>
__global__ __launch_bounds__(kBlock, (min_waves<MODE, PRE, FMIN>())) void scan_kernel(ScanParams p) {
  __shared__ uint32_t s_raw[kLoadVecs * 4];
  __shared__ uint32_t s_be[kWords + 2 + kBeOff];
  __shared__ uint32_t s_lc[kWords + 2];
  __shared__ uint32_t s_inv[kWords + 2];
  __shared__ Queue<MODE> q;
  // (z, c) of windows past the low-bits pre-filter, per wave (PRE only)
  __shared__ ulonglong2 s_cand[PRE ? (kBlock / 64) * kCandCap : 1];
  // per wave: the cursor, the LDS byte address of its list's next free slot (PRE only)
  __shared__ uint32_t s_ctop[PRE ? kBlock / 64 : 1];

  __shared__ unsigned long long s_next;  // dynamic tiles: the next chunk's first tile

  const int tid = threadIdx.x;
  // Tiles: static — workgroup b streams the contiguous range b·T/grid ..; or
  // dynamic (p.tile_queue) — a persistent grid whose workgroups take chunks of
  // p.chunk consecutive tiles, the first one b·chunk, the rest from one global
  // counter, so no workgroup is left with a range when the others are done
  // (a static range's tail is up to one range: ~1/16 of the kernel).  A chunk's
  // grab is issued by thread 0 at its first tile and published through LDS at
  // its last, so the atomic's latency hides behind the chunk's tiles.
  const bool dyn = p.tile_queue != nullptr;
  uint64_t t_begin, t_end;
  if (dyn) {
    t_begin = (uint64_t)blockIdx.x * p.chunk;
    t_end = min(t_begin + p.chunk, p.n_tiles);
  } else {
    t_begin = (uint64_t)blockIdx.x * p.n_tiles / gridDim.x;
    t_end = (uint64_t)(blockIdx.x + 1) * p.n_tiles / gridDim.x;
  }
  if (tid == 0) {
    q.n = 0;
    q.wins = 0;
  }
  if (t_begin >= t_end) return;
  unsigned long long grab = 0;  // thread 0: the pending chunk grab

  const int w = p.w;
  // F of the window at base b is read as the 64 big-endian bits starting at
  // base b - (32 - w): its low 2w bits are F, the bits above are older bases
  // that the mask (bits < 2w) removes, so no per-window shift is needed.
  const uint32_t dshift = 2 * (32 - w);          // 0..62 bits
  const uint64_t wmask_bits = (w >= 64) ? ~0ull : ((1ull << w) - 1);
  if (tid < kBeOff) s_be[tid] = 0;
  // Lane (grp, r) owns the window starts 16 (16 grp + m) + r, m = 0..15: word
  // wbase + m of the tile, base r of it.  With P(m) the 32 BE bits from bit
  // 2r - dshift of word wbase + m and Q(m) the 32 LC bits from bit 2r of it,
  //   F(m) = P(m) : P(m + 1)      R(m) = Q(m + 1) : Q(m)
  // so a window adds one word and one funnel shift per strand to its
  // predecessor's.  2r - dshift + 64 = 32 qf + st with st in [1, 32]: P(m) starts
  // st bits into word wbase + m - 2 + qf, i.e. it is that word and the next
  // shifted right by 32 - st in [0, 31] (st = 32 is the next word itself, which
  // a shift of 0 gives; the kBeOff zero words cover wbase + m - 2 + qf < 0).
  const uint32_t r = tid & 15;
  const uint32_t wbase = (uint32_t)(tid >> 4) * kWPT;
  const uint32_t of = 2 * r + 64 - dshift;  // 2..94
  const uint32_t qf = (of - 1) >> 5;        // 0..2
  const uint32_t sF = 32 * qf + 32 - of;    // 0..31
  const uint32_t sR = 2 * r;
  const uint32_t* const fb = s_be + (kBeOff - 2) + wbase + qf;  // fb[m], fb[m + 1] -> P(m)
  const uint32_t* const rb = s_lc + wbase;                      // rb[m], rb[m + 1] -> Q(m)

  // segment cursors (wave-uniform) for the current tile and the prefetch
  uint32_t seg_lo = 0, seg_hi = p.n_seg;
  while (seg_lo + 1 < seg_hi) {  // last segment with tile_prefix[seg] <= t_begin
    uint32_t mid = (seg_lo + seg_hi) >> 1;
    if (p.tile_prefix[mid] <= t_begin) seg_lo = mid; else seg_hi = mid;
  }
  // The one segment cursor follows the prefetch: a tile's geometry is fixed
  // when its bytes are requested (pg) and handed to the tile's own iteration,
  // since the tile prefetched is always the next one processed.
  SegCursor<MODE> sc;
  sc.start(p, seg_lo);
  const GlobalBytes seq = global_bytes(own_sgprs((uint64_t)(uintptr_t)p.seq));
  TileGeom pg;
  uint4 v0, v1 = make_uint4(0, 0, 0, 0);
  // Tile t's geometry on the scalar unit, and its kLoadVecs 16-byte vectors
  // from the aligned base at or below its first window.  An interior tile — the
  // last vector ends inside the segment, a wave-uniform test — loads from that
  // scalar base plus the lane's constant offset; only a segment's last tile(s)
  // take load_vec's per-lane bounds and its byte-wise masked tail.  Both read
  // exactly the vectors that lie whole inside [.., seg_end).
  auto prefetch = [&](uint64_t t) {
    sc.seek(p, t);
    pg.seg = sc.seg;
    pg.thresh = (MODE == kModeBottom) ? sc.thresh : 0;
    pg.win0 = sc.win_off + t * (uint64_t)kTile;
    pg.shift = align_shift(seq, pg.win0);
    const int64_t base = (int64_t)pg.win0 - pg.shift;
    // (both sides are non-negative: base >= -15)
    const bool interior = !uniform_less((uint64_t)sc.end, (uint64_t)(base + 16 * kLoadVecs));
    const uint64_t bp = (uint64_t)(uintptr_t)seq + (uint64_t)base;
    // the lane's offset is made a 32-bit value of the very block that loads,
    // where the instruction selection sees base + zero-extended offset
    uint32_t lane_off = 16 * tid;
    asm volatile("" : "+v"(lane_off));
    if (interior) v0 = load16(global_bytes(own_sgprs(bp)) + lane_off);
    else v0 = load_vec(seq, base, tid, sc.end);
    if (lane_off < 16 * (kLoadVecs - kBlock)) {
      if (interior) {
        asm volatile("" : "+v"(lane_off));
        v1 = load16(global_bytes(own_sgprs(bp + 16 * kBlock)) + lane_off);
      } else {
        v1 = load_vec(seq, base, kBlock + tid, sc.end);
      }
    }
  };
  prefetch(t_begin);

  uint32_t win_count = 0;
  uint32_t count_seg = pg.seg;

  // pre-filter kernel: the LDS address of the lane's own slot in its wave's
  // candidate list, computed once (the empty asm keeps the compiler from
  // rebuilding it at each of the ~2.5 finishes per tile)
  uint32_t cb_lane = 0;
  if constexpr (PRE) {
    cb_lane = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(s_cand + (tid >> 6) * kCandCap + (tid & 63));
    asm volatile("" : "+v"(cb_lane));
  }

  for (uint64_t tile = t_begin; tile < t_end;) {
    const TileGeom g = pg;  // this tile's: the prefetch below moves pg on
    // The thread index as a value of this iteration: a lane predicate made from
    // it (tid == 0, tid < kHaloWords) is one v_cmp here, where the
    // compiler would hoist it out of the loop as a lane mask in an SGPR pair
    // that it then spills (two v_readlane per use, and SGPRs are what is short).
    int ltid = tid;
    asm volatile("" : "+v"(ltid));
    if (g.seg != count_seg) {  // segment change: publish the previous segment
      add_windows(q.wins, win_count);
      win_count = 0;
      flush<MODE>(p, q, count_seg);
      count_seg = g.seg;
    }
    const uint32_t shift = g.shift;
    const uint64_t thresh = g.thresh;
    const bool last_of_chunk = tile + 1 == t_end;
    if (dyn && ltid == 0) {
      if (tile == t_begin)
        grab = (unsigned long long)gridDim.x * p.chunk + atomicAdd(p.tile_queue, (unsigned long long)p.chunk);
      if (last_of_chunk) s_next = grab;
    }

    // 1) + 2) pack: word i covers bases [16 i, 16 i + 16) of the tile
    auto store_word = [&](int i, uint32_t le, uint32_t inv) {
      s_be[kBeOff + i] = rev_pairs(le);
      s_lc[i] = ~le;
      s_inv[i] = inv;
    };
    if (shift == 0) {
      // the tile starts on a 16-byte boundary (wave-uniform; every tile of a
      // genome that does, e.g. config 3): lane tid's prefetched vector is word
      // tid and lanes 0..3 hold the halo words, so they are packed from the
      // registers without the trip through s_raw and its barrier
      uint32_t le, inv;
      const uint32_t x0[5] = {v0.x, v0.y, v0.z, v0.w, 0u};
      pack16<true>(x0, 0, le, inv);
      store_word(tid, le, inv);
      if (ltid < kHaloWords) {
        const uint32_t x1[5] = {v1.x, v1.y, v1.z, v1.w, 0u};
        pack16<true>(x1, 0, le, inv);
        store_word(kBlock + tid, le, inv);
      }
    } else {
      reinterpret_cast<uint4*>(s_raw)[tid] = v0;
      if (tid < kLoadVecs - kBlock) reinterpret_cast<uint4*>(s_raw)[kBlock + tid] = v1;
      __syncthreads();
      const uint32_t sb = (shift & 3) * 8;  // wave-uniform
      for (int i = tid; i < kWords; i += kBlock) {
        const uint32_t wi = (16 * i + shift) >> 2;  // dword offset in s_raw
        uint32_t x[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) x[k] = s_raw[wi + k];
        uint32_t le, inv;
        pack16<false>(x, sb, le, inv);
        store_word(i, le, inv);
      }
    }
    __syncthreads();
    // the next tile: the chunk's next, else the next chunk's first (read here,
    // after the barrier; s_next is rewritten only at the next chunk's last
    // tile).  Every lane reads the same value: readfirstlane keeps the tile
    // counters and their 64-bit compares on the scalar unit.
    uint64_t next_tile = tile + 1;
    bool more = !last_of_chunk;  // a static range ends with its last tile
    if (last_of_chunk && dyn) {
      next_tile = uniform64(s_next);
      more = uniform_less(next_tile, p.n_tiles);
    }

    // 3) prefetch the next tile while this one is hashed
    if (more) prefetch(next_tile);

    // 4) 16 windows per lane: starts 16 (wbase + m) + r
    // A wave's windows read the invalid map of its 64 words and of the 2 after
    // them (bases up to 15 + 31 past its last word's first).
    const int lane = tid & 63;
    bool dirty = s_inv[tid] != 0;
    if (lane < 2) dirty = dirty || s_inv[(tid | 63) + 1 + lane] != 0;
    const bool wave_clean = !__any(dirty);
    auto canon_of = [&](uint32_t fh, uint32_t fl, uint32_t rh, uint32_t rl) -> uint64_t {
      const uint64_t F = (((uint64_t)fh) << 32) | fl;
      const uint64_t R = (((uint64_t)rh) << 32) | rl;
      const uint64_t fm = F & p.mask_lo, rm = R & p.mask_lo;
      if constexpr (FMIN) return min_below_2_62(fm, rm);
      else return fm < rm ? fm : rm;
    };
    // canonical masked k-mer of window m, re-read from LDS (run-time m: the
    // survivors of the keep-mask loop)
    auto canon_at = [&](uint32_t m) -> uint64_t {
      const uint32_t f0 = fb[m], f1 = fb[m + 1], f2 = fb[m + 2];
      const uint32_t r0 = rb[m], r1 = rb[m + 1], r2 = rb[m + 2];
      return canon_of(funnel(f0, f1, sF), funnel(f1, f2, sF), funnel(r2, r1, sR), funnel(r1, r0, sR));
    };
    // The walk of a wave that holds an invalid base (rare; a loop, to keep it out
    // of the unrolled code): body(m, c, valid).  Same carried words as the clean
    // walk, plus the invalid map: window m is valid iff bits [r, r + w) of the
    // map from word wbase + m are 0 (r + w <= 47: three 16-bit words).  Words up
    // to wbase + 18 are read (the last unused): all inside the packed tile.
    auto for_windows_checked = [&](auto body) {
      const uint32_t* const ib = s_inv + wbase;
      uint32_t fw = fb[1], rw = rb[1];
      uint32_t fp = funnel(fb[0], fw, sF), rp = funnel(rw, rb[0], sR);
      uint32_t i0 = ib[0], i1 = ib[1];
      // the reads run one window ahead where registers allow (not in the
      // pre-filter kernel, which sits at its occupancy's register limit)
      uint32_t fnext = 0, rnext = 0, inext = 0;
      if constexpr (!PRE) {
        fnext = fb[2];
        rnext = rb[2];
        inext = ib[2];
      }
#pragma unroll 1
      for (int m = 0; m < kWPT; ++m) {
        uint32_t fw2, rw2, i2;
        if constexpr (PRE) {
          fw2 = fb[m + 2];
          rw2 = rb[m + 2];
          i2 = ib[m + 2];
        } else {
          fw2 = fnext;
          rw2 = rnext;
          i2 = inext;
          fnext = fb[m + 3];
          rnext = rb[m + 3];
          inext = ib[m + 3];
        }
        const uint32_t fn = funnel(fw, fw2, sF), rn = funnel(rw2, rw, sR);
        const uint64_t iv = (uint64_t)i0 | ((uint64_t)i1 << 16) | ((uint64_t)i2 << 32);
        body(m, canon_of(fp, fn, rn, rp), ((iv >> r) & wmask_bits) == 0);
        fw = fw2; rw = rw2; fp = fn; rp = rn; i0 = i1; i1 = i2;
      }
    };
    // The clean wave's unrolled walk over its 16 windows: body(m, c) gets the
    // canonical k-mer; each step reads one new word per strand, one window
    // ahead of its use.  The compiler barrier keeps the reads there: hoisted to
    // the top, the 36 words would cost the registers that set the occupancy.
    auto for_windows = [&](auto body) {
      uint32_t fw = fb[1], rw = rb[1];
      uint32_t fp = funnel(fb[0], fw, sF), rp = funnel(rw, rb[0], sR);
      uint32_t fnext = fb[2], rnext = rb[2];
#pragma unroll
      for (int m = 0; m < kWPT; ++m) {
        const uint32_t fw2 = fnext, rw2 = rnext;
        if (m + 1 < kWPT) {
          fnext = fb[m + 3];
          rnext = rb[m + 3];
        }
        asm volatile("" ::: "memory");
        const uint32_t fn = funnel(fw, fw2, sF), rn = funnel(rw2, rw, sR);
        body(m, canon_of(fp, fn, rn, rp));
        fw = fw2; rw = rw2; fp = fn; rp = rn;
      }
    };
    // Hot loop: no branches — one keep bit per window, so the compiler can
    // interleave the 16 independent hash chains.  Survivors (~1/c) are
    // re-derived and emitted afterwards.
    if constexpr (PRE) {
      // FracMinHash with an even c: a window survives only if the low
      // min(s, 4) bits of its fmh are zero, and those follow from the low 32
      // bits of the last multiply. Windows passing that test (1/8 for c = 1000)
      // are queued per wave in LDS and finished 64 at a time, all lanes busy.
      // A passing lane takes its slot from the wave's cursor with a returning
      // LDS atomic (ds_add_rtn_u32: the LDS unit hands the passing lanes
      // distinct consecutive slots, in no particular order — the sketch is a
      // sorted set), so the append costs no ballot rank (2 v_mbcnt) and no slot
      // arithmetic.  This needs the unit built without the compiler's atomic
      // optimizer (Makefile), which would turn the atomic back into exactly that.
      // The cursor holds the slot's LDS byte address itself (the list's base plus
      // 16 per candidate), so the atomic's return is the ds_write's address.
      // the wave's candidate buffer, wave-uniform: readfirstlane keeps it in SGPRs
      const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
      ulonglong2* cb = s_cand + wv * kCandCap;
      uint32_t* const ctop = s_ctop + wv;
      typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
      typedef __attribute__((address_space(3))) u64x2 lds_u64x2;
      const uint32_t cb_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)cb;
      // The cursor is written (reset) by lane 0 and added to by the passing
      // lanes of the same wave.  A wave's LDS instructions are issued and
      // executed in program order, so all that is needed is that the compiler
      // keeps that order: the store and the atomic name the same word, and the
      // wavefront-scope fences around the wave barrier (no instructions) make
      // the hand-over between lanes an ordering the memory model knows.
      auto set_cursor = [&](uint32_t n) {  // the list holds n candidates
        if (lane == 0) *ctop = cb_lds + 16 * n;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      };
      // candidate lane + i of the list, from the lane's own slot address (held in a
      // register; 16 i goes into the LDS instruction's offset field)
      auto cand_at = [&](uint32_t i) { return (lds_u64x2*)(uintptr_t)(cb_lane + 16 * i); };
      const uint32_t pmask = p.low_mask & 0xFu;
      const uint32_t kbits = (uint32_t)p.kconst & pmask;
      // low bits of c = 2^s * d the pre-filter has not tested (none when s <= 4):
      // a finished candidate needs only d | fmh then
      const uint32_t rest_lo = p.low_mask & ~0xFu, rest_hi = p.high_mask;
      uint32_t cnt = 0;  // wave-uniform: candidates in the list (the cursor's count, kept scalar)
      set_cursor(0);
      auto finish = [&](uint32_t n) {  // candidates [0, n), n <= 64
        __builtin_amdgcn_wave_barrier();
        if ((uint32_t)lane < n) {
          const u64x2 e = *cand_at(0);
          // f = y ^ (y >> 28) ^ kconst, one three-input xor (v_bitop3_b32) per half
          const uint64_t y = mul_const<kMixMul>(e.x);
          const uint32_t ylo = (uint32_t)y, yhi = (uint32_t)(y >> 32);
          const uint32_t flo = __builtin_amdgcn_bitop3_b32(ylo, funnel(yhi, ylo, 28), (uint32_t)p.kconst, 0x96);
          const uint32_t fhi = __builtin_amdgcn_bitop3_b32(yhi, yhi >> 28, (uint32_t)(p.kconst >> 32), 0x96);
          const uint64_t f = ((uint64_t)fhi << 32) | flo;
          if (mul_uniform(f, p.dinv) <= p.dlim) {  // few lanes, often none: the rest is skipped then
            bool keep = true;
            if (rest_lo | rest_hi)  // wave-uniform
              keep = ((flo & rest_lo) | (fhi & rest_hi)) == 0;
            if (keep) emit<MODE>(p, q, g.seg, e.y, 0);
          }
        }
        __builtin_amdgcn_wave_barrier();
      };
      auto window_pre = [&](uint64_t c, bool valid) {
          const uint64_t z = mix3_head(c);
          const uint32_t ylo = (uint32_t)z * (uint32_t)kMixMul;
          const bool pass = (((ylo ^ (ylo >> 28)) & pmask) == kbits) && valid;
          // the ballot feeds the scalar count only (taken next to the compare: after
          // the branch the compiler would rebuild the mask with a select and a compare)
          const uint64_t bal = __ballot(pass);
          if (pass) {
            // cnt < 64 before the window and at most 64 lanes pass: slots < kCandCap
            const uint32_t slot = atomicAdd(ctop, 16u);
            u64x2 zc;
            zc.x = z;
            zc.y = c;
            *(lds_u64x2*)(uintptr_t)slot = zc;
          }
          cnt += (uint32_t)__popcll(bal);
          if (cnt >= 64) {
            finish(64);
            // < 64: move them to the front.  Slots [64, 64 + rest) and [0, rest) do
            // not overlap and a wave's LDS accesses run in program order, so each
            // lane moves its own candidate, after the finish's reads of the front
            const uint32_t rest = cnt - 64;
            if ((uint32_t)lane < rest) *cand_at(0) = *cand_at(64);
            cnt = rest;
            set_cursor(rest);
          }
      };
      if (wave_clean) {
        for_windows([&](int, uint64_t c) { window_pre(c, true); });
        win_count += kWPT;
      } else {
        for_windows_checked([&](int, uint64_t c, bool valid) {
          win_count += valid ? 1u : 0u;
          window_pre(c, valid);
        });
      }
      if (cnt) finish(cnt);
    } else {
    uint32_t keepmask = 0;
    // bottom-s, flavour B: the candidate test only needs fmh's top 28 bits, which
    // are the top bits of the last product y (H = y ^ (y >> 28) changes only
    // bits < 36), so the xor-shift, the constant and the 64-bit compare go; a
    // window whose top 28 bits equal the threshold's passes even if fmh > T (a
    // superset of candidates: the post-processing selects exactly)
    const uint32_t thr_top = (uint32_t)(thresh >> 36);
    const uint32_t k_top = (uint32_t)(p.kconst >> 32);
    auto keep_window = [&](uint64_t c) -> bool {
      if constexpr (MODE == kModeBottom && FLAVOUR == 0) {
        const uint64_t y = mul_const<kMixMul>(mix3_head(c));
        return (((uint32_t)(y >> 32) ^ k_top) >> 4) <= thr_top;
      } else {
        return keep_fmh<MODE>(p, fmh_narrow<FLAVOUR>(p, c), thresh);
      }
    };
    if (wave_clean) {
      for_windows([&](int m, uint64_t c) { keepmask |= (keep_window(c) ? 1u : 0u) << m; });
      win_count += kWPT;
    } else {
      for_windows_checked([&](int m, uint64_t c, bool valid) {
        win_count += valid ? 1u : 0u;
        keepmask |= (keep_window(c) && valid ? 1u : 0u) << m;
      });
    }
    while (keepmask) {
      const uint32_t j = __builtin_ctz(keepmask);
      keepmask &= keepmask - 1;
      if constexpr (MODE == kModeList) {
        emit<MODE>(p, q, g.seg, g.win0 + (uint64_t)(16 * (wbase + j) + r), 0);  // window start byte
      } else {
        const uint64_t c = canon_at(j);
        // bottom-s: the candidate's fmh is recomputed after compaction
        // (launch_fmh_narrow) instead of here, where the whole wave would wait
        // on the ~45-VALU hash for the ~5% of lanes holding a candidate
        if constexpr (MODE == kModeFrac) emit<MODE>(p, q, g.seg, c, 0);
        else emit<MODE>(p, q, g.seg, c, c);
      }
    }
    }  // !PRE

    // 5) flush the queue once it is half full
    __syncthreads();
    if (q.n >= (uint32_t)qcap<MODE>() / 2) {
      add_windows(q.wins, win_count);
      win_count = 0;
      flush<MODE>(p, q, g.seg);
    }
    if (!last_of_chunk) {
      ++tile;
    } else if (dyn) {  // next chunk (every thread holds the same next_tile): exits past n_tiles
      t_begin = tile = next_tile;
      t_end = min(next_tile + p.chunk, p.n_tiles);
    } else {
      break;
    }
  }
  add_windows(q.wins, win_count);
  flush<MODE>(p, q, count_seg);
}

// ---- wide path: 32 < w <= 64 (128-bit windows) -------------------------------------
// Same structure; F and R are 128-bit.  Survivors carry (lo, hi) in (key, val)
// for FracMinHash and (fmh, lo) + hi in a side array for bottom-s.
template <int MODE, int FLAVOUR>
__global__ __launch_bounds__(kBlock) void scan_kernel_wide(ScanParams p) {
  __shared__ uint32_t s_raw[kLoadVecs * 4];
  __shared__ uint32_t s_be[kWords + 2];
  __shared__ uint32_t s_lc[kWords + 2];
  __shared__ uint32_t s_inv[kWords + 2];
  __shared__ uint64_t q_a[kQCap / 2], q_b[kQCap / 2], q_c[kQCap / 2];
  __shared__ uint32_t q_n;
  __shared__ unsigned long long q_base, q_wins;

  const int tid = threadIdx.x;
  const uint64_t t_begin = (uint64_t)blockIdx.x * p.n_tiles / gridDim.x;
  const uint64_t t_end = (uint64_t)(blockIdx.x + 1) * p.n_tiles / gridDim.x;
  if (tid == 0) {
    q_n = 0;
    q_wins = 0;
  }
  if (t_begin >= t_end) return;
  constexpr uint32_t cap = kQCap / 2;

  const int w = p.w;
  const uint32_t fshift = 128 - 2 * w;  // 0..62
  const uint64_t wmask_bits = (w >= 64) ? ~0ull : ((1ull << w) - 1);

  uint32_t seg_lo = 0, seg_hi = p.n_seg;
  while (seg_lo + 1 < seg_hi) {
    uint32_t mid = (seg_lo + seg_hi) >> 1;
    if (p.tile_prefix[mid] <= t_begin) seg_lo = mid; else seg_hi = mid;
  }
  uint32_t cur_seg = seg_lo, pf_seg = seg_lo;
  Geom pg = tile_geom(p, t_begin, pf_seg);
  int64_t pf_base = (int64_t)pg.win0 - align_shift(p.seq, pg.win0);
  uint4 v0 = load_vec(p.seq, pf_base, tid, (int64_t)pg.seg_end);
  uint4 v1 = make_uint4(0, 0, 0, 0);
  if (tid < kLoadVecs - kBlock) v1 = load_vec(p.seq, pf_base, kBlock + tid, (int64_t)pg.seg_end);
  uint32_t win_count = 0;
  uint32_t count_seg = cur_seg;

  auto wflush = [&](uint32_t seg) {
    __syncthreads();
    if (tid == 0 && q_wins) atomicAdd(&p.seg_windows[seg], q_wins);
    uint32_t n = q_n < cap ? q_n : cap;
    if (n) {
      if (tid == 0) q_base = atomicAdd(&p.seg_count[seg], (unsigned long long)n);
      __syncthreads();
      uint64_t base = q_base, c = p.seg_out_cap[seg], off = p.seg_out_off[seg];
      for (uint32_t i = tid; i < n; i += kBlock)
        if (base + i < c) {
          p.out_key[off + base + i] = q_a[i];
          if (MODE != kModeList) p.out_val[off + base + i] = q_b[i];
          if (MODE == kModeBottom) p.out_hi[off + base + i] = q_c[i];
        }
    }
    __syncthreads();
    if (tid == 0) {
      q_n = 0;
      q_wins = 0;
    }
    __syncthreads();
  };

  for (uint64_t tile = t_begin; tile < t_end; ++tile) {
    Geom g = tile_geom(p, tile, cur_seg);
    if (g.seg != count_seg) {
      add_windows(q_wins, win_count);
      win_count = 0;
      wflush(count_seg);
      count_seg = g.seg;
    }
    const uint32_t shift = align_shift(p.seq, g.win0);
    const uint64_t thresh = (MODE == kModeBottom) ? p.seg_thresh[g.seg] : 0;
    reinterpret_cast<uint4*>(s_raw)[tid] = v0;
    if (tid < kLoadVecs - kBlock) reinterpret_cast<uint4*>(s_raw)[kBlock + tid] = v1;
    __syncthreads();
    for (int i = tid; i < kWords; i += kBlock) {
      const uint32_t b0 = 16 * i + shift;
      const uint32_t wi = b0 >> 2, sb = (b0 & 3) * 8;
      uint32_t x[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) x[k] = s_raw[wi + k];
      uint32_t le, inv;
      pack16<false>(x, sb, le, inv);
      s_be[i] = rev_pairs(le);
      s_lc[i] = ~le;
      s_inv[i] = inv;
    }
    __syncthreads();
    if (tile + 1 < t_end) {
      Geom ng = tile_geom(p, tile + 1, pf_seg);
      pf_base = (int64_t)ng.win0 - align_shift(p.seq, ng.win0);
      v0 = load_vec(p.seq, pf_base, tid, (int64_t)ng.seg_end);
      if (tid < kLoadVecs - kBlock) v1 = load_vec(p.seq, pf_base, kBlock + tid, (int64_t)ng.seg_end);
    }
    uint32_t be[5], lc[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) { be[k] = s_be[tid + k]; lc[k] = s_lc[tid + k]; }
    // 80 invalid bits: bases [16 tid, 16 tid + 80)
    const uint64_t inv_lo = (uint64_t)s_inv[tid] | ((uint64_t)s_inv[tid + 1] << 16) |
                            ((uint64_t)s_inv[tid + 2] << 32) | ((uint64_t)s_inv[tid + 3] << 48);
    const uint64_t inv_hi = (uint64_t)s_inv[tid + 4];
#pragma unroll
    for (int j = 0; j < kWPT; ++j) {
      // 128 BE bits of bases [16 tid + j, 16 tid + j + 64)
      uint32_t f3 = j ? funnel(be[0], be[1], 32 - 2 * j) : be[0];
      uint32_t f2 = j ? funnel(be[1], be[2], 32 - 2 * j) : be[1];
      uint32_t f1 = j ? funnel(be[2], be[3], 32 - 2 * j) : be[2];
      uint32_t f0 = j ? funnel(be[3], be[4], 32 - 2 * j) : be[3];
      uint64_t Fh = ((uint64_t)f3 << 32) | f2, Fl = ((uint64_t)f1 << 32) | f0;
      // >> fshift (0..62)
      if (fshift) { Fl = (Fl >> fshift) | (Fh << (64 - fshift)); Fh >>= fshift; }
      uint32_t r0 = j ? funnel(lc[1], lc[0], 2 * j) : lc[0];
      uint32_t r1 = j ? funnel(lc[2], lc[1], 2 * j) : lc[1];
      uint32_t r2 = j ? funnel(lc[3], lc[2], 2 * j) : lc[2];
      uint32_t r3 = j ? funnel(lc[4], lc[3], 2 * j) : lc[3];
      uint64_t Rl = ((uint64_t)r1 << 32) | r0, Rh = ((uint64_t)r3 << 32) | r2;
      uint64_t fml = Fl & p.mask_lo, fmh = Fh & p.mask_hi;
      uint64_t rml = Rl & p.mask_lo, rmh = Rh & p.mask_hi;
      bool f_lt = (fmh < rmh) || (fmh == rmh && fml < rml);
      uint64_t cl = f_lt ? fml : rml, ch = f_lt ? fmh : rmh;
      // window bits [j, j + w) of the 80-bit invalid map
      uint64_t iv = (inv_lo >> j) | (j ? (inv_hi << (64 - j)) : 0);
      bool valid = (iv & wmask_bits) == 0;
      win_count += valid ? 1u : 0u;
      uint64_t h;
      if constexpr (FLAVOUR == 0) {
        h = hash_mix(cl + kGolden32);
        h = hash_mix(h + kGolden32 + ch);
        h = hash_mix(h + (128 + kGolden32));
      } else {
        h = hash_bitset128<1>(cl, ch);
      }
      uint64_t f = h ^ p.kconst;
      bool keep = (MODE != kModeBottom) ? div_test(f, p.low_mask, p.high_mask, p.dinv, p.dlim)
                                        : (f <= thresh);
      if (valid && keep) {
        uint32_t slot = atomicAdd(&q_n, 1u);
        uint64_t a = (MODE == kModeList) ? g.win0 + (uint64_t)(kWPT * tid) + j
                                         : (MODE == kModeFrac) ? cl : f;
        uint64_t b = (MODE == kModeFrac) ? ch : cl;
        if (slot < cap) {
          q_a[slot] = a; q_b[slot] = b; q_c[slot] = ch;
        } else {
          unsigned long long gi = wave_aggregated_inc(&p.seg_count[g.seg]);
          if (gi < p.seg_out_cap[g.seg]) {
            uint64_t o = p.seg_out_off[g.seg] + gi;
            p.out_key[o] = a;
            if (MODE != kModeList) p.out_val[o] = b;
            if (MODE == kModeBottom) p.out_hi[o] = ch;
          }
        }
      }
    }
    __syncthreads();
    if (q_n >= cap / 2) {
      add_windows(q_wins, win_count);
      win_count = 0;
      wflush(g.seg);
    }
  }
  add_windows(q_wins, win_count);
  wflush(count_seg);
}

// The narrow FracMinHash and bottom-s kernels in the instantiation their window
// length allows: the one-op canonical minimum for w <= kFminMaxW.
template <int MODE, int FLAVOUR, int PRE, class Run>
hipError_t run_narrow(const ScanParams& p, Run run) {
  return p.w <= kFminMaxW ? run(scan_kernel<MODE, FLAVOUR, PRE, 1>) : run(scan_kernel<MODE, FLAVOUR, PRE, 0>);
}

constexpr int kGridOversubscribe = 16;
constexpr int kDynOversubscribe = 2;

template <class K>
int occupancy_grid(K kernel, int device) {
  int per_cu = 0;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0);
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  if (per_cu < 1) per_cu = 1;
  if (cus < 1) cus = 1;
  return per_cu * cus;
}

}  // namespace

uint64_t scan_tiles_for(uint64_t seg_bytes) { return (seg_bytes + kTile - 1) / kTile; }

hipError_t launch_scan(const ScanParams& p, int mode, int flavour, bool wide, int device,
                       hipStream_t stream, int grid_override) {
  if (p.n_tiles == 0) return hipSuccess;
  auto pick = [&](auto kernel) -> hipError_t {
    // Oversubscribe the resident slots 16x (config 3, pre-filter kernel: 20480
    // workgroups of ~36 tiles): the workgroup dispatcher then refills CUs as
    // ranges finish, which evens out per-CU speed differences and keeps every
    // SIMD at its wave limit. Measured on config 3 (tools/scan_grid_sweep.py):
    // 5.95 ms at 1x, 5.19 ms at 8x-16x before the pre-filter; with it 4.7 ms at
    // 8x and 16x (equal within noise in full benches), 5.6 ms at 32x and 9.2 at
    // 64x (per-workgroup start-up and flush costs).
    ScanParams q = p;
    q.tile_queue = nullptr;  // static tile ranges
    int grid = grid_override > 0 ? grid_override : kGridOversubscribe * occupancy_grid(kernel, device);
    if ((uint64_t)grid > p.n_tiles) grid = (int)p.n_tiles;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, q);
    return hipGetLastError();
  };
  // dynamic tiles (narrow kernels, p.tile_queue set): twice the resident
  // workgroups (every slot filled even if the occupancy query is conservative),
  // chunks of ~T / (16 grid) tiles, 2..16: the tail is at most one chunk, and
  // the counter takes <= ~1 grab per 16 tiles (config 3: ~21 per microsecond,
  // below the ~88 one word serves, MI355X_MICROARCH.md)
  auto pick_dyn = [&](auto kernel) -> hipError_t {
    ScanParams q = p;
    int grid = grid_override > 0 ? grid_override : kDynOversubscribe * occupancy_grid(kernel, device);
    const uint64_t per = p.n_tiles / ((uint64_t)grid * 16);
    // smallest chunk 3 (SKS_SCAN_MIN_CHUNK overrides): config 2's one 5 Mb genome
    // (1221 tiles) scans in 27.4 us in chunks of 3 against 32.2 in chunks of 2
    // (1: 43, 4: 30, 6: 29); 128 config-4 genomes are the same at 2 and 3
    static const uint64_t min_chunk = getenv("SKS_SCAN_MIN_CHUNK") ? std::max(1, atoi(getenv("SKS_SCAN_MIN_CHUNK"))) : 3;
    q.chunk = (uint32_t)std::min<uint64_t>(16, std::max<uint64_t>(min_chunk, per));
    const uint64_t need = (p.n_tiles + q.chunk - 1) / q.chunk;
    if ((uint64_t)grid > need) grid = (int)need;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, q);
    return hipGetLastError();
  };
  if (!wide && p.tile_queue) {
    if (mode == kModeFrac) {
      static const bool no_pre = getenv("SKS_NO_PREFILTER") != nullptr;
      if (flavour == 0 && (p.low_mask & 0xFu) && !no_pre) return run_narrow<kModeFrac, 0, 1>(p, pick_dyn);
      return flavour == 0 ? run_narrow<kModeFrac, 0, 0>(p, pick_dyn) : run_narrow<kModeFrac, 1, 0>(p, pick_dyn);
    }
    if (mode == kModeBottom)
      return flavour == 0 ? run_narrow<kModeBottom, 0, 0>(p, pick_dyn) : run_narrow<kModeBottom, 1, 0>(p, pick_dyn);
  }
  if (!wide) {
    if (mode == kModeFrac) {
      static const bool no_pre = getenv("SKS_NO_PREFILTER") != nullptr;
      if (flavour == 0 && (p.low_mask & 0xFu) && !no_pre) return run_narrow<kModeFrac, 0, 1>(p, pick);
      return flavour == 0 ? run_narrow<kModeFrac, 0, 0>(p, pick) : run_narrow<kModeFrac, 1, 0>(p, pick);
    }
    if (mode == kModeList) return flavour == 0 ? pick(scan_kernel<kModeList, 0>) : pick(scan_kernel<kModeList, 1>);
    return flavour == 0 ? run_narrow<kModeBottom, 0, 0>(p, pick) : run_narrow<kModeBottom, 1, 0>(p, pick);
  }
  if (mode == kModeFrac) return flavour == 0 ? pick(scan_kernel_wide<kModeFrac, 0>) : pick(scan_kernel_wide<kModeFrac, 1>);
  if (mode == kModeList) return flavour == 0 ? pick(scan_kernel_wide<kModeList, 0>) : pick(scan_kernel_wide<kModeList, 1>);
  return flavour == 0 ? pick(scan_kernel_wide<kModeBottom, 0>) : pick(scan_kernel_wide<kModeBottom, 1>);
}

SKS_CODE_OBJECT_HOOK(scan)

}  // namespace sks
