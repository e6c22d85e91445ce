// C-ABI implementation (include/sks.h): the last error, contexts and their
// setters, the host-side helpers of the reference API and the entry points that
// only pass their arguments to one launch.
#include <cmath>
#include <numeric>
#include <random>
#include <thread>

#include "sks_ani.hpp"
#include "sks_ctx.hpp"
#include "sks_hash.hpp"

namespace sks {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int check_layout_args(const char* who, const sks_ctx* c, uint32_t log_b, int elem_words) {
  if (!c) return fail(SKS_E_ARG, std::string(who) + ": null ctx");
  if (log_b > 14) return fail(SKS_E_ARG, std::string(who) + ": log_b > 14");
  if (elem_words != 1 && elem_words != 2) return fail(SKS_E_ARG, "elem_words must be 1 or 2");
  return SKS_OK;
}

int device_view_of_ani(double* ani, double** d_ani, const char* who) {
  hipPointerAttribute_t at{};
  const hipError_t e = hipPointerGetAttributes(&at, ani);
  (void)hipGetLastError();  // an unknown pointer leaves an error behind
  if (e != hipSuccess || at.type == hipMemoryTypeUnregistered)
    return sks::fail(SKS_E_ARG, std::string(who) + ": the ANI matrix is neither device memory nor pinned "
                                "host memory mapped into the device (use sks_host_alloc)");
  if (at.type == hipMemoryTypeHost) {
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, ani, 0) != hipSuccess || !dp) {
      (void)hipGetLastError();
      return sks::fail(SKS_E_ARG, std::string(who) + ": the pinned host ANI matrix is not mapped into the "
                                  "device (use sks_host_alloc)");
    }
    *d_ani = static_cast<double*>(dp);
  } else {
    *d_ani = ani;
  }
  return SKS_OK;
}

void attach_ani_root(const sks_ctx* c, int kmer_num_ones, JoinAni& A) {
  if (c->root_k != kmer_num_ones) return;
  A.root = static_cast<const double*>(c->root.ptr);
  A.root_size = c->root_size;
}

}  // namespace sks

using sks::DeviceGuard;

extern "C" {

int sks_abi_version(void) { return SKS_ABI_VERSION; }

const char* sks_last_error(void) { return sks::g_last_error.c_str(); }

// ---- host helpers -----------------------------------------------------------------------

// kmer_bitset.cpp:132-152 — std::shuffle(iota(w), std::mt19937(seed)); the
// first k shuffled indices j set mask bits 2j and 2j+1.  libstdc++ is used on
// purpose: the reference's masks are defined by its shuffle algorithm.
int sks_mask_generate(int window, int k, uint64_t seed, uint64_t mask[2]) {
  if (!mask) return sks::fail(SKS_E_ARG, "sks_mask_generate: null mask");
  if (window < 1 || window > 64 || k < 0 || k > window)
    return sks::fail(SKS_E_ARG, "sks_mask_generate: need 0 <= k <= window <= 64");
  std::vector<int> idx(window);
  std::iota(idx.begin(), idx.end(), 0);
  std::shuffle(idx.begin(), idx.end(), std::mt19937((std::mt19937::result_type)seed));
  mask[0] = mask[1] = 0;
  for (int i = 0; i < k; ++i) {
    int b = 2 * idx[i];
    mask[b >> 6] |= 3ull << (b & 63);
  }
  return SKS_OK;
}

// kmer_bitset.cpp:50-56 — 2l low bits set; l > 64 throws in the reference.
int sks_mask_contiguous(int length, uint64_t mask[2]) {
  if (!mask) return sks::fail(SKS_E_ARG, "sks_mask_contiguous: null mask");
  if (length > 64) return sks::fail(SKS_E_ARG, "Given k-mer length exceeds maximum k-mer length");
  if (length < 0) return sks::fail(SKS_E_ARG, "sks_mask_contiguous: negative length");
  int bits = 2 * length;
  mask[0] = bits >= 64 ? ~0ull : ((1ull << bits) - 1);
  mask[1] = bits <= 64 ? 0 : (bits >= 128 ? ~0ull : ((1ull << (bits - 64)) - 1));
  return SKS_OK;
}

uint64_t sks_frac_min_hash(const uint64_t kmer[2], const uint64_t mask[2], int window, int64_t nonce, int flavour) {
  return sks::hash_bitset128_rt(kmer[0], kmer[1], flavour) ^
         sks::fmh_const(mask[0], mask[1], window, nonce, flavour);
}

double sks_containment(int intersection, int set_size) {
  if (intersection == 0) return 0;
  return ((double)intersection) / ((double)set_size);
}

double sks_binomial_estimator(double containment, int kmer_num_ones) {
  if (containment <= 0) return 0;
  return std::pow(containment, ((double)1.0) / ((double)kmer_num_ones));
}

int sks_ani_from_counts(const int32_t* inter, const int32_t* size_first, uint64_t n,
                        int kmer_num_ones, double* cont, double* ani) {
  if (n && (!inter || !size_first)) return sks::fail(SKS_E_ARG, "sks_ani_from_counts: null input");
  // element-wise and order-free: large batches (an all-vs-all matrix) are split
  // over host threads; every element is the same scalar double arithmetic
  auto run = [=](uint64_t b, uint64_t e) {
    for (uint64_t i = b; i < e; ++i) {
      double c = sks_containment(inter[i], size_first[i]);
      if (cont) cont[i] = c;
      if (ani) ani[i] = sks_binomial_estimator(c, kmer_num_ones);
    }
  };
  const uint64_t kPer = 8192;
  unsigned T = std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
  T = (unsigned)std::min<uint64_t>(T, (n + kPer - 1) / kPer);
  if (T <= 1) {
    run(0, n);
    return SKS_OK;
  }
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < T; ++t) pool.emplace_back(run, n * t / T, n * (t + 1) / T);
  run(0, n / T);
  for (auto& th : pool) th.join();
  return SKS_OK;
}

// Group bounds fixed by the mask alone (no sample of the sketches): a masked
// canonical k-mer of random sequence is min(F & M, R & M) of two near-uniform
// values over the mask's 2k bits, so its packed value (the mask bits gathered)
// has CDF 1 - (1 - x)^2 and the g/G quantile is x = 1 - sqrt(1 - g/G); the
// bound is that packed value scattered back onto the mask bits (a pdep).  Any
// non-decreasing bounds give exact counts (layout.hip): these only balance the
// groups, and need no device pass and no exchange between ranks.
int sks_join_layout_bounds_for_mask(const uint64_t mask[2], uint32_t log_b, int elem_words, uint64_t* bounds) {
  if (!mask || !bounds) return sks::fail(SKS_E_ARG, "sks_join_layout_bounds_for_mask: null argument");
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (elem_words == 1 && mask[1]) return sks::fail(SKS_E_ARG, "sks_join_layout_bounds_for_mask: a 128-bit mask "
                                                               "needs elem_words = 2");
  const uint32_t G = sks_join_layout_groups(log_b);
  const int P = __builtin_popcountll(mask[0]) + __builtin_popcountll(mask[1]);
  auto pdep = [&](uint64_t vlo, uint64_t vhi, uint64_t* lo, uint64_t* hi) {
    *lo = *hi = 0;
    int j = 0;  // packed bit j -> the j-th set bit of the mask
    for (int b = 0; b < 128; ++b) {
      if (!((b < 64 ? mask[0] >> b : mask[1] >> (b - 64)) & 1)) continue;
      const uint64_t bit = j < 64 ? (vlo >> j) & 1 : (vhi >> (j - 64)) & 1;
      if (bit) {
        if (b < 64) *lo |= 1ull << b;
        else *hi |= 1ull << (b - 64);
      }
      ++j;
    }
  };
  for (uint32_t g = 0; g <= G; ++g) {
    uint64_t lo = 0, hi = 0;
    if (g == G) {
      lo = ~0ull;
      hi = elem_words == 2 ? ~0ull : 0;
    } else if (g > 0 && P > 0) {
      const long double x = 1.0L - std::sqrt(1.0L - (long double)g / (long double)G);
      uint64_t vlo = 0, vhi = 0;
      if (P <= 64) {
        const long double v = std::ldexp(x, P);
        vlo = v >= 18446744073709551615.0L ? (P == 64 ? ~0ull : (1ull << P) - 1) : (uint64_t)v;
      } else {
        const long double v = std::ldexp(x, P - 64);
        vhi = (uint64_t)std::floor(v);
        vlo = (uint64_t)std::ldexp(v - std::floor(v), 64);
      }
      pdep(vlo, vhi, &lo, &hi);
    }
    bounds[(size_t)g * elem_words] = lo;
    if (elem_words == 2) bounds[(size_t)g * 2 + 1] = hi;
  }
  return SKS_OK;
}

int sks_host_alloc(uint64_t bytes, int coherent, void** out) {
  if (!out) return sks::fail(SKS_E_ARG, "sks_host_alloc: null out");
  *out = nullptr;
  if (!bytes) return SKS_OK;
  void* p = nullptr;
  const unsigned flags = (coherent ? hipHostMallocCoherent : hipHostMallocNonCoherent) | hipHostMallocPortable |
                         hipHostMallocMapped;
  if (hipHostMalloc(&p, bytes, flags) != hipSuccess) {
    (void)hipGetLastError();
    return sks::fail(SKS_E_NOMEM, "sks_host_alloc: hipHostMalloc of " + std::to_string(bytes) + " bytes failed");
  }
  *out = p;
  return SKS_OK;
}

int sks_host_free(void* p) {
  if (p) SKS_HIP(hipHostFree(p));
  return SKS_OK;
}

// ---- contexts -----------------------------------------------------------------------------

int sks_ctx_create(int device, void* stream, sks_ctx** out) {
  if (!out) return sks::fail(SKS_E_ARG, "sks_ctx_create: null out");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return sks::fail(SKS_E_HIP, std::string("sks_ctx_create: no HIP device available (the engine has "
                                            "no CPU path): hipGetDeviceCount -> ") +
                                    hipGetErrorString(e) + ", " + std::to_string(n) + " devices");
  if (device < 0 || device >= n) return sks::fail(SKS_E_ARG, "sks_ctx_create: bad device index");
  DeviceGuard g(device);
  sks_ctx* c = new (std::nothrow) sks_ctx();
  if (!c) return sks::fail(SKS_E_NOMEM, "sks_ctx_create: out of memory");
  c->device = device;
  c->stream = reinterpret_cast<hipStream_t>(stream);
  // every scratch buffer is used on the context's stream only
  c->each_scratch([c](sks::Scratch& sc) { sc.owner = &c->stream; });
  if (hipEventCreate(&c->ev_begin) != hipSuccess || hipEventCreate(&c->ev_end) != hipSuccess ||
      hipEventCreate(&c->ev_s0) != hipSuccess || hipEventCreate(&c->ev_s1) != hipSuccess ||
      hipEventCreate(&c->ev_i0) != hipSuccess || hipEventCreate(&c->ev_i1) != hipSuccess) {
    delete c;  // destroys the events created so far
    return sks::fail(SKS_E_HIP, "sks_ctx_create: hipEventCreate failed");
  }
  // every code object of the library on this device, before the first build
#define SKS_CALL_HOOK(tu) \
  if (e == hipSuccess) e = sks::code_object_hook_##tu(c->stream);
  e = hipSuccess;
  SKS_TU_LIST(SKS_CALL_HOOK)
#undef SKS_CALL_HOOK
  if (e != hipSuccess) {
    delete c;
    return sks::fail(SKS_E_HIP, std::string("sks_ctx_create: code object load: ") + hipGetErrorString(e));
  }
  *out = c;
  return SKS_OK;
}

int sks_ctx_destroy(sks_ctx* c) {
  if (!c) return SKS_OK;
  DeviceGuard g(c->device);
  (void)hipStreamSynchronize(c->stream);
  c->each_scratch([](sks::Scratch& sc) { sc.release(); });
  sks::trim_device_cache(c->device);
  delete c;
  return SKS_OK;
}

int sks_ctx_device(const sks_ctx* c) { return c ? c->device : -1; }

int sks_ctx_set_stream(sks_ctx* c, void* stream) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ctx_set_stream: null ctx");
  // scratch blocks are released in the order of the context's stream: let the
  // old stream's work finish before the order changes
  if (c->stream != reinterpret_cast<hipStream_t>(stream)) {
    DeviceGuard g(c->device);
    SKS_HIP(hipStreamSynchronize(c->stream));
  }
  c->stream = reinterpret_cast<hipStream_t>(stream);
  return SKS_OK;
}

int sks_ctx_synchronize(sks_ctx* c) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ctx_synchronize: null ctx");
  DeviceGuard g(c->device);
  SKS_HIP(hipStreamSynchronize(c->stream));
  return SKS_OK;
}

int sks_ctx_last_timings(const sks_ctx* c, sks_timings* out) {
  if (!c || !out) return sks::fail(SKS_E_ARG, "sks_ctx_last_timings: null argument");
  *out = c->last;
  return SKS_OK;
}

// Test/bench knob (not in sks.h): fixed scan grid size, 0 = occupancy-derived.
int sks_ctx_set_scan_grid(sks_ctx* c, int grid) {
  if (!c) return sks::fail(SKS_E_ARG, "null ctx");
  c->grid_override = grid;
  return SKS_OK;
}

int sks_ctx_set_frac_post(sks_ctx* c, int mode, uint32_t bucket_capacity, uint32_t buckets) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ctx_set_frac_post: null ctx");
  if (mode != SKS_FRAC_POST_AUTO && mode != SKS_FRAC_POST_GENERAL && mode != SKS_FRAC_POST_FUSED)
    return sks::fail(SKS_E_ARG, "sks_ctx_set_frac_post: unknown mode");
  if (buckets & (buckets - 1)) return sks::fail(SKS_E_ARG, "sks_ctx_set_frac_post: buckets must be a power of two");
  c->frac_mode = mode;
  c->frac_bucket_cap = bucket_capacity;
  c->frac_buckets = buckets;
  return SKS_OK;
}

int sks_ctx_last_build_path(const sks_ctx* c) { return c ? c->last_path : -1; }

int sks_ctx_set_intersect_kernel(sks_ctx* c, int kind) {
  if (!c) return sks::fail(SKS_E_ARG, "null ctx");
  if (kind < SKS_INTERSECT_AUTO || kind > SKS_INTERSECT_GLOBAL)
    return sks::fail(SKS_E_ARG, "sks_ctx_set_intersect_kernel: unknown kernel");
  c->intersect_algo = kind;
  return SKS_OK;
}

int sks_ctx_set_layout_blocks_hint(sks_ctx* c, uint32_t blocks) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ctx_set_layout_blocks_hint: null ctx");
  c->layout_blocks_hint = blocks;
  return SKS_OK;
}

int sks_ctx_ani_table(sks_ctx* c, uint32_t size, int kmer_num_ones) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ctx_ani_table: null ctx");
  if (kmer_num_ones <= 0) return sks::fail(SKS_E_ARG, "sks_ctx_ani_table: kmer_num_ones must be positive");
  if (size == 0 || size > SKS_ANI_TABLE_MAX) {
    c->root_k = 0;
    return SKS_OK;
  }
  if (c->root_k == kmer_num_ones && c->root_size == size) return SKS_OK;  // already built (stream order)
  DeviceGuard g(c->device);
  SKS_HIP(c->root.reserve(((size_t)size + 1) * sizeof(double)));
  SKS_HIP(sks::launch_ani_root(static_cast<double*>(c->root.ptr), size, kmer_num_ones, c->stream));
  c->root_size = size;
  c->root_k = kmer_num_ones;
  return SKS_OK;
}

int sks_ctx_set_join_check(sks_ctx* c, int on) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ctx_set_join_check: null ctx");
  c->join_check = on != 0;
  return SKS_OK;
}

int sks_ctx_join_check_violations(sks_ctx* c, uint64_t* violations) {
  if (!c || !violations) return sks::fail(SKS_E_ARG, "sks_ctx_join_check_violations: null argument");
  DeviceGuard g(c->device);
  SKS_HIP(hipStreamSynchronize(c->stream));
  *violations = sks::join_check_take() + sks::layout_check_take();
  return SKS_OK;
}

int sks_ctx_set_search_batch(sks_ctx* c, uint32_t ref_blocks) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ctx_set_search_batch: null ctx");
  c->search_batch = ref_blocks;
  return SKS_OK;
}

int sks_ctx_set_gather_rounds(sks_ctx* c, uint32_t rounds_per_wait) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_ctx_set_gather_rounds: null ctx");
  c->gather_rounds = rounds_per_wait;
  return SKS_OK;
}

// Device time of the last intersection call (after the stream has reached it).
int sks_ctx_last_intersect_ms(sks_ctx* c, float* ms) {
  if (!c || !ms) return sks::fail(SKS_E_ARG, "null argument");
  DeviceGuard g(c->device);
  SKS_HIP(hipEventSynchronize(c->ev_end));
  SKS_HIP(hipEventElapsedTime(ms, c->ev_begin, c->ev_end));
  return SKS_OK;
}

int sks_ctx_last_ingress_ms(sks_ctx* c, float* ms) {
  if (!c || !ms) return sks::fail(SKS_E_ARG, "null argument");
  DeviceGuard g(c->device);
  SKS_HIP(hipEventSynchronize(c->ev_i1));
  SKS_HIP(hipEventElapsedTime(ms, c->ev_i0, c->ev_i1));
  return SKS_OK;
}

// ---- pass-through wrappers: one launch on the context's stream ------------------------------

int sks_windows_dense_row_words(int window) { return window > 32 ? 4 : 3; }

int sks_windows_dense(sks_ctx* c, const uint8_t* d_seq, uint64_t n_bytes, uint64_t first, uint64_t n_windows,
                      int window, const uint64_t mask[2], uint64_t* d_rows, uint64_t* d_valid) {
  if (!c || !mask) return sks::fail(SKS_E_ARG, "sks_windows_dense: null argument");
  if (window < 1 || window > 64) return sks::fail(SKS_E_ARG, "sks_windows_dense: window must be 1..64");
  if (first > n_bytes) return sks::fail(SKS_E_ARG, "sks_windows_dense: first beyond the buffer");
  if (n_windows == 0) return SKS_OK;
  if (!d_seq || !d_rows || !d_valid) return sks::fail(SKS_E_ARG, "sks_windows_dense: null buffer");
  DeviceGuard g(c->device);
  SKS_HIP(sks::launch_windows_dense(d_seq, n_bytes, first, n_windows, window, mask[0], mask[1], d_rows, d_valid,
                                    c->stream));
  return SKS_OK;
}

int sks_sketch_union(sks_ctx* c, const uint64_t* d_in, uint64_t n, uint64_t* d_out, uint64_t* n_out) {
  if (!c || !n_out) return sks::fail(SKS_E_ARG, "sks_sketch_union: null argument");
  if (n && (!d_in || !d_out)) return sks::fail(SKS_E_ARG, "sks_sketch_union: null argument");
  if (n >= (1ull << 32)) return sks::fail(SKS_E_UNSUPPORTED, "sks_sketch_union: n >= 2^32");
  DeviceGuard g(c->device);
  SKS_HIP(sks::sort_unique_u64(d_in, n, d_out, n_out, c->iwork, c->stream));
  return SKS_OK;
}

int sks_sketch_union_wide(sks_ctx* c, const uint64_t* d_in, uint64_t n, uint64_t* d_out, uint64_t* n_out) {
  if (!c || !n_out) return sks::fail(SKS_E_ARG, "sks_sketch_union_wide: null argument");
  if (n && (!d_in || !d_out)) return sks::fail(SKS_E_ARG, "sks_sketch_union_wide: null argument");
  if (n >= (1ull << 32)) return sks::fail(SKS_E_UNSUPPORTED, "sks_sketch_union_wide: n >= 2^32");
  if ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 15)
    return sks::fail(SKS_E_ARG, "sks_sketch_union_wide: buffers must be 16-byte aligned");
  DeviceGuard g(c->device);
  SKS_HIP(sks::sort_unique_u128(d_in, n, d_out, n_out, c->iwork, c->stream));
  return SKS_OK;
}

int sks_sketches_export(sks_ctx* c, const uint64_t* d_data, const uint64_t* d_starts, const uint32_t* d_sizes,
                        int elem_words, uint32_t n, uint64_t* d_dst, uint64_t stride, uint32_t* d_dst_sizes) {
  if (!c) return sks::fail(SKS_E_ARG, "sks_sketches_export: null ctx");
  if (elem_words != 1 && elem_words != 2) return sks::fail(SKS_E_ARG, "elem_words must be 1 or 2");
  if (n && (!d_starts || !d_sizes || !d_dst || !d_dst_sizes || !stride))
    return sks::fail(SKS_E_ARG, "sks_sketches_export: null argument or zero stride");
  DeviceGuard g(c->device);
  SKS_HIP(sks::launch_export(d_data, d_starts, d_sizes, n, elem_words, d_dst, stride, d_dst_sizes, c->stream));
  return SKS_OK;
}

// ---- device FASTA ingress (ingress.hip) -----------------------------------------------------

int sks_fasta_parse_device(sks_ctx* c, const uint8_t* d_raw, uint64_t n_raw, uint8_t* d_stream, uint64_t stream_cap,
                           uint64_t* d_rec_end, uint64_t rec_cap, uint64_t* stream_bytes, uint64_t* n_records) {
  if (!c || !stream_bytes || !n_records || (n_raw && !d_raw))
    return sks::fail(SKS_E_ARG, "sks_fasta_parse_device: null argument");
  DeviceGuard g(c->device);
  bool too_small = false;
  SKS_HIP(hipEventRecord(c->ev_i0, c->stream));
  SKS_HIP(sks::fasta_parse_device(d_raw, n_raw, d_stream, stream_cap, d_rec_end, rec_cap, c->ingress,
                                  c->tmp, c->stream, stream_bytes, n_records, &too_small));
  SKS_HIP(hipEventRecord(c->ev_i1, c->stream));
  if (too_small)
    return sks::fail(SKS_E_LENGTH, "sks_fasta_parse_device: stream_cap or rec_cap too small for " +
                                       std::to_string(*stream_bytes) + " bytes / " +
                                       std::to_string(*n_records) + " records");
  return SKS_OK;
}

// ---- synthetic genomes ------------------------------------------------------------------------

int sks_synth_bases(sks_ctx* c, uint8_t* d_out, uint64_t n, uint64_t seed, uint64_t mut_seed,
                    double mut_rate, uint64_t pos_offset) {
  if (!c || (n && !d_out)) return sks::fail(SKS_E_ARG, "sks_synth_bases: null argument");
  uint64_t thr = 0;
  if (mut_rate > 0) {
    long double t = (long double)mut_rate * 18446744073709551616.0L;
    thr = t >= 18446744073709551615.0L ? ~0ull : (uint64_t)t;
  }
  DeviceGuard g(c->device);
  SKS_HIP(sks::launch_synth(d_out, n, seed, mut_seed, thr, pos_offset, c->stream));
  return SKS_OK;
}

}  // extern "C"
