// C-ABI implementation (include/sks.h): the ordered k-mer lists
// (nucleotide_string_list_to_kmers).
#include <memory>

#include "build_internal.hpp"

using namespace sks;

extern "C" {

int sks_kmer_list_build(sks_ctx* c, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* seg_off, uint32_t n_seg,
                        int window, const uint64_t mask[2], const sks_policy* policy, sks_kmer_list** out) {
  if (!out) return sks::fail(SKS_E_ARG, "sks_kmer_list_build: null argument");
  *out = nullptr;
  SKS_TRY(validate_build("sks_kmer_list_build", c, d_seq, n_bytes, seg_off, n_seg, window, mask, policy));
  if (policy->kind != SKS_FRAC_MOD)
    return sks::fail(SKS_E_UNSUPPORTED,
                     "sks_kmer_list_build: lists take a per-k-mer predicate (SKS_FRAC_MOD); "
                     "bottom-s is a set selection");
  DeviceGuard guard(c->device);
  hipStream_t st = c->stream;
  const BuildState S = build_state(c, window, mask, *policy);
  std::vector<uint64_t> cap(n_seg), counts(n_seg, 0);
  for (uint32_t g = 0; g < n_seg; ++g)
    cap[g] = sks::plan_segment(false, policy->param, seg_off[g + 1] - seg_off[g]).cap;
  ScanSegs seg;
  for (int pass = 0; pass < 2; ++pass) {  // pass 2 only if a capacity estimate overflowed
    seg = ScanSegs{};
    for (uint32_t g = 0; g < n_seg; ++g) seg.push(seg_off[g], seg_off[g + 1], ~0ull, cap[g]);
    SKS_HIP(c->rec[0].reserve(std::max<uint64_t>(seg.total_cap, 1) * sizeof(uint64_t)));
    ScanMeta meta;
    SKS_TRY(scan_meta(S, d_seq, seg, true, {}, 0, &meta));
    SKS_HIP(sks::launch_scan(meta.p, sks::kModeList, policy->flavour, S.wide, c->device, st, c->grid_override));
    SKS_HIP(sks::pinned_d2h(counts.data(), meta.counters, n_seg * sizeof(uint64_t), st));
    bool overflow = false;
    for (uint32_t g = 0; g < n_seg; ++g)
      if (counts[g] > cap[g]) {
        overflow = true;
        cap[g] = counts[g];
      }
    if (!overflow) break;
    if (pass == 1) return sks::fail(SKS_E_HIP, "sks_kmer_list_build: survivor count changed between passes");
  }
  // dense positions (segments in stream order), then one sort: stream order
  std::vector<uint64_t> csr = prefix(counts);
  const uint64_t T = csr[n_seg];
  uint64_t max_len = 0;
  for (uint64_t v : counts) max_len = std::max(max_len, v);
  std::unique_ptr<sks_kmer_list> kl(new (std::nothrow) sks_kmer_list());
  if (!kl) return sks::fail(SKS_E_NOMEM, "sks_kmer_list_build: out of memory");
  kl->device = c->device;
  kl->n = n_seg;
  kl->total = T;
  kl->counts = counts;
  SKS_TRY(alloc_u64(kl->pos, T, st));
  SKS_TRY(alloc_u64(kl->bits, 4 * T, st));
  SKS_TRY(reserve_cols(c, {0}, T + 1));
  MetaArena arena(c);
  size_t o_src = arena.add(seg.off), o_csr = arena.add(csr), o_beg = arena.add(seg.beg);
  SKS_TRY(arena.upload());
  if (T) {
    uint64_t* d_pos = kl->pos.as<uint64_t>();
    SKS_HIP(sks::compact_regions(reinterpret_cast<uint64_t*>(c->rec[0].ptr), col(c, 0), arena.ptr(o_src),
                                 arena.ptr(o_csr), n_seg, max_len, st));
    SKS_HIP(sks::seg_sort_keys(col(c, 0), d_pos, T, {0, T}, nullptr, end_bit_of(n_bytes), c->tmp, st));
    SKS_HIP(sks::launch_materialise(d_seq, arena.ptr(o_beg), n_seg, d_pos, T, window, mask[0], mask[1],
                                    kl->bits.as<uint64_t>(), st));
    SKS_HIP(hipStreamSynchronize(st));
  }
  *out = kl.release();
  return SKS_OK;
}

int sks_kmer_list_free(sks_kmer_list* kl) {
  if (!kl) return SKS_OK;
  DeviceGuard g(kl->device);
  // as hipFree would: work queued on the arrays completes before they are reused
  if (kl->pos || kl->bits) (void)hipDeviceSynchronize();
  kl->pos.release();
  kl->bits.release();
  delete kl;
  return SKS_OK;
}

uint64_t sks_kmer_list_total(const sks_kmer_list* kl) { return kl ? kl->total : 0; }

int sks_kmer_list_counts(const sks_kmer_list* kl, uint64_t* counts) {
  if (!kl || (!counts && kl->n)) return sks::fail(SKS_E_ARG, "sks_kmer_list_counts: null argument");
  std::copy(kl->counts.begin(), kl->counts.end(), counts);
  return SKS_OK;
}

const uint64_t* sks_kmer_list_device_positions(const sks_kmer_list* kl) {
  return kl ? kl->pos.as<uint64_t>() : nullptr;
}
const uint64_t* sks_kmer_list_device_bits(const sks_kmer_list* kl) { return kl ? kl->bits.as<uint64_t>() : nullptr; }

int sks_kmer_list_copy(const sks_kmer_list* kl, uint64_t* positions, uint64_t* bits) {
  if (!kl) return sks::fail(SKS_E_ARG, "sks_kmer_list_copy: null list");
  DeviceGuard g(kl->device);
  if (positions && kl->total)
    SKS_HIP(hipMemcpy(positions, kl->pos.as<uint64_t>(), kl->total * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (bits && kl->total)
    SKS_HIP(hipMemcpy(bits, kl->bits.as<uint64_t>(), kl->total * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SKS_OK;
}

}  // extern "C"
