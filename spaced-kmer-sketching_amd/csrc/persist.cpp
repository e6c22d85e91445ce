// The sketch file format, host only (the entry points that move sets between a
// device and files are in sketch_set.cpp).
//
// Persisted sketches (no reference equivalent — the
// reference re-parses and re-sketches every FASTA for each of its 62
// configurations, kmer-sketching.cpp:168).
//
// File format "SKSKETCH", little-endian, 8-byte aligned sections.
// Version 1 (one window / mask for the whole file; every C-ABI set without
// abundances) and version 3 (the same with an abundance per element; a counted set):
//   header (96 bytes)
//     char     magic[8]   = "SKSKETCH"
//     uint32   version    = 1, 2 or 3
//     uint32   elem_words   1 (window <= 32: one u64 per k-mer) or 2 (lo, hi)
//     int32    window       w of the spaced seed
//     int32    policy_kind  sks_policy_kind
//     int32    flavour      sks_hash_flavour
//     int32    reserved     0
//     uint64   param        c (FracMinHash) or s (bottom-s)
//     int64    nonce
//     uint64   mask_lo, mask_hi
//     uint64   n            sketches
//     uint64   total        elements over all sketches
//     uint64   names_bytes  0, or the size of the name table
//     uint64   groups       0 (version 1); the group count (version 2)
//   uint32 sizes[n]           (zero-padded to a multiple of 8 bytes)
//   uint64 windows[n]         k-mer windows hashed per genome
//   [version 2 only] group table, `groups` entries of 32 bytes:
//     uint32 set, int32 window, uint64 mask_lo, uint64 mask_hi, uint64 size
//   uint64 data[total * elem_words]   each sketch (v1, v3) / group (v2) sorted ascending, unique
//   [version 3 only] uint32 abund[total]   the abundance (>= 1) of every element, in data's order
//                             (zero-padded to a multiple of 8 bytes)
//   char   names[names_bytes] n NUL-terminated strings (when names_bytes > 0)
//   uint64 checksum           FNV-1a 64 of every byte before it
// Version 2 is what the C++ facade writes for kmer_sets the reference allows but
// version 1 cannot hold (kmer.hpp:170-178 accepts any mix of masks): a set is a
// list of (window, mask) groups in set order, sizes[i] = the sum of set i's
// group sizes, and the header's window / mask are the first group's.  The C ABI
// reads versions 1 and 3 (an sks_sketch_set has one mask); a set without
// abundances is written as version 1, byte for byte as before version 3 existed.
// The facade reads versions 1 and 2 and rejects 3 (a kmer_set has no counts).
// A reader rejects a wrong magic / version, inconsistent sizes, a truncated
// or over-long file, a checksum mismatch, unsorted sketches and a zero abundance
// (SKS_E_IO).
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "abund_plan.hpp"
#include "sks.h"
#include "sks_api_internal.hpp"

namespace sks {

namespace {

constexpr char kMagic[8] = {'S', 'K', 'S', 'K', 'E', 'T', 'C', 'H'};
constexpr uint32_t kVersion = 1;
constexpr uint32_t kVersionGroups = 2;
constexpr uint32_t kVersionAbund = 3;

struct Header {
  char magic[8];
  uint32_t version;
  uint32_t elem_words;
  int32_t window;
  int32_t policy_kind;
  int32_t flavour;
  int32_t reserved0;
  uint64_t param;
  int64_t nonce;
  uint64_t mask_lo, mask_hi;
  uint64_t n;
  uint64_t total;
  uint64_t names_bytes;
  uint64_t groups;
};
static_assert(sizeof(Header) == 96, "sketch file header layout");

struct GroupRec {
  uint32_t set;
  int32_t window;
  uint64_t mask_lo, mask_hi;
  uint64_t size;
};
static_assert(sizeof(GroupRec) == 32, "sketch file group layout");

struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void add(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  }
};

size_t pad8(size_t x) { return (x + 7) & ~size_t(7); }

// Writes through a FILE*, hashing every byte.
struct Writer {
  FILE* f;
  Fnv fnv;
  bool ok = true;
  void put(const void* p, size_t n) {
    if (!n || !ok) return;
    fnv.add(p, n);
    ok = fwrite(p, 1, n, f) == n;
  }
};

bool less128(const uint64_t* a, const uint64_t* b, int ew) {
  if (ew == 1) return a[0] < b[0];
  return a[1] < b[1] || (a[1] == b[1] && a[0] < b[0]);
}

int write_impl(const char* path, const SketchFileMeta& meta, const std::vector<uint32_t>& sizes,
               const std::vector<uint64_t>& windows, const std::vector<SketchGroup>* groups,
               const uint64_t* data, const std::vector<std::string>& names,
               const std::vector<uint32_t>* abund = nullptr) {
  if (!path) return fail(SKS_E_ARG, "sketch file: null path");
  if (windows.size() != sizes.size() || (!names.empty() && names.size() != sizes.size()))
    return fail(SKS_E_ARG, "sketch file: names / windows must match the number of sketches");
  if (abund && groups) return fail(SKS_E_ARG, "sketch file: a grouped set holds no abundances");
  Header h{};
  std::memcpy(h.magic, kMagic, 8);
  h.version = groups ? kVersionGroups : (abund ? kVersionAbund : kVersion);
  h.elem_words = (uint32_t)meta.elem_words;
  h.window = meta.window;
  h.policy_kind = meta.policy.kind;
  h.flavour = meta.policy.flavour;
  h.param = meta.policy.param;
  h.nonce = meta.policy.nonce;
  h.mask_lo = meta.mask[0];
  h.mask_hi = meta.mask[1];
  h.n = sizes.size();
  for (uint32_t v : sizes) h.total += v;
  std::vector<GroupRec> recs;
  if (groups) {
    uint64_t gtotal = 0;
    for (const SketchGroup& g : *groups) {
      if (g.set >= sizes.size()) return fail(SKS_E_ARG, "sketch file: group names a missing set");
      recs.push_back(GroupRec{g.set, g.window, g.mask[0], g.mask[1], g.size});
      gtotal += g.size;
    }
    if (gtotal != h.total) return fail(SKS_E_ARG, "sketch file: group sizes do not add up");
    h.groups = recs.size();
  }
  if (abund && abund->size() != h.total)
    return fail(SKS_E_ARG, "sketch file: one abundance per element is needed");
  std::string table;
  for (const std::string& s : names) {
    if (s.find('\0') != std::string::npos) return fail(SKS_E_ARG, "sketch file: name contains NUL");
    table += s;
    table.push_back('\0');
  }
  h.names_bytes = table.size();
  FILE* f = fopen(path, "wb");
  if (!f) return fail(SKS_E_IO, std::string("sketch file: cannot open ") + path + ": " + strerror(errno));
  Writer w{f};
  w.put(&h, sizeof h);
  w.put(sizes.data(), sizes.size() * 4);
  const uint64_t zero = 0;
  w.put(&zero, pad8(sizes.size() * 4) - sizes.size() * 4);
  w.put(windows.data(), windows.size() * 8);
  w.put(recs.data(), recs.size() * sizeof(GroupRec));
  w.put(data, h.total * h.elem_words * 8);
  if (abund) {
    w.put(abund->data(), h.total * 4);
    w.put(&zero, abund_section_bytes(h.total) - h.total * 4);
  }
  w.put(table.data(), table.size());
  const uint64_t sum = w.fnv.h;
  if (w.ok) w.ok = fwrite(&sum, 1, 8, f) == 8;
  const bool closed = fclose(f) == 0;
  if (!w.ok || !closed) return fail(SKS_E_IO, std::string("sketch file: write failed for ") + path);
  return SKS_OK;
}

int read_impl(const char* path, SketchFileMeta& meta, std::vector<uint32_t>& sizes,
              std::vector<uint64_t>& windows, std::vector<uint64_t>& data,
              std::vector<std::string>& names, std::vector<SketchGroup>* groups,
              bool* grouped_out = nullptr, std::vector<uint32_t>* abund = nullptr, bool* counted_out = nullptr) {
  if (!path) return fail(SKS_E_ARG, "sketch file: null path");
  FILE* f = fopen(path, "rb");
  if (!f) return fail(SKS_E_IO, std::string("sketch file: cannot open ") + path);
  std::vector<uint8_t> buf;
  uint8_t tmp[1 << 16];
  size_t got;
  while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  const bool rd_ok = !ferror(f);
  fclose(f);
  const std::string where = std::string("sketch file ") + path + ": ";
  if (!rd_ok) return fail(SKS_E_IO, where + "read error");
  if (buf.size() < sizeof(Header) + 8) return fail(SKS_E_IO, where + "truncated");
  Header h;
  std::memcpy(&h, buf.data(), sizeof h);
  if (std::memcmp(h.magic, kMagic, 8) != 0) return fail(SKS_E_IO, where + "not a sketch file");
  if (h.version == kVersionGroups && !groups)
    return fail(SKS_E_IO, where + "version 2 (kmer_sets with several masks): load it with sks::load_kmer_sets");
  const bool counted = h.version == kVersionAbund && abund;  // only for a reader that takes abundances
  if (h.version != kVersion && h.version != kVersionGroups && !counted)
    return fail(SKS_E_IO, where + "unsupported version " + std::to_string(h.version));
  const bool grouped = h.version == kVersionGroups;
  if (h.window < 1 || h.window > 64 || h.elem_words < 1 || h.elem_words > 2 ||
      (!grouped && h.elem_words != (h.window > 32 ? 2u : 1u)))
    return fail(SKS_E_IO, where + "bad window / element width");
  if (h.n > (1ull << 32) || h.total > (1ull << 40) || (!grouped && h.groups) || h.groups > (1ull << 32))
    return fail(SKS_E_IO, where + "bad counts");
  // every region must fit in the file before any offset past it is formed: the
  // counts are bounded above, so o_names cannot wrap; names_bytes is checked
  // against the bytes left rather than added first
  const size_t o_sizes = sizeof(Header);
  const size_t o_win = o_sizes + pad8(h.n * 4);
  const size_t o_groups = o_win + h.n * 8;
  const size_t o_data = o_groups + h.groups * sizeof(GroupRec);
  const size_t o_abund = o_data + h.total * h.elem_words * 8;
  const size_t o_names = o_abund + (counted ? abund_section_bytes(h.total) : 0);
  const size_t body = buf.size() - 8;  // bytes before the checksum
  if (o_names > body || h.names_bytes > body - o_names)
    return fail(SKS_E_IO, where + "length does not match the header");
  const size_t o_sum = o_names + h.names_bytes;
  if (o_sum != body) return fail(SKS_E_IO, where + "length does not match the header");
  Fnv fnv;
  fnv.add(buf.data(), o_sum);
  uint64_t sum;
  std::memcpy(&sum, buf.data() + o_sum, 8);
  if (sum != fnv.h) return fail(SKS_E_IO, where + "checksum mismatch");
  sizes.resize(h.n);
  windows.resize(h.n);
  data.resize(h.total * h.elem_words);
  std::memcpy(sizes.data(), buf.data() + o_sizes, h.n * 4);
  std::memcpy(windows.data(), buf.data() + o_win, h.n * 8);
  if (!data.empty()) std::memcpy(data.data(), buf.data() + o_data, data.size() * 8);
  uint64_t total = 0;
  for (uint32_t v : sizes) total += v;
  if (total != h.total) return fail(SKS_E_IO, where + "sizes do not add up");
  if (counted) {
    abund->resize(h.total);
    if (h.total) std::memcpy(abund->data(), buf.data() + o_abund, h.total * 4);
    for (uint32_t a : *abund)
      if (a == 0) return fail(SKS_E_IO, where + "an abundance is zero");
  }
  if (counted_out) *counted_out = counted;
  const int ew = (int)h.elem_words;
  // runs that must each be sorted and unique: the sketches (v1) or the groups (v2)
  std::vector<uint64_t> runs;
  if (grouped) {
    std::vector<GroupRec> recs(h.groups);
    if (!recs.empty()) std::memcpy(recs.data(), buf.data() + o_groups, recs.size() * sizeof(GroupRec));
    std::vector<uint64_t> per_set(h.n, 0);
    groups->clear();
    uint32_t prev_set = 0;
    for (const GroupRec& r : recs) {
      if (r.set >= h.n || r.set < prev_set || r.window < 1 || r.window > 64 ||
          (r.window > 32 && ew != 2) || r.size > h.total)
        return fail(SKS_E_IO, where + "bad group table");
      prev_set = r.set;
      per_set[r.set] += r.size;
      runs.push_back(r.size);
      groups->push_back(SketchGroup{r.set, r.window, {r.mask_lo, r.mask_hi}, r.size});
    }
    for (uint64_t i = 0; i < h.n; ++i)
      if (per_set[i] != sizes[i]) return fail(SKS_E_IO, where + "group sizes do not add up");
  } else {
    runs.assign(sizes.begin(), sizes.end());
  }
  uint64_t e = 0;
  for (uint64_t v : runs) {
    for (uint64_t i = 1; i < v; ++i)
      if (!less128(&data[(e + i - 1) * ew], &data[(e + i) * ew], ew))
        return fail(SKS_E_IO, where + "a sketch is not sorted and unique");
    e += v;
  }
  names.clear();
  if (h.names_bytes) {
    const char* p = reinterpret_cast<const char*>(buf.data() + o_names);
    const char* end = p + h.names_bytes;
    if (end[-1] != '\0') return fail(SKS_E_IO, where + "name table not terminated");
    while (p < end) {
      names.emplace_back(p);
      p += names.back().size() + 1;
    }
    if (names.size() != h.n) return fail(SKS_E_IO, where + "name count does not match");
  }
  meta.window = h.window;
  meta.elem_words = ew;
  meta.mask[0] = h.mask_lo;
  meta.mask[1] = h.mask_hi;
  meta.policy = sks_policy{h.policy_kind, h.flavour, h.param, h.nonce};
  if (grouped_out) *grouped_out = grouped;
  return SKS_OK;
}

}  // namespace

int write_sketch_file(const char* path, const SketchFileMeta& meta, const std::vector<uint32_t>& sizes,
                      const std::vector<uint64_t>& windows, const uint64_t* data,
                      const std::vector<std::string>& names, const std::vector<uint32_t>* abund) {
  return write_impl(path, meta, sizes, windows, nullptr, data, names, abund);
}

int write_sketch_file_groups(const char* path, const SketchFileMeta& meta,
                             const std::vector<uint32_t>& sizes, const std::vector<uint64_t>& windows,
                             const std::vector<SketchGroup>& groups, const uint64_t* data,
                             const std::vector<std::string>& names) {
  return write_impl(path, meta, sizes, windows, &groups, data, names);
}

int read_sketch_file(const char* path, SketchFileMeta& meta, std::vector<uint32_t>& sizes,
                     std::vector<uint64_t>& windows, std::vector<uint64_t>& data,
                     std::vector<std::string>& names, std::vector<uint32_t>* abund, bool* counted) {
  if (counted) *counted = false;
  return read_impl(path, meta, sizes, windows, data, names, nullptr, nullptr, abund, counted);
}

int read_sketch_file_any(const char* path, SketchFileMeta& meta, std::vector<uint32_t>& sizes,
                         std::vector<uint64_t>& windows, std::vector<uint64_t>& data,
                         std::vector<std::string>& names, std::vector<SketchGroup>& groups,
                         bool& grouped) {
  grouped = false;
  return read_impl(path, meta, sizes, windows, data, names, &groups, &grouped);
}

}  // namespace sks
