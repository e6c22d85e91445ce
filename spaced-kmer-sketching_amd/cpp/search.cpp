// sks::search_hits: the facade's kmer_sets through sks_search.
#include "search.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

#include "facade_internal.hpp"
#include "sks.h"

namespace sks {
namespace {

// One vector of kmer_sets resident on the facade's device in the C ABI's
// sketch layout (data, starts, sizes).
struct ResidentSets {
  DevMem words, starts, sizes;
  uint32_t n = 0, max_size = 0;
  uint64_t total = 0;
  ResidentSets(const std::vector<kmer_set>& sets, int ew)
      : words(count(sets) * 8 * ew), starts(sets.size() * 8), sizes(sets.size() * 4), n((uint32_t)sets.size()) {
    std::vector<uint64_t> h_words, h_starts(sets.size());
    std::vector<uint32_t> h_sizes(sets.size());
    h_words.reserve(count(sets) * ew);
    for (size_t i = 0; i < sets.size(); ++i) {
      h_starts[i] = total;
      h_sizes[i] = (uint32_t)sets[i].elements.size();
      max_size = std::max(max_size, h_sizes[i]);
      total += h_sizes[i];
      for (const kmer_bitset& e : sets[i].elements) {
        h_words.push_back(e.lo());
        if (ew == 2) h_words.push_back(e.hi());
      }
    }
    if (!h_words.empty())
      check_hip(hipMemcpy(words.p, h_words.data(), h_words.size() * 8, hipMemcpyHostToDevice), "H2D");
    if (n) {
      check_hip(hipMemcpy(starts.p, h_starts.data(), h_starts.size() * 8, hipMemcpyHostToDevice), "H2D");
      check_hip(hipMemcpy(sizes.p, h_sizes.data(), h_sizes.size() * 4, hipMemcpyHostToDevice), "H2D");
    }
  }
  static size_t count(const std::vector<kmer_set>& sets) {
    size_t t = 0;
    for (const kmer_set& s : sets) t += s.elements.size();
    return t;
  }
};

}  // namespace

std::vector<search_hit> search_hits(const std::vector<kmer_set>& queries, const std::vector<kmer_set>& refs,
                                    double min_containment, int min_shared) {
  // one mask for every set that holds k-mers (identity includes the mask, kmer.hpp:82-85)
  const kmer_set* first = nullptr;
  for (const std::vector<kmer_set>* v : {&queries, &refs})
    for (const kmer_set& s : *v) {
      if (!s.other_masks.empty()) throw std::invalid_argument("search_hits: a set holds k-mers of several masks");
      if (!s.has_mask || s.elements.empty()) continue;
      if (!first) first = &s;
      if (!(s.mask == first->mask) || s.window_length != first->window_length)
        throw std::invalid_argument("search_hits: the sets differ in mask or window");
    }
  std::vector<search_hit> out;
  if (!first || queries.empty() || refs.empty()) return out;
  const int ew = first->mask.hi() ? 2 : 1;
  const int k = (int)first->mask.count() / NUCLEOTIDE_BIT_SIZE;
  if (k <= 0) throw std::invalid_argument("search_hits: the mask selects no position");
  sks_ctx* c = ctx();
  const ResidentSets Q(queries, ew), R(refs, ew);
  auto call = [&](sks_hit* d_hits, uint64_t cap, uint64_t* n) {
    check(sks_search(c, Q.words.as<uint64_t>(), Q.starts.as<uint64_t>(), Q.sizes.as<uint32_t>(), Q.n, Q.max_size,
                     Q.total, R.words.as<uint64_t>(), R.starts.as<uint64_t>(), R.sizes.as<uint32_t>(), R.n,
                     R.max_size, R.total, ew, k, min_containment, min_shared, d_hits, cap, n));
  };
  uint64_t n = 0;
  call(nullptr, 0, &n);  // size query, then a buffer of exactly that many records
  if (!n) return out;
  DevMem d_hits(n * sizeof(sks_hit));
  call(d_hits.as<sks_hit>(), n, &n);
  check(sks_ctx_synchronize(c));
  std::vector<sks_hit> h(n);
  check_hip(hipMemcpy(h.data(), d_hits.p, n * sizeof(sks_hit), hipMemcpyDeviceToHost), "D2H");
  out.reserve(n);
  for (const sks_hit& x : h) out.push_back(search_hit{x.query, x.ref, x.shared, x.containment, x.ani});
  return out;
}

std::vector<gather_hit> gather_hits(const kmer_set& query, const std::vector<kmer_set>& refs, int min_shared,
                                    int max_rounds) {
  if (max_rounds < 0) throw std::invalid_argument("gather_hits: max_rounds is negative");
  if (!query.other_masks.empty()) throw std::invalid_argument("gather_hits: a set holds k-mers of several masks");
  std::vector<gather_hit> out;
  if (!query.has_mask || query.elements.empty() || refs.empty()) return out;
  for (const kmer_set& s : refs) {
    if (!s.other_masks.empty()) throw std::invalid_argument("gather_hits: a set holds k-mers of several masks");
    if (!s.has_mask || s.elements.empty()) continue;
    if (!(s.mask == query.mask) || s.window_length != query.window_length)
      throw std::invalid_argument("gather_hits: the sets differ in mask or window");
  }
  const int ew = query.mask.hi() ? 2 : 1;
  const int k = (int)query.mask.count() / NUCLEOTIDE_BIT_SIZE;
  if (k <= 0) throw std::invalid_argument("gather_hits: the mask selects no position");
  sks_ctx* c = ctx();
  const ResidentSets Q(std::vector<kmer_set>{query}, ew), R(refs, ew);
  // min(refs, query elements) records always suffice: one call
  const uint64_t cap = std::min<uint64_t>(R.n, Q.total);
  DevMem d_hits(cap * sizeof(sks_gather_hit));
  uint64_t n = 0;
  check(sks_gather(c, Q.words.as<uint64_t>(), (uint32_t)Q.total, R.words.as<uint64_t>(), R.starts.as<uint64_t>(),
                   R.sizes.as<uint32_t>(), R.n, R.max_size, R.total, ew, k, min_shared, (uint32_t)max_rounds,
                   d_hits.as<sks_gather_hit>(), cap, &n, nullptr));
  check(sks_ctx_synchronize(c));
  if (!n) return out;
  std::vector<sks_gather_hit> h(n);
  check_hip(hipMemcpy(h.data(), d_hits.p, n * sizeof(sks_gather_hit), hipMemcpyDeviceToHost), "D2H");
  out.reserve(n);
  for (const sks_gather_hit& x : h)
    out.push_back(gather_hit{x.ref, x.shared, x.shared_new, x.ref_size, x.f_query_new, x.ani});
  return out;
}

}  // namespace sks
