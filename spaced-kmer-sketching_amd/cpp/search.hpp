// search.hpp — query-vs-reference search over the facade's kmer_sets (no
// reference equivalent): sks_search of libsks.so on host sets.
#pragma once

#include <vector>

#include "kmer.hpp"

namespace sks {

struct search_hit {
  uint32_t query, ref;  // indices into the two vectors
  int shared;           // kmer_set_intersection(queries[query], refs[ref])
  double containment;   // containment(shared, queries[query].kmer_set_size())
  double ani;           // binomial_estimator(containment, mask.count() / NUCLEOTIDE_BIT_SIZE)
};

// Every (query, ref) pair sharing at least max(min_shared, 1) k-mers whose
// containment is >= min_containment, in ascending (query, ref) order.  Both
// vectors are uploaded once (device-resident for the call) and compared on the
// GPU in reference batches; only the hits come back.  Every non-empty set must
// hold k-mers of one common mask (std::invalid_argument otherwise).
std::vector<search_hit> search_hits(const std::vector<kmer_set>& queries, const std::vector<kmer_set>& refs,
                                    double min_containment, int min_shared);

struct gather_hit {
  uint32_t ref;        // index into refs
  int shared;          // kmer_set_intersection(query, refs[ref])
  int shared_new;      // the query elements this round explains (those no earlier hit held)
  int ref_size;        // refs[ref].kmer_set_size()
  double f_query_new;  // containment(shared_new, query.kmer_set_size())
  double ani;          // binomial_estimator(containment(shared, ref_size), mask.count() / NUCLEOTIDE_BIT_SIZE)
};

// The greedy min-set cover of `query` by `refs` (sks_gather): each round reports
// the reference sharing the most still unexplained query k-mers, ties to the
// smallest index, while that is at least max(min_shared, 1) and fewer than
// max_rounds rounds were reported (0: no limit), then removes its k-mers from
// the query.  Hits in round order.  The sets are uploaded once, like
// search_hits, and must hold k-mers of one common mask.
std::vector<gather_hit> gather_hits(const kmer_set& query, const std::vector<kmer_set>& refs, int min_shared,
                                    int max_rounds = 0);

}  // namespace sks
