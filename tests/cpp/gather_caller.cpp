// sks::gather_hits (cpp/search.hpp) on sets sketched from FASTA files: the first
// file is the query, the others are the references.  Prints JSON for
// tests/test_gather_facade.py (doubles as hex floats).
//   gather_caller <w> <k> <c> <min_shared> <max_rounds> <query file> <reference file>...
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kmer.hpp"
#include "search.hpp"

int main(int argc, char* argv[]) {
  if (argc < 8) return 64;
  const int w = std::atoi(argv[1]), k = std::atoi(argv[2]);
  const unsigned long long c = std::strtoull(argv[3], nullptr, 10);
  const int min_shared = std::atoi(argv[4]), max_rounds = std::atoi(argv[5]);
  const int num_files = argc - 6;
  const kmer_bitset mask = generate_random_spaced_seed_mask(w, k);
  const std::vector<kmer_set> sets =
      parallel_kmer_sets_from_fasta_files(num_files, argv + 6, mask, w, sketch_policy::frac(c));
  const std::vector<kmer_set> refs(sets.begin() + 1, sets.end());
  const std::vector<sks::gather_hit> hits = sks::gather_hits(sets[0], refs, min_shared, max_rounds);

  // on the host: every hit's shared is the facade's own intersection, and the
  // rounds' shared_new add up to what the hits' references hold of the query together
  int mismatches = 0;
  long long explained = 0;
  for (const sks::gather_hit& h : hits) {
    if (h.ref >= refs.size() || h.shared != kmer_set_intersection(sets[0], refs[h.ref]) ||
        h.ref_size != refs[h.ref].kmer_set_size() || h.shared_new > h.shared || h.shared_new < 1)
      ++mismatches;
    explained += h.shared_new;
  }
  if (explained > sets[0].kmer_set_size()) ++mismatches;

  std::printf("{\"query_size\":%d,\"sizes\":[", sets[0].kmer_set_size());
  for (size_t i = 0; i < refs.size(); ++i) std::printf("%s%d", i ? "," : "", refs[i].kmer_set_size());
  std::printf("],\"mismatches\":%d,\"hits\":[", mismatches);
  for (size_t i = 0; i < hits.size(); ++i)
    std::printf("%s[%u,%d,%d,%d,\"%a\",\"%a\"]", i ? "," : "", hits[i].ref, hits[i].shared, hits[i].shared_new,
                hits[i].ref_size, hits[i].f_query_new, hits[i].ani);
  std::printf("]}\n");
  return mismatches ? 1 : 0;
}
