// sks::search_hits (cpp/search.hpp) on sets sketched from FASTA files, compared
// in place with the facade's own kmer_set_intersection / containment /
// binomial_estimator over every (query, ref) pair.  Prints JSON for
// tests/test_search_facade.py.
//   search_caller <w> <k> <c> <min_containment> <min_shared> <file>...
// The files are both the queries and the references.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ani_estimator.hpp"
#include "kmer.hpp"
#include "search.hpp"

int main(int argc, char* argv[]) {
  if (argc < 7) return 64;
  const int w = std::atoi(argv[1]), k = std::atoi(argv[2]);
  const unsigned long long c = std::strtoull(argv[3], nullptr, 10);
  const double min_containment = std::strtod(argv[4], nullptr);
  const int min_shared = std::atoi(argv[5]);
  const int num_files = argc - 6;
  const kmer_bitset mask = generate_random_spaced_seed_mask(w, k);
  const int ones = (int)mask.count() / NUCLEOTIDE_BIT_SIZE;
  const std::vector<kmer_set> sets =
      parallel_kmer_sets_from_fasta_files(num_files, argv + 6, mask, w, sketch_policy::frac(c));
  const std::vector<sks::search_hit> hits = sks::search_hits(sets, sets, min_containment, min_shared);

  // the expected list, pair by pair on the host, in (query, ref) order
  int mismatches = 0;
  size_t at = 0, sharing = 0;
  for (size_t q = 0; q < sets.size(); ++q)
    for (size_t r = 0; r < sets.size(); ++r) {
      const int shared = kmer_set_intersection(sets[q], sets[r]);
      if (shared > 0) ++sharing;
      const double cont = containment(shared, sets[q].kmer_set_size());
      if (shared < (min_shared < 1 ? 1 : min_shared) || cont < min_containment) continue;
      if (at >= hits.size()) {
        ++mismatches;
        continue;
      }
      const sks::search_hit& h = hits[at++];
      const double ani = binomial_estimator(cont, ones);
      if (h.query != q || h.ref != r || h.shared != shared || h.containment != cont ||
          !(std::fabs(h.ani - ani) <= 1e-9))
        ++mismatches;
    }
  if (at != hits.size()) ++mismatches;

  std::printf("{\"k\":%d,\"sizes\":[", ones);
  for (size_t i = 0; i < sets.size(); ++i) std::printf("%s%d", i ? "," : "", sets[i].kmer_set_size());
  std::printf("],\"sharing_pairs\":%zu,\"mismatches\":%d,\"hits\":[", sharing, mismatches);
  for (size_t i = 0; i < hits.size(); ++i)
    std::printf("%s[%u,%u,%d,\"%a\",\"%a\"]", i ? "," : "", hits[i].query, hits[i].ref, hits[i].shared,
                hits[i].containment, hits[i].ani);
  std::printf("]}\n");
  return mismatches ? 1 : 0;
}
