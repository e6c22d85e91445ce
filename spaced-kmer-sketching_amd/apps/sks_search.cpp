// sks-search — a sketch database and thresholded queries against it, on the
// C ABI (include/sks.h); no reference counterpart.
//
//   sks-search index <out.sks> <w> <k> <c> <a.fa> <b.fa> ...
//       one FracMinHash sketch (1/c) per FASTA file under the seed-0 spaced mask
//       of (w, k), stored with the file names (sks_sketch_set_save)
//   sks-search index-abund <out.sks> <w> <k> <c> <min> <max|-> <a.fa> <b.fa> ...
//       as index, but counted (sks_sketch_build_counted): every kept k-mer with
//       the number of times it was selected in its file, and only the k-mers
//       selected <min> .. <max> times (- for no maximum; min 2 drops the k-mers
//       seen once, the sequencing errors of raw reads)
//   sks-search weigh <sample.sks> <db.sks> <min_containment> <out.csv>
//       the pairs query finds between the sketches of a counted database
//       (index-abund) and a reference database (sks_search_sets), each with the
//       sample's abundances over the shared k-mers (sks_abund_pairs):
//         Query,Reference,Shared,Containment,ANI,Weight,MeanDepth,FWeighted   (doubles as %.17g)
//       MeanDepth = Weight / Shared, FWeighted = Weight / the sum of the query's abundances
//   sks-search query <db.sks> <min_containment> <out.csv> <q.fa> ...
//       sketches the queries with the database's window, mask and policy and
//       writes every (query, reference) pair whose containment of the query is
//       at least min_containment (sks_search_sets):
//         Query,Reference,Shared,Containment,ANI     (doubles as %.17g)
//   sks-search downsample <in.sks> <c> <out.sks>
//       a coarser copy of a database (sks_sketch_set_downsample): FracMinHash 1/c
//       with c a multiple of the database's, or bottom-s with a smaller s; the
//       result equals a database indexed at c directly, names kept
//   sks-search merge <out.sks> <groups.tsv> <in.sks> [<in.sks> ...]
//       one sketch per group, the union of the sketches the group lists
//       (sks_sketch_set_merge): groups.tsv holds lines group_name<TAB>sketch_name,
//       the sketches are found by name across the input databases, the groups
//       come in order of first appearance and name the output's sketches; the
//       result equals a database indexed from each group's sequences together
//   sks-search tally <out.sks> <groups.tsv> <min> <max> <in.sks> [<in.sks> ...]
//       one sketch per group of groups.tsv (read and named as merge does), the
//       k-mers held by <min> .. <max> of the sketches the group lists
//       (sks_sketch_set_tally).  <min> and <max> are each a count (3), a fraction
//       of the group's listed sketches written with a decimal point (0.9, 1.0:
//       ceil(f m) as a minimum, at least 1, floor(f m) as a maximum), or - for no
//       limit.  The 90 % core of every group:   tally out.sks groups.tsv 0.9 - ...
//       the strict core: 1.0 -;  the k-mers of exactly one sketch: 1 1;  - - is merge
//   sks-search subtract <db.sks> <filter.sks> <out.sks>
//   sks-search intersect <db.sks> <filter.sks> <out.sks>
//       every sketch of the database without (subtract) or within (intersect)
//       the union of all sketches of filter.sks (sks_sketch_set_merge, one group
//       of all, then sks_sketch_set_filter): host or contaminant k-mers out of
//       every sample, or the part of every sample inside a pangenome.  Both
//       databases must share window, mask, scale and hash; names kept
//   sks-search cluster <db.sks> <min_containment> <out.tsv> [<reps.sks>]
//       single-linkage clusters of the database (sks_cluster_set, min_shared 1):
//       two sketches are linked when the larger of their two containments is at
//       least min_containment.  One line per sketch, in database order:
//         cluster<TAB>representative name<TAB>sketch name
//       (clusters numbered by their first member; a cluster's representative is
//       its largest sketch; names fall back to the index).  With reps.sks the
//       representatives are written as a database, in cluster order, each with
//       its elements, windows and name (dereplication)
//   sks-search gather <db.sks> <min_shared> <out.csv> <q.fa> ...
//       each FASTA file is one query (a mixture), sketched with the database's
//       window, mask and policy; the greedy min-set cover of it by the database
//       (sks_gather_sets): per round the reference explaining the most still
//       unexplained query k-mers, at least min_shared of them:
//         Query,Round,Reference,Shared,SharedNew,RefSize,FQueryNew,ANI   (doubles as %.17g)
//       and after each query's rows one line  Query,-,unexplained,<n_unexplained>,,,,
//   sks-search top <db.sks> <k> <out.csv> <q.fa> ...
//       each FASTA file is one query, sketched with the database's window, mask
//       and policy; its k best references (k <= 64), best first, by containment
//       of the shared k-mers in the query (sks_search_topk_sets, SKS_RANK_QUERY;
//       ties to the larger Shared, then to the earlier reference); a query with
//       fewer than k references sharing a k-mer has fewer rows:
//         Query,Rank,Reference,Shared,Score,ANI     (doubles as %.17g)
#include <hip/hip_runtime.h>

#include <algorithm>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "sks.h"
#include "tally_plan.hpp"

namespace {

void check(int rc) {
  if (rc != SKS_OK) throw std::runtime_error(std::string(sks_last_error()) + " (status " + std::to_string(rc) + ")");
}

void check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// One sketch per file: the files' record streams back to back in device memory,
// a segment per file, one build; the file names become the sketch names.
// With `limits` = {min, max} the build also counts (sks_sketch_build_counted).
sks_sketch_set* sketch_files(sks_ctx* ctx, int n, char* files[], int window, const uint64_t mask[2],
                             const sks_policy& policy, const uint32_t* limits = nullptr) {
  std::vector<uint8_t> stream;
  std::vector<uint64_t> seg_off{0};
  for (int i = 0; i < n; ++i) {
    sks_fasta* f = nullptr;
    check(sks_fasta_open(files[i], &f));
    const uint64_t bytes = sks_fasta_stream_bytes(f);
    if (bytes) stream.insert(stream.end(), sks_fasta_stream(f), sks_fasta_stream(f) + bytes);
    sks_fasta_close(f);
    seg_off.push_back(stream.size());
  }
  void* d_seq = nullptr;
  check_hip(hipMalloc(&d_seq, stream.size() ? stream.size() : 1), "hipMalloc");
  if (!stream.empty()) check_hip(hipMemcpy(d_seq, stream.data(), stream.size(), hipMemcpyHostToDevice), "hipMemcpy");
  sks_sketch_set* set = nullptr;
  const int rc = limits ? sks_sketch_build_counted(ctx, static_cast<const uint8_t*>(d_seq), stream.size(),
                                                   seg_off.data(), (uint32_t)n, window, mask, &policy, limits[0],
                                                   limits[1], &set)
                        : sks_sketch_build(ctx, static_cast<const uint8_t*>(d_seq), stream.size(), seg_off.data(),
                                           (uint32_t)n, window, mask, &policy, &set);
  if (rc == SKS_OK) (void)sks_ctx_synchronize(ctx);
  (void)hipFree(d_seq);
  check(rc);
  std::vector<const char*> names(files, files + n);
  check(sks_sketch_set_set_names(set, names.data()));
  return set;
}

// merge and tally: the input databases and the groups of groups.tsv (lines
// group_name<TAB>sketch_name; the sketches are found by name across the inputs,
// numbered as the library numbers the sources; groups in order of first appearance).
struct NamedGroups {
  std::vector<sks_sketch_set*> dbs;
  std::vector<std::string> names;
  std::vector<uint32_t> group_off{0}, members;
};

NamedGroups read_groups(sks_ctx* ctx, const char* tsv_path, int n_dbs, char* db_paths[]) {
  NamedGroups G;
  std::map<std::string, uint32_t> index_of;
  uint32_t n_src = 0;
  for (int i = 0; i < n_dbs; ++i) {
    sks_sketch_set* db = nullptr;
    check(sks_sketch_set_load(ctx, db_paths[i], &db));
    G.dbs.push_back(db);
    const uint32_t n = sks_sketch_set_num(db);
    for (uint32_t k = 0; k < n; ++k) {
      const char* name = sks_sketch_set_name(db, k);
      if (!name) throw std::runtime_error(std::string(db_paths[i]) + " has no sketch names");
      if (!index_of.emplace(name, n_src + k).second)
        throw std::runtime_error(std::string("sketch name found twice in the inputs: ") + name);
    }
    n_src += n;
  }
  std::ifstream tsv(tsv_path);
  if (!tsv) throw std::runtime_error(std::string("cannot read ") + tsv_path);
  std::map<std::string, size_t> group_of;
  std::vector<std::vector<uint32_t>> listed;
  std::string line;
  while (std::getline(tsv, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    const size_t tab = line.find('\t');
    if (tab == std::string::npos) throw std::runtime_error("groups line without a tab: " + line);
    const std::string group = line.substr(0, tab), sketch = line.substr(tab + 1);
    const auto src = index_of.find(sketch);
    if (src == index_of.end()) throw std::runtime_error("sketch name not found in the inputs: " + sketch);
    const auto g = group_of.emplace(group, G.names.size());
    if (g.second) {
      G.names.push_back(group);
      listed.emplace_back();
    }
    listed[g.first->second].push_back(src->second);
  }
  for (const auto& l : listed) {
    G.members.insert(G.members.end(), l.begin(), l.end());
    G.group_off.push_back((uint32_t)G.members.size());
  }
  return G;
}

// Names the grouped result after its groups, saves it, and frees it and the inputs.
void save_grouped(sks_ctx* ctx, sks_sketch_set* result, const NamedGroups& G, const char* path) {
  check(sks_ctx_synchronize(ctx));
  std::vector<const char*> names;
  for (const std::string& g : G.names) names.push_back(g.c_str());
  check(sks_sketch_set_set_names(result, names.data()));
  check(sks_sketch_set_save(result, path));
  std::printf("%u sketches -> %s\n", sks_sketch_set_num(result), path);
  sks_sketch_set_free(result);
  for (sks_sketch_set* db : G.dbs) sks_sketch_set_free(db);
}

int usage(const char* argv0) {
  std::fprintf(stderr,
               "usage: %s index <out.sks> <w> <k> <c> <fasta files...>\n"
               "       %s index-abund <out.sks> <w> <k> <c> <min> <max|-> <fasta files...>\n"
               "       %s weigh <sample.sks> <db.sks> <min_containment> <out.csv>\n"
               "       %s query <db.sks> <min_containment> <out.csv> <fasta files...>\n"
               "       %s downsample <in.sks> <c> <out.sks>\n"
               "       %s merge <out.sks> <groups.tsv> <in.sks> [<in.sks> ...]\n"
               "       %s tally <out.sks> <groups.tsv> <min> <max> <in.sks> [<in.sks> ...]\n"
               "           (<min>, <max>: a count, a fraction of the group's members written with a\n"
               "            decimal point, or - for no limit; the 90%% core: tally out groups 0.9 - ...)\n"
               "       %s subtract <db.sks> <filter.sks> <out.sks>\n"
               "       %s intersect <db.sks> <filter.sks> <out.sks>\n"
               "       %s cluster <db.sks> <min_containment> <out.tsv> [<reps.sks>]\n"
               "       %s gather <db.sks> <min_shared> <out.csv> <fasta files...>\n"
               "       %s top <db.sks> <k> <out.csv> <fasta files...>\n",
               argv0, argv0, argv0, argv0, argv0, argv0, argv0, argv0, argv0, argv0, argv0, argv0);
  return 64;
}

int run(int argc, char* argv[]) {
  const std::string mode = argc > 1 ? argv[1] : "";
  sks_ctx* ctx = nullptr;
  if (mode == "index" && argc >= 7) {
    const int w = std::atoi(argv[3]), k = std::atoi(argv[4]);
    const uint64_t c = std::strtoull(argv[5], nullptr, 10);
    uint64_t mask[2];
    check(sks_mask_generate(w, k, 0, mask));
    check(sks_ctx_create(0, nullptr, &ctx));
    const sks_policy policy{SKS_FRAC_MOD, SKS_HASH_BOOST_MIX, c, 1};
    sks_sketch_set* set = sketch_files(ctx, argc - 6, argv + 6, w, mask, policy);
    check(sks_sketch_set_save(set, argv[2]));
    std::printf("%u sketches -> %s\n", sks_sketch_set_num(set), argv[2]);
    sks_sketch_set_free(set);
    sks_ctx_destroy(ctx);
    return 0;
  }
  if (mode == "index-abund" && argc >= 9) {
    const int w = std::atoi(argv[3]), k = std::atoi(argv[4]);
    const uint64_t c = std::strtoull(argv[5], nullptr, 10);
    uint32_t limits[2] = {1, UINT32_MAX};
    for (int i = 0; i < 2; ++i) {
      const char* text = argv[6 + i];
      if (i == 1 && std::strcmp(text, "-") == 0) continue;
      char* end = nullptr;
      const unsigned long long v = std::strtoull(text, &end, 10);
      if (end == text || *end || text[0] == '-' || v > UINT32_MAX)
        throw std::runtime_error(std::string(i ? "bad <max>: " : "bad <min>: ") + text);
      limits[i] = (uint32_t)v;
    }
    uint64_t mask[2];
    check(sks_mask_generate(w, k, 0, mask));
    check(sks_ctx_create(0, nullptr, &ctx));
    const sks_policy policy{SKS_FRAC_MOD, SKS_HASH_BOOST_MIX, c, 1};
    sks_sketch_set* set = sketch_files(ctx, argc - 8, argv + 8, w, mask, policy, limits);
    check(sks_sketch_set_save(set, argv[2]));
    std::printf("%u sketches -> %s\n", sks_sketch_set_num(set), argv[2]);
    sks_sketch_set_free(set);
    sks_ctx_destroy(ctx);
    return 0;
  }
  if (mode == "weigh" && argc == 6) {
    char* end = nullptr;
    const double min_containment = std::strtod(argv[4], &end);
    if (end == argv[4] || *end) throw std::runtime_error(std::string("bad min_containment: ") + argv[4]);
    check(sks_ctx_create(0, nullptr, &ctx));
    sks_sketch_set *sample = nullptr, *db = nullptr;
    check(sks_sketch_set_load(ctx, argv[2], &sample));
    check(sks_sketch_set_load(ctx, argv[3], &db));
    // refused here, with the library's message, for a sample without abundances
    check(sks_abund_pairs(ctx, sample, db, nullptr, nullptr, 0, nullptr, nullptr));
    std::vector<uint64_t> totals(sks_sketch_set_num(sample));
    check(sks_sketch_set_abund_totals(sample, totals.data()));
    uint64_t n = 0;
    check(sks_search_sets(ctx, sample, db, min_containment, 1, nullptr, 0, &n));
    std::vector<sks_hit> hits(n);
    std::vector<int32_t> shared(n);
    std::vector<uint64_t> weight(n);
    if (n) {
      void *d_hits = nullptr, *d_idx = nullptr, *d_shared = nullptr, *d_weight = nullptr;
      check_hip(hipMalloc(&d_hits, n * sizeof(sks_hit)), "hipMalloc");
      check_hip(hipMalloc(&d_idx, 2 * n * sizeof(int32_t)), "hipMalloc");
      check_hip(hipMalloc(&d_shared, n * sizeof(int32_t)), "hipMalloc");
      check_hip(hipMalloc(&d_weight, n * sizeof(uint64_t)), "hipMalloc");
      int rc = sks_search_sets(ctx, sample, db, min_containment, 1, static_cast<sks_hit*>(d_hits), n, &n);
      if (rc == SKS_OK) rc = sks_ctx_synchronize(ctx);
      if (rc == SKS_OK) {
        check_hip(hipMemcpy(hits.data(), d_hits, n * sizeof(sks_hit), hipMemcpyDeviceToHost), "hipMemcpy");
        std::vector<int32_t> idx(2 * n);
        for (uint64_t i = 0; i < n; ++i) {
          idx[i] = (int32_t)hits[i].query;
          idx[n + i] = (int32_t)hits[i].ref;
        }
        check_hip(hipMemcpy(d_idx, idx.data(), 2 * n * sizeof(int32_t), hipMemcpyHostToDevice), "hipMemcpy");
        rc = sks_abund_pairs(ctx, sample, db, static_cast<const int32_t*>(d_idx),
                             static_cast<const int32_t*>(d_idx) + n, n, static_cast<int32_t*>(d_shared),
                             static_cast<uint64_t*>(d_weight));
        if (rc == SKS_OK) rc = sks_ctx_synchronize(ctx);
        if (rc == SKS_OK) {
          check_hip(hipMemcpy(shared.data(), d_shared, n * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy");
          check_hip(hipMemcpy(weight.data(), d_weight, n * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy");
        }
      }
      for (void* p : {d_hits, d_idx, d_shared, d_weight}) (void)hipFree(p);
      check(rc);
    }
    FILE* out = std::fopen(argv[5], "w");
    if (!out) throw std::runtime_error(std::string("cannot write ") + argv[5]);
    std::fprintf(out, "Query,Reference,Shared,Containment,ANI,Weight,MeanDepth,FWeighted\n");
    for (uint64_t i = 0; i < n; ++i) {
      const sks_hit& h = hits[i];
      if (shared[i] != h.shared) throw std::runtime_error("the weighted overlap and the search disagree on a pair");
      const char *qn = sks_sketch_set_name(sample, h.query), *rn = sks_sketch_set_name(db, h.ref);
      const std::string q_name = qn ? qn : std::to_string(h.query), r_name = rn ? rn : std::to_string(h.ref);
      std::fprintf(out, "%s,%s,%d,%.17g,%.17g,%llu,%.17g,%.17g\n", q_name.c_str(), r_name.c_str(), h.shared,
                   h.containment, h.ani, (unsigned long long)weight[i], (double)weight[i] / (double)h.shared,
                   (double)weight[i] / (double)totals[h.query]);
    }
    std::fclose(out);
    std::printf("%llu hits -> %s\n", (unsigned long long)n, argv[5]);
    sks_sketch_set_free(sample);
    sks_sketch_set_free(db);
    sks_ctx_destroy(ctx);
    return 0;
  }
  if (mode == "query" && argc >= 6) {
    char* end = nullptr;
    const double min_containment = std::strtod(argv[3], &end);
    if (end == argv[3] || *end) throw std::runtime_error(std::string("bad min_containment: ") + argv[3]);
    check(sks_ctx_create(0, nullptr, &ctx));
    sks_sketch_set* db = nullptr;
    check(sks_sketch_set_load(ctx, argv[2], &db));
    sks_sketch_info info{};
    check(sks_sketch_set_info(db, &info));
    sks_sketch_set* q = sketch_files(ctx, argc - 5, argv + 5, info.window, info.mask, info.policy);
    uint64_t n = 0;
    check(sks_search_sets(ctx, q, db, min_containment, 1, nullptr, 0, &n));
    std::vector<sks_hit> hits(n);
    if (n) {
      void* d_hits = nullptr;
      check_hip(hipMalloc(&d_hits, n * sizeof(sks_hit)), "hipMalloc");
      const int rc = sks_search_sets(ctx, q, db, min_containment, 1, static_cast<sks_hit*>(d_hits), n, &n);
      if (rc == SKS_OK && sks_ctx_synchronize(ctx) == SKS_OK)
        check_hip(hipMemcpy(hits.data(), d_hits, n * sizeof(sks_hit), hipMemcpyDeviceToHost), "hipMemcpy");
      (void)hipFree(d_hits);
      check(rc);
    }
    FILE* out = std::fopen(argv[4], "w");
    if (!out) throw std::runtime_error(std::string("cannot write ") + argv[4]);
    std::fprintf(out, "Query,Reference,Shared,Containment,ANI\n");
    for (const sks_hit& h : hits) {
      const char* ref = sks_sketch_set_name(db, h.ref);
      const std::string ref_name = ref ? ref : std::to_string(h.ref);
      std::fprintf(out, "%s,%s,%d,%.17g,%.17g\n", argv[5 + h.query], ref_name.c_str(), h.shared, h.containment,
                   h.ani);
    }
    std::fclose(out);
    std::printf("%llu hits -> %s\n", (unsigned long long)n, argv[4]);
    sks_sketch_set_free(q);
    sks_sketch_set_free(db);
    sks_ctx_destroy(ctx);
    return 0;
  }
  if (mode == "downsample" && argc == 5) {
    char* end = nullptr;
    const uint64_t c = std::strtoull(argv[3], &end, 10);
    if (end == argv[3] || *end) throw std::runtime_error(std::string("bad c: ") + argv[3]);
    check(sks_ctx_create(0, nullptr, &ctx));
    sks_sketch_set* db = nullptr;
    check(sks_sketch_set_load(ctx, argv[2], &db));
    sks_sketch_set* small = nullptr;
    check(sks_sketch_set_downsample(ctx, db, c, &small));
    check(sks_ctx_synchronize(ctx));
    check(sks_sketch_set_save(small, argv[4]));
    std::printf("%u sketches -> %s\n", sks_sketch_set_num(small), argv[4]);
    sks_sketch_set_free(small);
    sks_sketch_set_free(db);
    sks_ctx_destroy(ctx);
    return 0;
  }
  if (mode == "merge" && argc >= 5) {
    check(sks_ctx_create(0, nullptr, &ctx));
    const NamedGroups G = read_groups(ctx, argv[3], argc - 4, argv + 4);
    sks_sketch_set* merged = nullptr;
    check(sks_sketch_set_merge(ctx, G.dbs.data(), (uint32_t)G.dbs.size(), G.group_off.data(), G.members.data(),
                               (uint32_t)G.names.size(), &merged));
    save_grouped(ctx, merged, G, argv[2]);
    sks_ctx_destroy(ctx);
    return 0;
  }
  if (mode == "tally" && argc >= 7) {
    sks::TallyThreshold lo, hi;
    if (const char* bad = sks::tally_parse_threshold(argv[4], &lo))
      throw std::runtime_error(std::string("bad <min> '") + argv[4] + "': " + bad);
    if (const char* bad = sks::tally_parse_threshold(argv[5], &hi))
      throw std::runtime_error(std::string("bad <max> '") + argv[5] + "': " + bad);
    check(sks_ctx_create(0, nullptr, &ctx));
    const NamedGroups G = read_groups(ctx, argv[3], argc - 6, argv + 6);
    const uint32_t n_groups = (uint32_t)G.names.size();
    std::vector<uint32_t> min_count(n_groups + 1, 1), max_count(n_groups + 1, UINT32_MAX);
    for (uint32_t g = 0; g < n_groups; ++g) {
      const uint32_t m = G.group_off[g + 1] - G.group_off[g];
      min_count[g] = sks::tally_min_of(lo, m);
      max_count[g] = sks::tally_max_of(hi, m);
    }
    sks_sketch_set* kept = nullptr;
    check(sks_sketch_set_tally(ctx, G.dbs.data(), (uint32_t)G.dbs.size(), G.group_off.data(), G.members.data(),
                               n_groups, min_count.data(), max_count.data(), &kept, nullptr, 0));
    save_grouped(ctx, kept, G, argv[2]);
    sks_ctx_destroy(ctx);
    return 0;
  }
  if ((mode == "subtract" || mode == "intersect") && argc == 5) {
    check(sks_ctx_create(0, nullptr, &ctx));
    sks_sketch_set *db = nullptr, *filter = nullptr, *united = nullptr, *kept = nullptr;
    check(sks_sketch_set_load(ctx, argv[2], &db));
    check(sks_sketch_set_load(ctx, argv[3], &filter));
    // the filter database as one sketch: one group of all its sketches
    const uint32_t n_filter = sks_sketch_set_num(filter);
    std::vector<uint32_t> members(n_filter);
    for (uint32_t i = 0; i < n_filter; ++i) members[i] = i;
    const uint32_t group_off[2] = {0, n_filter};
    check(sks_sketch_set_merge(ctx, &filter, 1, group_off, members.data(), 1, &united));
    check(sks_sketch_set_filter(ctx, db, united, nullptr,
                                mode == "subtract" ? SKS_FILTER_SUBTRACT : SKS_FILTER_INTERSECT, &kept));
    check(sks_ctx_synchronize(ctx));
    check(sks_sketch_set_save(kept, argv[4]));
    const uint32_t n = sks_sketch_set_num(kept);
    std::vector<uint32_t> sizes(n);
    if (n) check(sks_sketch_set_sizes(kept, sizes.data()));
    unsigned long long elements = 0;
    for (uint32_t v : sizes) elements += v;
    std::printf("%u sketches, %llu elements -> %s\n", n, elements, argv[4]);
    sks_sketch_set_free(kept);
    sks_sketch_set_free(united);
    sks_sketch_set_free(filter);
    sks_sketch_set_free(db);
    sks_ctx_destroy(ctx);
    return 0;
  }
  if (mode == "cluster" && (argc == 5 || argc == 6)) {
    char* end = nullptr;
    const double min_containment = std::strtod(argv[3], &end);
    if (end == argv[3] || *end) throw std::runtime_error(std::string("bad min_containment: ") + argv[3]);
    check(sks_ctx_create(0, nullptr, &ctx));
    sks_sketch_set* db = nullptr;
    check(sks_sketch_set_load(ctx, argv[2], &db));
    const uint32_t n = sks_sketch_set_num(db);
    std::vector<uint32_t> label(n), rep(n);
    uint32_t n_clusters = 0;
    if (n) {
      void* d_out = nullptr;  // labels, then representatives
      check_hip(hipMalloc(&d_out, (size_t)n * 2 * sizeof(uint32_t)), "hipMalloc");
      uint32_t* d_label = static_cast<uint32_t*>(d_out);
      const int rc = sks_cluster_set(ctx, db, min_containment, 1, d_label, d_label + n, &n_clusters);
      if (rc == SKS_OK && sks_ctx_synchronize(ctx) == SKS_OK) {
        check_hip(hipMemcpy(label.data(), d_label, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy");
        check_hip(hipMemcpy(rep.data(), d_label + n, (size_t)n_clusters * sizeof(uint32_t), hipMemcpyDeviceToHost),
                  "hipMemcpy");
      }
      (void)hipFree(d_out);
      check(rc);
    }
    rep.resize(n_clusters);
    const auto name_of = [db](uint32_t i) {
      const char* name = sks_sketch_set_name(db, i);
      return name ? std::string(name) : std::to_string(i);
    };
    FILE* out = std::fopen(argv[4], "w");
    if (!out) throw std::runtime_error(std::string("cannot write ") + argv[4]);
    for (uint32_t i = 0; i < n; ++i)
      std::fprintf(out, "%u\t%s\t%s\n", label[i], name_of(rep[label[i]]).c_str(), name_of(i).c_str());
    std::fclose(out);
    if (argc == 6) {
      // the representatives as a database: one single-member group each
      std::vector<uint32_t> group_off(n_clusters + 1);
      for (uint32_t g = 0; g <= n_clusters; ++g) group_off[g] = g;
      sks_sketch_set* reps = nullptr;
      check(sks_sketch_set_merge(ctx, &db, 1, group_off.data(), rep.data(), n_clusters, &reps));
      check(sks_ctx_synchronize(ctx));
      std::vector<std::string> rep_names;
      for (uint32_t r : rep) rep_names.push_back(name_of(r));
      std::vector<const char*> names;
      for (const std::string& r : rep_names) names.push_back(r.c_str());
      if (n_clusters) check(sks_sketch_set_set_names(reps, names.data()));
      check(sks_sketch_set_save(reps, argv[5]));
      sks_sketch_set_free(reps);
    }
    std::printf("%u sketches, %u clusters -> %s\n", n, n_clusters, argv[4]);
    sks_sketch_set_free(db);
    sks_ctx_destroy(ctx);
    return 0;
  }
  if (mode == "gather" && argc >= 6) {
    char* end = nullptr;
    const long min_shared = std::strtol(argv[3], &end, 10);
    if (end == argv[3] || *end) throw std::runtime_error(std::string("bad min_shared: ") + argv[3]);
    check(sks_ctx_create(0, nullptr, &ctx));
    sks_sketch_set* db = nullptr;
    check(sks_sketch_set_load(ctx, argv[2], &db));
    sks_sketch_info info{};
    check(sks_sketch_set_info(db, &info));
    const int nq = argc - 5;
    sks_sketch_set* q = sketch_files(ctx, nq, argv + 5, info.window, info.mask, info.policy);
    std::vector<uint32_t> q_sizes(nq);
    check(sks_sketch_set_sizes(q, q_sizes.data()));
    FILE* out = std::fopen(argv[4], "w");
    if (!out) throw std::runtime_error(std::string("cannot write ") + argv[4]);
    std::fprintf(out, "Query,Round,Reference,Shared,SharedNew,RefSize,FQueryNew,ANI\n");
    unsigned long long total = 0;
    for (int i = 0; i < nq; ++i) {
      // min(references, query elements) records always suffice
      const uint64_t cap = std::min<uint64_t>(sks_sketch_set_num(db), q_sizes[i]);
      std::vector<sks_gather_hit> hits(cap);
      uint64_t n = 0;
      uint32_t unexplained = 0;
      void* d_hits = nullptr;
      check_hip(hipMalloc(&d_hits, (cap ? cap : 1) * sizeof(sks_gather_hit)), "hipMalloc");
      const int rc = sks_gather_sets(ctx, q, (uint32_t)i, db, (int32_t)min_shared, 0,
                                     static_cast<sks_gather_hit*>(d_hits), cap, &n, &unexplained);
      if (rc == SKS_OK && n && sks_ctx_synchronize(ctx) == SKS_OK)
        check_hip(hipMemcpy(hits.data(), d_hits, n * sizeof(sks_gather_hit), hipMemcpyDeviceToHost), "hipMemcpy");
      (void)hipFree(d_hits);
      check(rc);
      for (uint64_t r = 0; r < n; ++r) {
        const sks_gather_hit& h = hits[r];
        const char* ref = sks_sketch_set_name(db, h.ref);
        const std::string ref_name = ref ? ref : std::to_string(h.ref);
        std::fprintf(out, "%s,%llu,%s,%d,%d,%d,%.17g,%.17g\n", argv[5 + i], (unsigned long long)r, ref_name.c_str(),
                     h.shared, h.shared_new, h.ref_size, h.f_query_new, h.ani);
      }
      std::fprintf(out, "%s,-,unexplained,%u,,,,\n", argv[5 + i], unexplained);
      total += n;
    }
    std::fclose(out);
    std::printf("%llu hits -> %s\n", total, argv[4]);
    sks_sketch_set_free(q);
    sks_sketch_set_free(db);
    sks_ctx_destroy(ctx);
    return 0;
  }
  if (mode == "top" && argc >= 6) {
    char* end = nullptr;
    const unsigned long k = std::strtoul(argv[3], &end, 10);
    if (end == argv[3] || *end || k == 0 || k > SKS_TOPK_MAX)
      throw std::runtime_error(std::string("bad k (1 .. ") + std::to_string(SKS_TOPK_MAX) + "): " + argv[3]);
    check(sks_ctx_create(0, nullptr, &ctx));
    sks_sketch_set* db = nullptr;
    check(sks_sketch_set_load(ctx, argv[2], &db));
    sks_sketch_info info{};
    check(sks_sketch_set_info(db, &info));
    const int nq = argc - 5;
    sks_sketch_set* q = sketch_files(ctx, nq, argv + 5, info.window, info.mask, info.policy);
    std::vector<sks_top_hit> hits((size_t)nq * k);
    void* d_hits = nullptr;
    check_hip(hipMalloc(&d_hits, hits.size() * sizeof(sks_top_hit)), "hipMalloc");
    const int rc = sks_search_topk_sets(ctx, q, db, SKS_RANK_QUERY, (uint32_t)k, 0.0, 1, 0,
                                        static_cast<sks_top_hit*>(d_hits), nullptr);
    if (rc == SKS_OK && sks_ctx_synchronize(ctx) == SKS_OK)
      check_hip(hipMemcpy(hits.data(), d_hits, hits.size() * sizeof(sks_top_hit), hipMemcpyDeviceToHost), "hipMemcpy");
    (void)hipFree(d_hits);
    check(rc);
    FILE* out = std::fopen(argv[4], "w");
    if (!out) throw std::runtime_error(std::string("cannot write ") + argv[4]);
    std::fprintf(out, "Query,Rank,Reference,Shared,Score,ANI\n");
    unsigned long long total = 0;
    for (const sks_top_hit& h : hits) {
      if (h.ref == UINT32_MAX) continue;  // an empty slot
      const char* ref = sks_sketch_set_name(db, h.ref);
      const std::string ref_name = ref ? ref : std::to_string(h.ref);
      std::fprintf(out, "%s,%u,%s,%d,%.17g,%.17g\n", argv[5 + h.query], h.rank, ref_name.c_str(), h.shared, h.score,
                   h.ani);
      ++total;
    }
    std::fclose(out);
    std::printf("%llu hits -> %s\n", total, argv[4]);
    sks_sketch_set_free(q);
    sks_sketch_set_free(db);
    sks_ctx_destroy(ctx);
    return 0;
  }
  return usage(argv[0]);
}

}  // namespace

int main(int argc, char* argv[]) {
  try {
    return run(argc, argv);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sks-search: %s\n", e.what());
    return 1;
  }
}
