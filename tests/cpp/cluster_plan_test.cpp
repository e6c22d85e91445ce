// CPU check of csrc/cluster_plan.hpp (no HIP, no libsks): the lock-free union
// by index against a breadth-first search, over every graph on up to 6 vertices
// with the edges in several orders and on random graphs whose edges four
// threads share; the link rule at its corners; and the triangle tiles, each in
// exactly one batch range for every block count and batch size.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <numeric>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "cluster_plan.hpp"

using namespace sks;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

namespace {

// the host's memory operations: relaxed atomics on the plain words
struct HostOps {
  uint32_t load(const uint32_t* p) const { return __atomic_load_n(p, __ATOMIC_RELAXED); }
  uint32_t cas(uint32_t* p, uint32_t expected, uint32_t desired) const {
    __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expected;  // the value found (== the caller's `expected` on success)
  }
};

using Edges = std::vector<std::pair<uint32_t, uint32_t>>;

// the smallest member of each vertex's component, by breadth-first search
std::vector<uint32_t> bfs_roots(uint32_t n, const Edges& edges) {
  std::vector<std::vector<uint32_t>> adj(n);
  for (const auto& e : edges) {
    adj[e.first].push_back(e.second);
    adj[e.second].push_back(e.first);
  }
  std::vector<uint32_t> root(n, UINT32_MAX);
  for (uint32_t s = 0; s < n; ++s) {
    if (root[s] != UINT32_MAX) continue;
    std::vector<uint32_t> todo{s};
    root[s] = s;  // s is the smallest vertex not reached before
    while (!todo.empty()) {
      const uint32_t v = todo.back();
      todo.pop_back();
      for (uint32_t u : adj[v])
        if (root[u] == UINT32_MAX) {
          root[u] = s;
          todo.push_back(u);
        }
    }
  }
  return root;
}

void check_parent(const std::vector<uint32_t>& parent, const std::vector<uint32_t>& want) {
  const HostOps ops;
  std::vector<uint32_t> p = parent;
  for (uint32_t i = 0; i < p.size(); ++i) {
    CHECK(p[i] <= i);  // a parent is never larger than its child
    CHECK(cluster_find(ops, p.data(), i) == want[i]);  // the root is the smallest member
  }
}

void unite_all(std::vector<uint32_t>& parent, const Edges& edges, size_t begin, size_t step) {
  const HostOps ops;
  for (size_t e = begin; e < edges.size(); e += step) cluster_unite(ops, parent.data(), edges[e].first, edges[e].second);
}

void test_small_graphs() {
  std::mt19937 rng(7);
  for (uint32_t n = 1; n <= 6; ++n) {
    Edges all;
    for (uint32_t a = 0; a < n; ++a)
      for (uint32_t b = a + 1; b < n; ++b) all.push_back({a, b});
    for (uint32_t m = 0; m < (1u << all.size()); ++m) {
      Edges edges;
      for (size_t e = 0; e < all.size(); ++e)
        if ((m >> e) & 1) edges.push_back((e & 1) ? all[e] : std::make_pair(all[e].second, all[e].first));
      const std::vector<uint32_t> want = bfs_roots(n, edges);
      for (int order = 0; order < 4; ++order) {
        if (order == 1) std::reverse(edges.begin(), edges.end());
        if (order >= 2) std::shuffle(edges.begin(), edges.end(), rng);
        std::vector<uint32_t> parent(n);
        std::iota(parent.begin(), parent.end(), 0u);
        unite_all(parent, edges, 0, 1);
        check_parent(parent, want);
        unite_all(parent, edges, 0, 1);  // a second pass finds every pair united: no change
        check_parent(parent, want);
      }
    }
  }
}

void test_threads() {
  std::mt19937 rng(11);
  for (int round = 0; round < 40; ++round) {
    const uint32_t n = 200 + (uint32_t)(rng() % 300);
    // sparse to dense: many components down to one; self loops and repeats included
    const size_t m = (size_t)n * (1 + round % 8) / 4;
    Edges edges;
    for (size_t e = 0; e < m; ++e) edges.push_back({(uint32_t)(rng() % n), (uint32_t)(rng() % n)});
    const std::vector<uint32_t> want = bfs_roots(n, edges);
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    std::vector<std::thread> th;
    for (size_t t = 0; t < 4; ++t) th.emplace_back(unite_all, std::ref(parent), std::cref(edges), t, 4);
    for (auto& t : th) t.join();
    check_parent(parent, want);
  }
}

void test_link_rule() {
  // nothing shared: never linked, whatever the thresholds
  CHECK(!cluster_linked(0, 10, 10, 0.0, 1));
  CHECK(!cluster_linked(0, 10, 10, -1.0, -5));
  CHECK(!cluster_linked(0, 0, 10, -1.0, 0));  // an empty sketch shares nothing
  CHECK(!cluster_linked(0, 0, 0, 0.0, 1));
  // min_shared below 1 counts as 1
  CHECK(cluster_linked(1, 10, 10, 0.0, 0));
  CHECK(cluster_linked(1, 10, 10, 0.0, -5));
  CHECK(cluster_linked(1, 10, 10, -1.0, 1));
  CHECK(cluster_linked(3, 10, 10, 0.0, 3));
  CHECK(!cluster_linked(2, 10, 10, 0.0, 3));
  // the larger of the two containments decides, in either argument order
  CHECK(cluster_linked(5, 10, 100, 0.5, 1));   // 5 / 10 reaches 0.5 exactly
  CHECK(cluster_linked(5, 100, 10, 0.5, 1));
  CHECK(!cluster_linked(5, 11, 100, 0.5, 1));
  CHECK(!cluster_linked(5, 100, 11, 0.5, 1));
  // a threshold equal to an attainable ratio links; the next double above it does not
  const double third = (double)1 / (double)3;
  CHECK(cluster_containment(7, 21) == third);
  CHECK(cluster_linked(7, 21, 50, third, 1));
  CHECK(!cluster_linked(7, 21, 50, std::nextafter(third, 1.0), 1));
  CHECK(cluster_linked(21, 21, 50, 1.0, 1));
  CHECK(!cluster_linked(21, 21, 50, 2.0, 1));  // no pair meets a threshold above 1
  CHECK(cluster_containment(0, 0) == 0.0);
}

void test_tiles() {
  for (uint32_t nb = 1; nb <= 9; ++nb) {
    const std::vector<uint32_t> list = cluster_tile_list(nb);
    const uint64_t all = cluster_tiles_before(nb);
    CHECK(list.size() == all * 2);
    // every (I, J), I <= J, exactly once, at the position the closed form names
    std::vector<int> seen((size_t)nb * nb, 0);
    for (uint64_t t = 0; t < all; ++t) {
      const uint32_t I = list[2 * t], J = list[2 * t + 1];
      CHECK(I <= J && J < nb);
      CHECK(cluster_tiles_before(J) + I == t);
      ++seen[(size_t)I * nb + J];
    }
    for (uint32_t I = 0; I < nb; ++I)
      for (uint32_t J = 0; J < nb; ++J) CHECK(seen[(size_t)I * nb + J] == (I <= J ? 1 : 0));
    for (uint32_t bb = 1; bb <= nb; ++bb) {
      const uint32_t batches = cluster_batches(nb, bb);
      CHECK(batches == (nb + bb - 1) / bb);
      // the ranges tile [0, all) in order; a tile's column is one of its batch's
      uint64_t at = 0;
      for (uint32_t b = 0; b < batches; ++b) {
        const ClusterRange r = cluster_batch_range(nb, bb, b);
        CHECK(r.begin == at && r.end > r.begin);
        for (uint64_t t = r.begin; t < r.end; ++t) CHECK(list[2 * t + 1] / bb == b);
        at = r.end;
      }
      CHECK(at == all);
    }
  }
}

}  // namespace

int main() {
  test_small_graphs();
  test_threads();
  test_link_rule();
  test_tiles();
  std::printf("cluster plan ok\n");
  return 0;
}
