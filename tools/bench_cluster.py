"""Single-linkage clusters of a resident sketch set against the two ways to the
same answer before sks_cluster_set: n genomes of `length` bases (default
1000 x 5 Mb), narrow w=31 / k=21, FracMinHash 1/200.

Two inputs:
  families:  genome g belongs to family g // 8, whose first member is the
             ancestor and whose others descend from it at substitution rates
             0.5% .. 3.5%, so clusters exist at the threshold (default 0.5)
  identical: n copies of one sketch: one cluster, n^2 hits (the worst case of
             the hit list)

Per input, timed in alternation after one warm-up round in which the labels
are compared:
  cluster:  Context.cluster_set_raw into resident label / representative buffers
  search:   sks_search_sets(set, set) at the same thresholds the way a caller
            must run it: the size query, the call into a buffer of that size,
            the copy of the hits to the host and a host union-find (numpy
            minimum propagation over the hit list; its share is reported apart);
            and, as search_size_query, the first of those calls alone
  ani:      sks_all_pairs_ani (counts + ANI matrix on the device) on the same set

Each is timed with events on the context's stream (the null stream) and with
the host clock around the call and a device synchronise.  Prints one JSON line
(median, minimum and maximum in ms) and writes it to
profiles/cluster/bench_cluster.json.
    python tools/bench_cluster.py [n_genomes] [length] [reps] [c] [min_containment]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spaced-kmer-sketching_amd"))
import sksffi  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def host_components(n, q, r):
    """Canonical labels of the graph with edges (q[i], r[i]): the smallest member
    of each component by repeated minimum propagation, numbered in index order."""
    low = np.arange(n, dtype=np.int64)
    while True:
        nxt = low.copy()
        np.minimum.at(nxt, q, low[r])
        np.minimum.at(nxt, r, low[q])
        nxt = nxt[nxt]  # pointer jumping
        if np.array_equal(nxt, low):
            break
        low = nxt
    roots, labels = np.unique(low, return_inverse=True)
    return labels.astype(np.uint32), len(roots)


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
    n, length, reps, c = arg(1, 1000), arg(2, 5_000_000), arg(3, 20), arg(4, 200)
    thr = float(sys.argv[5]) if len(sys.argv) > 5 else 0.5
    ctx = sksffi.Context(0)
    w, k = 31, 21
    mask = sksffi.mask_generate(w, k, 0)
    seg = [0]
    for _ in range(n):
        seg.append(seg[-1] + length + 1)
    buf = torch.full((seg[-1],), ord("\n"), dtype=torch.uint8, device="cuda")
    for g in range(n):
        fam, member = divmod(g, 8)
        ctx.synth_bases(buf.data_ptr() + seg[g], length, 4000 + fam, 9000 + g, 0.005 * member)
    torch.cuda.synchronize()
    families = ctx.sketch_build(buf.data_ptr(), seg[-1], seg, w, mask, sksffi.SKS_FRAC_MOD, c)
    ctx.synchronize()
    del buf
    torch.cuda.empty_cache()
    first = ctx.merge([families], [[0]])
    identical = ctx.merge([first], [[0]] * n)
    ctx.synchronize()

    labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    rep = torch.zeros(n, dtype=torch.int32, device="cuda")
    ani = torch.zeros(n * n, dtype=torch.float64, device="cuda")
    result = {"genomes": n, "length": length, "c": c, "reps": reps, "min_containment": thr, "min_shared": 1,
              "inputs": []}
    for name, S in (("families", families), ("identical", identical)):
        sizes = S.sizes().astype(np.int64)
        data, starts, d_sizes = S.device_ptrs()

        def cluster():
            rc, count = ctx.cluster_set_raw(S, thr, 1, labels.data_ptr(), rep.data_ptr())
            sksffi.check(rc)
            return count

        def search():
            hits = ctx.search(S, S, min_containment=thr, min_shared=1)  # size query, fill, D2H
            t0 = time.perf_counter()
            got = host_components(n, hits["query"].astype(np.int64), hits["ref"].astype(np.int64))
            return got + (len(hits), (time.perf_counter() - t0) * 1e3)

        def search_once():  # the size query alone: one sks_search_sets call, no hit buffer, no sort
            return ctx.search_sets_raw(S, S, thr, 1, 0, 0)

        def all_pairs():
            ctx.all_pairs_ani(data, starts, d_sizes, n, int(sizes.max()), int(sizes.sum()), k, ani.data_ptr(), 0, 0)

        t = {x: ([], []) for x in ("cluster", "search", "search_size_query", "ani")}
        cluster_call_ms, host_ms = [], []
        for r in range(reps + 1):
            ev_c, wall_c, count = timed(cluster)
            call_ms = ctx.last_intersect_ms()
            ev_s, wall_s, (want, want_count, n_hits, uf_ms) = timed(search)
            ev_q, wall_q, _ = timed(search_once)
            ev_a, wall_a, _ = timed(all_pairs)
            if r == 0:  # the warm-up round: also the comparison
                assert count == want_count, (count, want_count)
                assert np.array_equal(labels.cpu().numpy().view(np.uint32), want), "cluster and search disagree"
            else:
                cluster_call_ms.append(call_ms)
                host_ms.append(uf_ms)
                for x, ev, wall in (("cluster", ev_c, wall_c), ("search", ev_s, wall_s),
                                    ("search_size_query", ev_q, wall_q), ("ani", ev_a, wall_a)):
                    t[x][0].append(ev), t[x][1].append(wall)
        row = {"input": name, "elements": int(sizes.sum()), "clusters": count, "hits": n_hits,
               "cluster_last_intersect_ms": stats(cluster_call_ms),
               "search_host_union_find_ms": stats(host_ms)}
        for x, (ev, wall) in t.items():
            row[f"{x}_event_ms"], row[f"{x}_wall_ms"] = stats(ev), stats(wall)
        result["inputs"].append(row)
    line = json.dumps(result)
    print(line)
    out = os.path.join(ROOT, "profiles", "cluster")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "bench_cluster.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
