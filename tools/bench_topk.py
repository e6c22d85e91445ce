"""The k best references per query (sks_search_topk_sets) against the route to
the same answer before it: a resident set of n genomes of `length` bases
(default 1000 x 5 Mb; genome g belongs to family g // 8, whose first member is
the ancestor and whose others descend from it at substitution rates 0.5% ..
3.5%), narrow w=31 / k=21, FracMinHash 1/200, k = 10, SKS_RANK_QUERY.

Two query sets against those references:
  self:  the same n sketches with skip_same_index (the k-NN graph of the set)
  few:   the first 64 of them

Per query set, timed in alternation after one warm-up round in which the two
results are compared:
  topk:   Context.search_topk_sets_raw into resident hit / count buffers
  route:  sks_search_sets at the lowest thresholds the way a caller must run it:
          the size query, the call into a buffer of that size, the copy of the
          hits to the host and a numpy lexsort per query (its share is reported
          apart); and, as search_size_query, the first of those calls alone

Each is timed with events on the context's stream (the null stream) and with
the host clock around the call and a device synchronise.  Prints one JSON line
(median, minimum and maximum in ms, and the ratios of the medians) and writes
it to profiles/topk/bench_topk.json.
    python tools/bench_topk.py [n_genomes] [length] [reps] [c] [k]"""
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


def host_topk(hits, q_n, k, skip_same_index):
    """refs[q_n, k] (0xffffffff: empty) and shared[q_n, k] from a (query, ref)
    ordered hit list: per query a lexsort by (-containment, -shared, ref)."""
    refs = np.full((q_n, k), 0xffffffff, dtype=np.uint32)
    shared = np.zeros((q_n, k), dtype=np.int32)
    if skip_same_index:
        hits = hits[hits["query"] != hits["ref"]]
    cut = np.searchsorted(hits["query"], np.arange(q_n + 1))
    for q in range(q_n):
        h = hits[cut[q]:cut[q + 1]]
        h = h[np.lexsort((h["ref"], -h["shared"].astype(np.int64), -h["containment"]))][:k]
        refs[q, :len(h)], shared[q, :len(h)] = h["ref"], h["shared"]
    return refs, shared


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
    n, length, reps, c, k = arg(1, 1000), arg(2, 5_000_000), arg(3, 20), arg(4, 200), arg(5, 10)
    ctx = sksffi.Context(0)
    w, kmer = 31, 21
    mask = sksffi.mask_generate(w, kmer, 0)
    seg = [0]
    for _ in range(n):
        seg.append(seg[-1] + length + 1)
    buf = torch.full((seg[-1],), ord("\n"), dtype=torch.uint8, device="cuda")
    for g in range(n):
        fam, member = divmod(g, 8)
        ctx.synth_bases(buf.data_ptr() + seg[g], length, 4000 + fam, 9000 + g, 0.005 * member)
    torch.cuda.synchronize()
    refs = ctx.sketch_build(buf.data_ptr(), seg[-1], seg, w, mask, sksffi.SKS_FRAC_MOD, c)
    ctx.synchronize()
    del buf
    torch.cuda.empty_cache()
    few = ctx.merge([refs], [[i] for i in range(min(64, n))])
    ctx.synchronize()

    result = {"genomes": n, "length": length, "c": c, "reps": reps, "k": k, "rank": "SKS_RANK_QUERY",
              "elements": int(refs.sizes().astype(np.int64).sum()), "inputs": []}
    for name, Q, skip in (("self", refs, True), ("few", few, False)):
        d_hits = torch.zeros(Q.n * k * sksffi.TOP_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_counts = torch.zeros(Q.n, dtype=torch.int32, device="cuda")

        def topk():
            sksffi.check(ctx.search_topk_sets_raw(Q, refs, sksffi.SKS_RANK_QUERY, k, 0.0, 1, skip,
                                                  d_hits.data_ptr(), d_counts.data_ptr()))

        def route():
            hits = ctx.search(Q, refs, min_containment=0.0, min_shared=1)  # size query, fill, D2H
            t0 = time.perf_counter()
            got = host_topk(hits, Q.n, k, skip)
            return got + (len(hits), (time.perf_counter() - t0) * 1e3)

        def search_once():  # the size query alone: one sks_search_sets call, no hit buffer, no sort
            return ctx.search_sets_raw(Q, refs, 0.0, 1, 0, 0)

        t = {x: ([], []) for x in ("topk", "route", "search_size_query")}
        topk_call_ms, host_ms = [], []
        for r in range(reps + 1):
            ev_t, wall_t, _ = timed(topk)
            call_ms = ctx.last_intersect_ms()
            ev_r, wall_r, (want_refs, want_shared, n_hits, sort_ms) = timed(route)
            ev_q, wall_q, _ = timed(search_once)
            if r == 0:  # the warm-up round: also the comparison
                got = d_hits.cpu().numpy().view(sksffi.TOP_HIT_DTYPE).reshape(Q.n, k)
                assert np.array_equal(got["ref"], want_refs), "top-k and the search route disagree"
                assert np.array_equal(got["shared"], want_shared)
                filled = int(d_counts.cpu().numpy().sum())
            else:
                topk_call_ms.append(call_ms)
                host_ms.append(sort_ms)
                for x, ev, wall in (("topk", ev_t, wall_t), ("route", ev_r, wall_r),
                                    ("search_size_query", ev_q, wall_q)):
                    t[x][0].append(ev), t[x][1].append(wall)
        row = {"input": name, "queries": Q.n, "hits": n_hits, "filled_slots": filled,
               "topk_last_intersect_ms": stats(topk_call_ms), "route_host_lexsort_ms": stats(host_ms)}
        for x, (ev, wall) in t.items():
            row[f"{x}_event_ms"], row[f"{x}_wall_ms"] = stats(ev), stats(wall)
        med = lambda x: statistics.median(t[x][1])  # noqa: E731  (wall: the route's host work is part of it)
        row["topk_over_size_query_wall"] = round(med("topk") / med("search_size_query"), 3)
        row["topk_over_route_wall"] = round(med("topk") / med("route"), 3)
        row["topk_over_size_query_event"] = round(statistics.median(t["topk"][0]) /
                                                  statistics.median(t["search_size_query"][0]), 3)
        result["inputs"].append(row)
    line = json.dumps(result)
    print(line)
    out = os.path.join(ROOT, "profiles", "topk")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "bench_topk.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
