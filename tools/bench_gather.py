"""Greedy min-set cover of a mixture (sks_gather_sets) against the only route to
the same answer before it, a host loop around the search: n resident reference
genomes of `length` bases (default 1000 x 5 Mb), narrow w=31 / k=21,
FracMinHash 1/200.  Genome g belongs to family g // 8, whose first member is the
ancestor and whose others descend from it at substitution rates 0.5% .. 3.5%.

Two queries:
  mixture: one segment holding 50 of the references, one from each of the
           families 0 .. 49 (the ancestor of the even families, the 1.5%
           descendant of the odd ones, whose ancestors are references too), and
           10 Mb that matches nothing
  single:  one 5 Mb genome (a 1.5% descendant), about length / 200 elements

Per query, timed in alternation after one warm-up round in which the hit lists
are compared for equality:
  gather:      Context.gather_sets_raw into a resident hit buffer, at the
               default rounds per wait and at each value of the sweep
  membership:  the same call with a min_shared nothing reaches: the membership
               pass and its one wait, no round (rounds = gather - membership)
  host_loop:   per round sks_search of the remaining query against the
               references (size query, then the call), hits to the host, argmax
               (ties to the smallest index), numpy set-difference with the
               winner's sketch (the sketches' host copies are made outside the
               timing), the remaining query uploaded.  The remaining query goes
               in through the array form, the library having no call that wraps
               caller arrays as a set; total and per-round cost are reported
  search_once: one sks_search_sets(query, references) size query: the floor any
               answer pays

Each is timed with events on the context's stream (the null stream) and with
the host clock around the call and a device synchronise.  Prints one JSON line
(median, minimum and maximum in ms) and writes it to
profiles/gather/bench_gather.json.
    python tools/bench_gather.py [n_genomes] [length] [reps] [c] [min_shared] [rounds_per_wait,...]"""
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

DEFAULT_ROUNDS = 64  # kGatherDefaultRounds (csrc/gather_plan.hpp)


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


def genome(g):
    """(ancestor seed, mutation seed, rate) of reference g."""
    fam, member = divmod(g, 8)
    return 4000 + fam, 9000 + g, 0.005 * member


def sketch(ctx, pieces, w, mask, c):
    """One sketch of the pieces (length, seed, mutation seed, rate) laid out in one segment."""
    total = sum(p[0] + 1 for p in pieces)
    buf = torch.full((total,), ord("\n"), dtype=torch.uint8, device="cuda")
    at = 0
    for length, seed, mseed, rate in pieces:
        ctx.synth_bases(buf.data_ptr() + at, length, seed, mseed, rate)
        at += length + 1
    torch.cuda.synchronize()
    s = ctx.sketch_build(buf.data_ptr(), total, [0, total], w, mask, sksffi.SKS_FRAC_MOD, c)
    ctx.synchronize()
    return s


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
    n, length, reps, c, thr = arg(1, 1000), arg(2, 5_000_000), arg(3, 10), arg(4, 200), arg(5, 3)
    sweep = [int(x) for x in sys.argv[6].split(",")] if len(sys.argv) > 6 else [1, 2, 4, 8, 16, 32, 64]
    ctx = sksffi.Context(0)
    w, k = 31, 21
    mask = sksffi.mask_generate(w, k, 0)
    seg = [0]
    for _ in range(n):
        seg.append(seg[-1] + length + 1)
    buf = torch.full((seg[-1],), ord("\n"), dtype=torch.uint8, device="cuda")
    for g in range(n):
        ctx.synth_bases(buf.data_ptr() + seg[g], length, *genome(g))
    torch.cuda.synchronize()
    R = ctx.sketch_build(buf.data_ptr(), seg[-1], seg, w, mask, sksffi.SKS_FRAC_MOD, c)
    ctx.synchronize()
    del buf
    torch.cuda.empty_cache()
    families = min(50, n // 8)
    members = [8 * f + (3 if f % 2 else 0) for f in range(families)]
    queries = {
        "mixture": [(length,) + genome(g) for g in members] + [(2 * length, 777, 0, 0.0)],
        "single": [(length,) + genome(8 * (n // 8 - 1) + 3)],
    }
    r_sizes = R.sizes().astype(np.int64)
    r_host = [np.ascontiguousarray(R.sketch(i)[:, 0]) for i in range(n)]  # outside every timing
    r_side = R.device_ptrs() + (n, int(r_sizes.max()), int(r_sizes.sum()))
    hits_buf = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    result = {"genomes": n, "length": length, "c": c, "reps": reps, "min_shared": thr,
              "reference_elements": int(r_sizes.sum()), "default_rounds_per_wait": DEFAULT_ROUNDS, "inputs": []}
    for name, pieces in queries.items():
        Q = sketch(ctx, pieces, w, mask, c)
        q_host = np.ascontiguousarray(Q.sketch(0)[:, 0])

        def gather():
            rc, cnt, un = ctx.gather_sets_raw(Q, 0, R, thr, 0, hits_buf.data_ptr(), n)
            sksffi.check(rc)
            return cnt, un

        def membership():
            rc, cnt, un = ctx.gather_sets_raw(Q, 0, R, 0x7fffffff, 0, hits_buf.data_ptr(), n)
            sksffi.check(rc)
            assert cnt == 0
            return cnt

        def host_loop():
            rem, out, search_ms = q_host, [], 0.0
            while len(rem):
                d = torch.from_numpy(rem.view(np.int64)).cuda()
                st = torch.zeros(1, dtype=torch.int64, device="cuda")
                sz = torch.tensor([len(rem)], dtype=torch.int32, device="cuda")
                t0 = time.perf_counter()
                h = ctx.search_arrays((d.data_ptr(), st.data_ptr(), sz.data_ptr(), 1, len(rem), len(rem)), r_side, 1, k,
                                      min_containment=0.0, min_shared=thr)
                search_ms += (time.perf_counter() - t0) * 1e3
                if not len(h):
                    break
                best = int(np.argmax(h["shared"]))  # (query 0, ref) order: the first maximum is the smallest index
                ref = int(h["ref"][best])
                out.append((ref, int(h["shared"][best])))
                rem = np.setdiff1d(rem, r_host[ref], assume_unique=True)
            return out, len(rem), search_ms

        def search_once():
            return ctx.search_sets_raw(Q, R, 0.0, thr, 0, 0)

        names = ["gather", "membership", "host_loop", "search_once"] + [f"gather_rounds_{g}" for g in sweep]
        t = {x: ([], []) for x in names}
        call_ms, loop_search_ms = [], []
        for r in range(reps + 1):
            ev_g, wall_g, (count, unexplained) = timed(gather)
            last_ms = ctx.last_intersect_ms()
            ev_m, wall_m, _ = timed(membership)
            ev_h, wall_h, (want, want_un, s_ms) = timed(host_loop)
            ev_s, wall_s, _ = timed(search_once)
            swept = []
            for g in sweep:
                ctx.set_gather_rounds(g)
                try:
                    swept.append(timed(gather))
                finally:
                    ctx.set_gather_rounds(0)
            if r == 0:  # the warm-up round: also the comparison
                got = hits_buf.cpu().numpy().view(sksffi.GATHER_HIT_DTYPE)[:count]
                assert [(int(h["ref"]), int(h["shared_new"])) for h in got] == want, "gather and the host loop disagree"
                assert unexplained == want_un
                for _, _, (cnt, un) in swept:
                    assert (cnt, un) == (count, unexplained)
            else:
                call_ms.append(last_ms)
                loop_search_ms.append(s_ms)
                rows = [("gather", ev_g, wall_g), ("membership", ev_m, wall_m), ("host_loop", ev_h, wall_h),
                        ("search_once", ev_s, wall_s)]
                rows += [(f"gather_rounds_{g}", ev, wall) for g, (ev, wall, _) in zip(sweep, swept)]
                for x, ev, wall in rows:
                    t[x][0].append(ev), t[x][1].append(wall)
        rounds = count + 1  # the last round finds nothing left
        row = {"input": name, "query_elements": int(len(q_host)), "hits": count, "unexplained": unexplained,
               "rounds": rounds, "round_groups_waited_for": -(-rounds // DEFAULT_ROUNDS),
               "gather_last_intersect_ms": stats(call_ms), "host_loop_search_calls_ms": stats(loop_search_ms)}
        for x, (ev, wall) in t.items():
            row[f"{x}_event_ms"], row[f"{x}_wall_ms"] = stats(ev), stats(wall)
        row["rounds_wall_ms"] = round(row["gather_wall_ms"]["median"] - row["membership_wall_ms"]["median"], 3)
        row["host_loop_per_round_wall_ms"] = round(row["host_loop_wall_ms"]["median"] / max(len(want) + 1, 1), 3)
        # the membership pass against the bytes the algorithm needs: every reference
        # element read once, the query once (8 bytes an element at elem_words 1)
        bytes_needed = (int(r_sizes.sum()) + len(q_host)) * 8
        row["membership_algorithmic_bytes"] = bytes_needed
        row["membership_call_gb_per_s"] = round(bytes_needed / (row["membership_event_ms"]["median"] * 1e-3) / 1e9, 2)
        result["inputs"].append(row)
    line = json.dumps(result)
    print(line)
    out = os.path.join(ROOT, "profiles", "gather")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "bench_gather.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
