"""Grouped unions of a resident sketch set against the two ways to the same
result before sks_sketch_set_merge: n genomes of `length` bases (default
1000 x 5 Mb), narrow w=31 / k=21, FracMinHash 1/200, merged in groups of
consecutive sketches (default: groups of 8, of 2, and one group of all).

  merge:    Context.merge([S], groups) over the resident set
  rebuild:  Context.sketch_build of the resident sequences with the coarser
            seg_off (needs the sequences)
  union:    a host loop of Context.sketch_union (radix sort + unique), one call
            per group over the set's data (the only device union before; each
            call waits for its count)

Per grouping the three alternate, one warm-up round first in which the results
are compared element for element; each call is timed with events on the
context's stream (the null stream) and with the host clock around the call and
a device synchronise.  Prints one JSON line: median, minimum and maximum in ms.
    python tools/bench_merge.py [n_genomes] [length] [reps] [c] [group sizes, comma separated; 0: all]"""
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


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
    n, length, reps, c = arg(1, 1000), arg(2, 5_000_000), arg(3, 7), arg(4, 200)
    group_sizes = [int(x) for x in sys.argv[5].split(",")] if len(sys.argv) > 5 else [8, 2, 0]
    ctx = sksffi.Context(0)
    w, k = 31, 21
    mask = sksffi.mask_generate(w, k, 0)
    seg = [0]
    for _ in range(n):
        seg.append(seg[-1] + length + 1)
    buf = torch.full((seg[-1],), ord("\n"), dtype=torch.uint8, device="cuda")
    for g in range(n):
        ctx.synth_bases(buf.data_ptr() + seg[g], length, 4000 + g)
    torch.cuda.synchronize()
    src = ctx.sketch_build(buf.data_ptr(), seg[-1], seg, w, mask, sksffi.SKS_FRAC_MOD, c)
    ctx.synchronize()
    sizes = src.sizes().astype(np.int64)
    starts = src.starts().astype(np.int64)
    total = int(sizes.sum())
    d_data = src.device_ptrs()[0]
    union_out = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")

    result = {"genomes": n, "length": length, "c": c, "reps": reps, "elements_in": total, "groupings": []}
    for gs in group_sizes:
        gs = gs or n
        groups = [list(range(b, min(b + gs, n))) for b in range(0, n, gs)]
        cuts = [seg[g[0]] for g in groups] + [seg[-1]]

        def union_loop():
            counts, at = [], 0
            for g in groups:  # consecutive sketches lie back to back in the set's data
                m = int(sizes[g[0]:g[-1] + 1].sum())
                counts.append(ctx.sketch_union(d_data + 8 * int(starts[g[0]]), m, union_out.data_ptr() + 8 * at)
                              if m else 0)
                at += m
            return counts

        merge = lambda: ctx.merge([src], groups)  # noqa: E731
        build = lambda: ctx.sketch_build(buf.data_ptr(), seg[-1], cuts, w, mask, sksffi.SKS_FRAC_MOD, c)  # noqa: E731
        t = {name: ([], []) for name in ("merge", "rebuild", "union")}
        for r in range(reps + 1):
            ev_m, wall_m, got = timed(merge)
            ev_b, wall_b, want = timed(build)
            ev_u, wall_u, counts = timed(union_loop)
            if r == 0:  # the warm-up round: also the comparison
                assert (got.sizes() == want.sizes()).all(), "merge and rebuild disagree on sizes"
                assert (got.windows() == want.windows()).all(), "merge and rebuild disagree on windows"
                assert torch.equal(got.device_tensors()[0], want.device_tensors()[0]), "merge and rebuild disagree"
                assert counts == got.sizes().tolist(), "merge and the union loop disagree on sizes"
                data, at, pos = got.device_tensors()[0], 0, 0
                for g, cnt in zip(groups, counts):
                    assert torch.equal(union_out[at:at + cnt], data[pos:pos + cnt]), "merge and the union loop disagree"
                    at += int(sizes[g[0]:g[-1] + 1].sum())
                    pos += cnt
            else:
                for name, ev, wall in (("merge", ev_m, wall_m), ("rebuild", ev_b, wall_b), ("union", ev_u, wall_u)):
                    t[name][0].append(ev), t[name][1].append(wall)
            elems_out = int(got.sizes().astype("int64").sum())
            got.free()
            want.free()
        row = {"group_size": gs, "groups": len(groups), "elements_out": elems_out}
        for name, (ev, wall) in t.items():
            row[f"{name}_event_ms"], row[f"{name}_wall_ms"] = stats(ev), stats(wall)
        result["groupings"].append(row)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
