"""Grouped tallies of a resident sketch set against sks_sketch_set_merge on the
same groups (the yardstick: the same merge rounds with the cheaper last pass)
and against the host route: n genomes of `length` bases (default 1000 x 5 Mb),
narrow w=31 / k=21, FracMinHash 1/200, in groups of consecutive sketches
(default: groups of 8, of 2, and one group of all).

  union:  Context.tally, min_count 1, no maximum (merge's result)
  core:   min_count ceil(0.9 m), no maximum
  cloud:  min_count 1, max_count 1
  *_counts: the same three with d_counts (a resident device buffer)
  merge:  Context.merge([S], groups)
  host:   every sketch to the host, then np.unique(return_counts=True) per group
          (timed with the host clock only, `host_reps` times)

The genomes are independent random sequences, so nearly every k-mer is held by
one member: core is almost empty and cloud almost everything, the two ends of
what the last pass can be asked to write.  Per grouping the device calls
alternate, one warm-up round first in which union is compared with merge
element for element and core, cloud and the multiplicities with the host route;
each call is timed with events on the context's stream (the null stream) and
with the host clock around the call and a device synchronise.  Prints one JSON
line: median, minimum and maximum in ms, and tally / merge ratios of the medians.
    python tools/bench_tally.py [n_genomes] [length] [reps] [c] [group sizes, comma separated; 0: all] [host_reps]"""
import ctypes as C
import json
import math
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
    host_reps = arg(6, 2)
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
    del buf
    sizes = src.sizes().astype(np.int64)
    starts = src.starts().astype(np.int64)
    total = int(sizes.sum())
    d_counts = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")  # the members' sizes always suffice
    lib = sksffi.lib()

    result = {"genomes": n, "length": length, "c": c, "reps": reps, "host_reps": host_reps, "elements_in": total,
              "groupings": []}
    for gs in group_sizes:
        gs = gs or n
        groups = [list(range(b, min(b + gs, n))) for b in range(0, n, gs)]
        off = np.zeros(len(groups) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(g) for g in groups])
        mem = np.arange(n, dtype=np.uint32)
        ones = np.ones(len(groups) + 1, dtype=np.uint32)
        core_lo = np.array([max(1, math.ceil(0.9 * len(g) - 1e-9)) for g in groups] + [1], dtype=np.uint32)
        arr = (C.c_void_p * 1)(src.h)

        def tally(lo, hi, with_counts):
            h = C.c_void_p()
            sksffi.check(lib.sks_sketch_set_tally(ctx.h, arr, 1, off.ctypes.data, mem.ctypes.data, len(groups),
                                                  lo.ctypes.data, None if hi is None else hi.ctypes.data, C.byref(h),
                                                  C.c_void_p(d_counts.data_ptr()) if with_counts else None,
                                                  total if with_counts else 0))
            return sksffi.SketchSet(h)

        def host_route():
            data = src.device_tensors()[0].cpu().numpy().view(np.uint64)
            out = []
            for g in groups:  # consecutive sketches lie back to back in the set's data
                b, e = int(starts[g[0]]), int(starts[g[-1]] + sizes[g[-1]])
                out.append(np.unique(data[b:e], return_counts=True))
            return out

        calls = {"merge": lambda: ctx.merge([src], groups)}
        for name, lo, hi in (("union", ones, None), ("core", core_lo, None), ("cloud", ones, ones)):
            calls[name] = lambda lo=lo, hi=hi: tally(lo, hi, False)
            calls[name + "_counts"] = lambda lo=lo, hi=hi: tally(lo, hi, True)
        t = {name: ([], []) for name in calls}
        elems = {}
        for r in range(reps + 1):
            if r == 0:  # the warm-up round: also the comparison
                ref = host_route()
            for name, fn in calls.items():
                ev, wall, got = timed(fn)
                if r == 0:
                    data = got.device_tensors()[0].cpu().numpy().view(np.uint64)
                    elems[name] = int(got.sizes().astype(np.int64).sum())
                    kind = name.split("_")[0]
                    keep = [(cnt >= (1 if kind != "core" else core_lo[i])) & ((cnt <= 1) | (kind != "cloud"))
                            for i, (_, cnt) in enumerate(ref)]
                    want = np.concatenate([u[m] for (u, _), m in zip(ref, keep)])
                    assert np.array_equal(data[:elems[name]], want), f"{name} and the host route disagree"
                    if name.endswith("_counts"):
                        mult = np.concatenate([cnt[m] for (_, cnt), m in zip(ref, keep)])
                        got_mult = d_counts[:elems[name]].cpu().numpy().view(np.uint32)
                        assert np.array_equal(got_mult, mult), f"{name}: multiplicities disagree with the host route"
                else:
                    t[name][0].append(ev), t[name][1].append(wall)
                got.free()
        host = []
        for _ in range(host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_route()
            host.append((time.perf_counter() - t0) * 1e3)
        row = {"group_size": gs, "groups": len(groups), "elements_out": elems}
        for name, (ev, wall) in t.items():
            row[f"{name}_event_ms"], row[f"{name}_wall_ms"] = stats(ev), stats(wall)
        row["host_wall_ms"] = stats(host)
        m = row["merge_event_ms"]["median"]
        row["tally_over_merge_event"] = {name: round(row[f"{name}_event_ms"]["median"] / m, 3)
                                         for name in calls if name != "merge"}
        result["groupings"].append(row)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
