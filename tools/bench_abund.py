"""Counted builds, the trim and the weighted pairs on a resident sequence set:
n genomes of `length` bases (default 1000 x 5 Mb), FracMinHash 1/200, at
w=31 / k=21 (narrow) and once at w=45 / k=30 (wide).

  build:         Context.sketch_build of the resident sequences (the yardstick)
  build_counted: Context.sketch_build_counted, min 1, no maximum, same process
  build_min2:    the same with min_abund 2 (the trim pass inside the build)
  trim:          Context.abund_trim(counted, 2)
  pairs_*:       sks_abund_pairs over 1000 and 10^6 random pairs, device arrays
                 resident, against sks_intersect_pairs on the same lists
  host:          sks_kmer_list_build, a copy to the host and
                 np.unique(return_counts=True) per genome, once (host clock)

Random genomes hold nearly every k-mer once, so min 2 keeps almost nothing: the
records are about the cost of the passes, not about a typical result.  In the
warm-up round the counted build is compared with the plain one element for
element, the pairs' shared counts with sks_intersect_pairs, and (narrow) the
abundances of the first genomes with the host route.  Each call is timed with
events on the context's stream (the null stream) and with the host clock around
the call and a device synchronise.  Prints one JSON line: median, minimum and
maximum in ms, and counted / plain ratios of the medians.
    python tools/bench_abund.py [n_genomes] [length] [reps] [c] [host_genomes]"""
import ctypes as C
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


def run_shape(ctx, buf, seg, w, k, c, reps, host_genomes):
    n = len(seg) - 1
    mask = sksffi.mask_generate(w, k, 0)
    lib = sksffi.lib()
    build = lambda: ctx.sketch_build(buf.data_ptr(), seg[-1], seg, w, mask, sksffi.SKS_FRAC_MOD, c)  # noqa: E731

    def counted_of(lo):
        return ctx.sketch_build_counted(buf.data_ptr(), seg[-1], seg, w, mask, sksffi.SKS_FRAC_MOD, c, min_abund=lo)

    plain, counted = build(), counted_of(1)
    ctx.synchronize()
    ew = plain.elem_words
    total = int(plain.sizes().astype(np.int64).sum())
    same = torch.equal(plain.device_tensors()[0], counted.device_tensors()[0])
    assert same and np.array_equal(plain.sizes(), counted.sizes()), "the counted build differs from the plain one"
    totals = counted.abund_totals()
    row = {"w": w, "k": k, "elements": total, "abundance_mass": int(totals.sum())}

    rng = np.random.default_rng(11)
    lists = {}
    for m in (1000, 1_000_000):
        a = torch.from_numpy(rng.integers(0, n, m).astype(np.int32)).cuda()
        b = torch.from_numpy(rng.integers(0, n, m).astype(np.int32)).cuda()
        lists[m] = (a, b, torch.zeros(m, dtype=torch.int32, device="cuda"),
                    torch.zeros(m, dtype=torch.int64, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda"))
    data, starts, sizes = counted.device_ptrs()

    def abund_pairs(m):
        a, b, sh, wt, _ = lists[m]
        sksffi.check(lib.sks_abund_pairs(ctx.h, counted.h, counted.h, C.c_void_p(a.data_ptr()),
                                         C.c_void_p(b.data_ptr()), m, C.c_void_p(sh.data_ptr()),
                                         C.c_void_p(wt.data_ptr())))

    def intersect_pairs(m):
        a, b, _, _, out = lists[m]
        ctx.intersect_pairs(data, starts, sizes, ew, a.data_ptr(), b.data_ptr(), m, out.data_ptr())

    calls = {"build": build, "build_counted": lambda: counted_of(1), "build_min2": lambda: counted_of(2),
             "trim": lambda: ctx.abund_trim(counted, 2)}
    for m in lists:
        calls[f"pairs_abund_{m}"] = lambda m=m: abund_pairs(m)
        calls[f"pairs_intersect_{m}"] = lambda m=m: intersect_pairs(m)
    t = {name: ([], []) for name in calls}
    for r in range(reps + 1):
        for name, fn in calls.items():
            ev, wall, got = timed(fn)
            if r == 0 and name in ("build_min2", "trim"):
                row[f"{name}_elements"] = int(got.sizes().astype(np.int64).sum())
            if r:
                t[name][0].append(ev), t[name][1].append(wall)
            if got is not None:
                got.free()
        if r == 0:
            for m, (_, _, sh, _, out) in lists.items():
                assert torch.equal(sh, out), f"{m} pairs: shared differs from sks_intersect_pairs"
    for name, (ev, wall) in t.items():
        row[f"{name}_event_ms"], row[f"{name}_wall_ms"] = stats(ev), stats(wall)
    med = lambda name: row[f"{name}_event_ms"]["median"]  # noqa: E731
    row["counted_over_plain_event"] = round(med("build_counted") / med("build"), 3)
    row["min2_over_plain_event"] = round(med("build_min2") / med("build"), 3)
    for m in lists:
        row[f"pairs_abund_over_intersect_{m}"] = round(med(f"pairs_abund_{m}") / med(f"pairs_intersect_{m}"), 3)

    if host_genomes:
        # the host route over the first host_genomes genomes (all: pass n), checked against the device
        h = min(host_genomes, n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, bits, counts = ctx.kmer_list(buf.data_ptr(), seg[h], seg[:h + 1], w, mask, c)
        at, host = 0, []
        for g in range(h):
            rows = bits[at:at + int(counts[g])]
            host.append(np.unique(rows[:, [3, 2]], axis=0, return_counts=True))
            at += int(counts[g])
        row["host_genomes"] = h
        row["host_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        part = ctx.sketch_build_counted(buf.data_ptr(), seg[h], seg[:h + 1], w, mask, sksffi.SKS_FRAC_MOD, c)
        ctx.synchronize()
        row["device_same_genomes_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        for g in range(min(h, 8)):
            u, cnt = host[g]
            assert np.array_equal(part.sketch(g), u[:, ::-1]), "elements differ from the host route"
            assert np.array_equal(part.abund(g), cnt.astype(np.uint32)), "abundances differ from the host route"
        part.free()
    plain.free()
    counted.free()
    return row


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
    n, length, reps, c, host_genomes = arg(1, 1000), arg(2, 5_000_000), arg(3, 5), arg(4, 200), arg(5, 1000)
    ctx = sksffi.Context(0)
    seg = [0]
    for _ in range(n):
        seg.append(seg[-1] + length + 1)
    buf = torch.full((seg[-1],), ord("\n"), dtype=torch.uint8, device="cuda")
    for g in range(n):
        ctx.synth_bases(buf.data_ptr() + seg[g], length, 4000 + g)
    torch.cuda.synchronize()
    result = {"genomes": n, "length": length, "c": c, "reps": reps, "shapes": []}
    result["shapes"].append(run_shape(ctx, buf, seg, 31, 21, c, reps, host_genomes))
    result["shapes"].append(run_shape(ctx, buf, seg, 45, 30, c, 1, 0))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
