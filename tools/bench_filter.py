"""sks_sketch_set_filter on resident sets: n genomes of `length` bases (default
1000 x 5 Mb, config 4's shape), FracMinHash 1/200, narrow w=31 / k=21 and wide
w=45 / k=30, both kinds, two maps:

  a: filter_of[i] = (i + 1) % n over the set itself: a chunk brackets about one
     chunk of filter elements (the staged path); once more under
     SKS_FILTER_NO_STAGE=1 (every chunk on the direct path)
  b: one shared filter, the merge of 64 of the sketches: a chunk brackets far
     more than the stage holds (the direct path)

next to Context.downsample(set, 200) of the same set (the same passes without
any search: the floor of this call's shape) and to the only route there was
before, as far as it goes: elements to the host and np.isin per sketch (arrays,
not a set), timed on the first `host_sketches` sketches and scaled to n.

The calls alternate, one warm-up round first, which also compares the results
element for element (staged against direct on the device, and against numpy on
the first sketches); each call is timed with events on the context's stream
(the null stream) and with the host clock around the call and a device
synchronise.  Prints one JSON line: median, minimum and maximum in ms.
    python tools/bench_filter.py [n_genomes] [length] [reps] [shapes] [maps] [label]
shapes: narrow, wide or narrow,wide; maps: a, b or a,b; label: copied into the
line (e.g. the stage size of an A/B build loaded through SKS_LIB)."""
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

SHAPES = {"narrow": (31, 21), "wide": (45, 30)}
KINDS = {"subtract": sksffi.SKS_FILTER_SUBTRACT, "intersect": sksffi.SKS_FILTER_INTERSECT}
ROW = np.dtype([("hi", "<u8"), ("lo", "<u8")])


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


def rows(sketch):
    out = np.empty(len(sketch), dtype=ROW)
    out["hi"], out["lo"] = sketch[:, 1], sketch[:, 0]
    return out


def found_in(a, b, wide):
    if not len(a) or not len(b):
        return np.zeros(len(a), dtype=bool)
    return np.isin(rows(a), rows(b)) if wide else np.isin(a[:, 0], b[:, 0])


def no_stage(fn):
    def call():
        os.environ["SKS_FILTER_NO_STAGE"] = "1"
        try:
            return fn()
        finally:
            del os.environ["SKS_FILTER_NO_STAGE"]
    return call


def same_sets(x, y):
    return (x.sizes() == y.sizes()).all() and torch.equal(x.device_tensors()[0], y.device_tensors()[0])


def run_shape(ctx, shape, n, length, reps, maps, host_sketches):
    w, k = SHAPES[shape]
    wide = shape == "wide"
    mask = sksffi.mask_generate(w, k, 0)
    seg = [0]
    for _ in range(n):
        seg.append(seg[-1] + length + 1)
    buf = torch.full((seg[-1],), ord("\n"), dtype=torch.uint8, device="cuda")
    for g in range(n):
        ctx.synth_bases(buf.data_ptr() + seg[g], length, 4000 + g)
    torch.cuda.synchronize()
    src = ctx.sketch_build(buf.data_ptr(), seg[-1], seg, w, mask, sksffi.SKS_FRAC_MOD, 200)
    ctx.synchronize()
    print(f"{shape}: {n} sketches built", file=sys.stderr, flush=True)
    del buf
    torch.cuda.empty_cache()

    next_of = [(i + 1) % n for i in range(n)]
    shared = ctx.merge([src], [list(range(min(64, n)))])
    ctx.synchronize()
    calls, filters = {}, {}
    for kind, kv in KINDS.items():
        if "a" in maps:
            calls[f"a_{kind}"] = lambda kv=kv: ctx.filter(src, src, kv, next_of)
            calls[f"a_{kind}_no_stage"] = no_stage(calls[f"a_{kind}"])
            filters[f"a_{kind}"] = (src, next_of, kv)
        if "b" in maps:
            calls[f"b_{kind}"] = lambda kv=kv: ctx.filter(src, shared, kv)
            filters[f"b_{kind}"] = (shared, [0] * n, kv)
    calls["downsample_same_c"] = lambda: ctx.downsample(src, 200)

    ev, wall, kept = {c: [] for c in calls}, {c: [] for c in calls}, {}
    for r in range(reps + 1):
        warm = {}
        for name, fn in calls.items():
            e, t, got = timed(fn)
            if r == 0:  # the warm-up round: also the comparison
                warm[name] = got
                kept[name] = int(got.sizes().astype("int64").sum())
            else:
                ev[name].append(e), wall[name].append(t)
                got.free()
        print(f"{shape}: round {r} of {reps}", file=sys.stderr, flush=True)
        if r == 0:
            assert same_sets(warm["downsample_same_c"], src), "downsample at the same c is not a copy"
            for name, (filt, fo, kv) in filters.items():
                if name + "_no_stage" in warm:
                    assert same_sets(warm[name], warm[name + "_no_stage"]), f"{name}: staged and direct disagree"
                for i in range(min(n, 4)):
                    s = src.sketch(i)
                    want = s[found_in(s, filt.sketch(fo[i]), wide) != (kv == sksffi.SKS_FILTER_SUBTRACT)]
                    assert np.array_equal(warm[name].sketch(i), want), f"{name}: sketch {i} differs from numpy"
            for got in warm.values():
                got.free()

    # the route before this call: elements to the host, np.isin per sketch
    host = {}
    m = min(n, host_sketches)
    for tag, filt, fo in [("a", src, next_of), ("b", shared, [0] * n)]:
        if tag not in maps:
            continue
        t0 = time.perf_counter()
        for i in range(m if tag == "a" else min(m, 8)):
            found_in(src.sketch(i), filt.sketch(fo[i]), wide)
        done = m if tag == "a" else min(m, 8)
        host[f"{tag}_host_isin"] = {"sketches_timed": done,
                                    "ms_per_sketch": round((time.perf_counter() - t0) * 1e3 / done, 3),
                                    "ms_scaled_to_n": round((time.perf_counter() - t0) * 1e3 / done * n, 1)}
    out = {"w": w, "k": k, "elements_in": int(src.sizes().astype("int64").sum()),
           "filter_b_elements": int(shared.sizes()[0]), "elements_out": kept,
           "event_ms": {c: stats(v) for c, v in ev.items()}, "wall_ms": {c: stats(v) for c, v in wall.items()},
           "host_route": host}
    shared.free()
    src.free()
    return out


def main():
    arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d  # noqa: E731
    n, length, reps = int(arg(1, 1000)), int(arg(2, 5_000_000)), int(arg(3, 7))
    shapes, maps, label = arg(4, "narrow,wide").split(","), arg(5, "a,b").split(","), arg(6, "")
    ctx = sksffi.Context(0)
    line = {"genomes": n, "length": length, "c": 200, "reps": reps, "label": label, "lib": sksffi.build_info()}
    for shape in shapes:
        line[shape] = run_shape(ctx, shape, n, length, reps, maps, 100)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
