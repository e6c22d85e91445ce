"""Downsampling a resident sketch set against re-sketching the sequences, for
the same result: n genomes of `length` bases (default 1000 x 5 Mb),
narrow w=31 / k=21, FracMinHash 1/200 -> 1/1000.

  downsample: Context.downsample(S200, 1000) over the resident set
  rebuild:    Context.sketch_build(..., param=1000) of the resident sequences
              (what a caller had to do before sks_sketch_set_downsample)

The two alternate, one warm-up pair first; each call is timed with events on
the context's stream (the null stream) and with the host clock around the call
and a device synchronise.  The two results are compared element for element
once.  Prints one JSON line: median, minimum and maximum of both, in ms.
    python tools/bench_downsample.py [n_genomes] [length] [reps] [c] [c_coarse]"""
import json
import os
import statistics
import sys
import time

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
    n, length, reps, c, cc = arg(1, 1000), arg(2, 5_000_000), arg(3, 7), arg(4, 200), arg(5, 1000)
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

    down = lambda: ctx.downsample(src, cc)  # noqa: E731
    build = lambda: ctx.sketch_build(buf.data_ptr(), seg[-1], seg, w, mask, sksffi.SKS_FRAC_MOD, cc)  # noqa: E731
    d_ev, d_wall, b_ev, b_wall = [], [], [], []
    for r in range(reps + 1):
        ev, wall, got = timed(down)
        ev2, wall2, want = timed(build)
        if r == 0:  # the warm-up pair: also the comparison
            assert (got.sizes() == want.sizes()).all(), "downsample and rebuild disagree on sizes"
            assert torch.equal(got.device_tensors()[0], want.device_tensors()[0]), "downsample and rebuild disagree"
        else:
            d_ev.append(ev), d_wall.append(wall), b_ev.append(ev2), b_wall.append(wall2)
        elems_out = int(got.sizes().astype("int64").sum())
        got.free()
        want.free()
    elems_in = int(src.sizes().astype("int64").sum())
    print(json.dumps({"genomes": n, "length": length, "c": c, "c_coarse": cc, "reps": reps,
                      "elements_in": elems_in, "elements_out": elems_out,
                      "downsample_event_ms": stats(d_ev), "downsample_wall_ms": stats(d_wall),
                      "rebuild_event_ms": stats(b_ev), "rebuild_wall_ms": stats(b_wall)}))


if __name__ == "__main__":
    main()
