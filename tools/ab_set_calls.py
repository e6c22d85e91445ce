"""A/B of two libsks builds over the set-level calls' benchmarks (bench_search,
bench_topk, bench_cluster, bench_gather, bench_merge, bench_downsample at their
default shapes), for changes to the host code between launches.

Three libraries take turns, one process a run, through SKS_LIB: the parent
build, a byte-for-byte copy of it under another path (the control: what two
runs of the same code differ by) and the new build.  The order rotates every
round (P C N, C N P, N P C), so no build always follows the same neighbour.
Before the benchmarks, sks_join_layout_bounds_for_mask, the host loop every
set-form search, top-k and cluster call runs before its first launch, is timed
alone for each library (log_b 13, the benchmarks' sketch size; no device).

Writes OUT/bench_<tool>.jsonl (every run's JSON line with its build and round)
and OUT/ab_table.txt, one line per metric: the medians of the parent's runs
(parent and copy), of the new build's, the parent's range, and whether every
new run lies inside it or which way it leaves.  Stops at the first run that fails.
    python tools/ab_set_calls.py PARENT_LIB NEW_LIB OUT [rounds=3]"""
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ["search", "topk", "cluster", "gather", "merge", "downsample"]
HOST = """
import ctypes as C, sys, time
sys.path.insert(0, %r)
import sksffi
L = C.CDLL(sys.argv[1])
f = L.sks_join_layout_bounds_for_mask
f.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_int, C.c_void_p]
m = sksffi.mask_generate(31, 21, 0)
mask = (C.c_uint64 * 2)(m & (2**64 - 1), m >> 64)
buf = (C.c_uint64 * 4097)()
ts = []
for _ in range(2000):
    t0 = time.perf_counter_ns(); f(mask, 13, 1, buf); ts.append(time.perf_counter_ns() - t0)
ts.sort()
print('{"mask_bounds_us": {"median": %%.1f, "min": %%.1f}}' %% (ts[1000] / 1e3, ts[0] / 1e3))
""" % os.path.join(ROOT, "spaced-kmer-sketching_amd")


def flat(d, pre=""):
    """Every {"median": ...} block and every bare *_ms number, by its path."""
    r = {}
    if isinstance(d, dict):
        if "median" in d:
            return {pre: d["median"]}
        for k, v in d.items():
            r.update(flat(v, pre + "/" + k if pre else k))
    elif isinstance(d, list):
        for i, v in enumerate(d):
            tag = v.get("input", v.get("group_size", i)) if isinstance(v, dict) else i
            r.update(flat(v, "%s[%s]" % (pre, tag)))
    elif isinstance(d, (int, float)) and pre.endswith("_ms"):
        r[pre] = d
    return r


def main():
    parent, new, out = (os.path.abspath(p) for p in sys.argv[1:4])
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    os.makedirs(out, exist_ok=True)
    copy = os.path.join(out, "libsks_parent_copy.so")
    shutil.copyfile(parent, copy)
    libs = [("parent", parent), ("parent_copy", copy), ("new", new)]
    table = []
    for tool in ["host"] + TOOLS:
        cmd = [sys.executable] + (["-c", HOST] if tool == "host" else [os.path.join(ROOT, "tools", "bench_%s.py" % tool)])
        runs = {name: [] for name, _ in libs}
        with open(os.path.join(out, "bench_%s.jsonl" % tool), "w") as log:
            for r in range(rounds):
                for name, lib in libs[r % 3:] + libs[:r % 3]:
                    p = subprocess.run(cmd + ([lib] if tool == "host" else []), env=dict(os.environ, SKS_LIB=lib),
                                       capture_output=True, text=True, timeout=240, cwd=ROOT)
                    if p.returncode != 0:
                        sys.stderr.write(p.stderr[-2000:])
                        sys.exit("%s with %s failed (%d)" % (tool, name, p.returncode))
                    j = json.loads(p.stdout.strip().splitlines()[-1])
                    log.write(json.dumps({"build": name, "round": r, **j}) + "\n")
                    runs[name].append(flat(j))
        for k in runs["parent"][0]:
            par = [x[k] for x in runs["parent"] + runs["parent_copy"]]
            nw = [x[k] for x in runs["new"]]
            lo, hi = min(par), max(par)
            where = "above" if max(nw) > hi else "below" if min(nw) < lo else "within"
            table.append("%-10s %-58s parent %s  new %s  range %g..%g  %s" %
                         (tool, k, " ".join("%g" % v for v in par), " ".join("%g" % v for v in nw), lo, hi, where))
        print(tool, "done", flush=True)
    os.remove(copy)
    with open(os.path.join(out, "ab_table.txt"), "w") as f:
        f.write("\n".join(table) + "\n")
    print("\n".join(table))


if __name__ == "__main__":
    main()
