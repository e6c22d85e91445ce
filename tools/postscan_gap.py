"""Where the in-flight config-3 step's time beyond the scan goes, from one
rocprofv3 --kernel-trace --hip-trace run of the plain `python bench.py`.

    python tools/postscan_gap.py <kernel_trace.csv> <hip_api_trace.csv> [--serial-scan-ms 4.14]

The timed in-flight builds are the ones launched by the worker threads (every
warm-up build is launched by the main thread).  Printed: the scan launches in
start order (begin, end, duration, idle time since the scans before), per build
what runs between its scan's end and the return of sks_sketch_build (taken as
the end of the thread's last hipStreamSynchronize before its next scan launch),
and the split of `step - serial scan` into (1) scans longer than the serial
scan, less the time counted twice where scans run side by side, (2) idle gaps between scans, (3) run
edges: first launch to first scan start, and last scan end to the last return."""
import argparse
import collections
import csv


def short(name):
    k = name.replace("(anonymous namespace)::", "").replace("sks::", "")
    return k.split("(")[0].split("<")[0][-48:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kernels")
    ap.add_argument("api")
    ap.add_argument("--serial-scan-ms", type=float, default=4.14)
    a = ap.parse_args()
    ker = [dict(r, s=int(r["Start_Timestamp"]), e=int(r["End_Timestamp"]), tid=r["Thread_Id"])
           for r in csv.DictReader(open(a.kernels))]
    ker.sort(key=lambda r: r["s"])
    api = [dict(r, s=int(r["Start_Timestamp"]), e=int(r["End_Timestamp"]), tid=r["Thread_Id"])
           for r in csv.DictReader(open(a.api)) if r["Domain"].startswith("HIP_RUNTIME_API")]
    api.sort(key=lambda r: r["s"])
    launch_of = {r["Correlation_Id"]: r for r in api if r["Function"].startswith("hipLaunchKernel")}
    main_tid = ker[0]["tid"]
    scans = [k for k in ker if "scan_kernel" in k["Kernel_Name"] and k["tid"] != main_tid]
    if not scans:
        print("no in-flight scan launches found")
        return
    workers = sorted({k["tid"] for k in scans})
    t_begin = min(r["s"] for r in api if r["tid"] in workers)
    us = lambda t: (t - t_begin) / 1e3

    print(f"{len(scans)} timed in-flight builds on {len(workers)} threads; times in us from the workers' first HIP call")
    print("scan launches: thread begin end duration idle_before")
    covered = scans[0]["s"]
    gaps = overlap = 0
    for k in scans:
        idle = k["s"] - covered
        if idle > 0:
            gaps += idle
        else:
            overlap += min(-idle, k["e"] - k["s"])
        covered = max(covered, k["e"])
        print(f"  t{workers.index(k['tid'])} {us(k['s']):10.1f} {us(k['e']):10.1f} {(k['e'] - k['s']) / 1e3:8.1f} {idle / 1e3:8.1f}")

    print("per build, between its scan's end and the return of sks_sketch_build:")
    print("  thread kernels kernel_us wall_us memcpyAsync memsetAsync streamSync malloc | calls after the scan's launch")
    tot = collections.Counter()
    names = collections.Counter()
    t_end = 0
    for w in workers:
        mine = [k for k in scans if k["tid"] == w]
        calls = [r for r in api if r["tid"] == w]
        for i, k in enumerate(mine):
            launch = launch_of.get(k["Correlation_Id"])
            after = launch["e"] if launch else k["s"]
            nxt = launch_of.get(mine[i + 1]["Correlation_Id"]) if i + 1 < len(mine) else None
            before = nxt["s"] if nxt else float("inf")
            syncs = [r for r in calls if r["Function"] == "hipStreamSynchronize" and after <= r["s"] < before]
            ret = syncs[-1]["e"] if syncs else k["e"]
            t_end = max(t_end, ret)
            span = [r for r in calls if after <= r["s"] < ret]
            n = collections.Counter(r["Function"] for r in span)
            post = [q for q in ker if q["tid"] == w and k["e"] <= q["s"] < ret]
            kus = sum(q["e"] - q["s"] for q in post) / 1e3
            for q in post:
                names[short(q["Kernel_Name"])] += 1
            row = (len(post), kus, (ret - k["e"]) / 1e3, n["hipMemcpyAsync"], n["hipMemsetAsync"],
                   n["hipStreamSynchronize"], n["hipMalloc"])
            for j, v in enumerate(row):
                tot[j] += v
            print(f"  t{workers.index(w)} {row[0]:3d} {row[1]:8.1f} {row[2]:8.1f} {row[3]:3d} {row[4]:3d} {row[5]:3d} {row[6]:3d}")
    nb = len(scans)
    print("mean per build: kernels %.1f, kernel time %.1f us, scan end to return %.1f us, hipMemcpyAsync %.1f, "
          "hipMemsetAsync %.1f, hipStreamSynchronize %.1f, hipMalloc %.1f" % tuple(tot[j] / nb for j in range(7)))
    print("kernels in those spans (launches over all builds): " +
          ", ".join(f"{k} x{v}" for k, v in sorted(names.items(), key=lambda kv: -kv[1])))

    step = (t_end - t_begin) / nb / 1e6
    durs = sum(k["e"] - k["s"] for k in scans) / nb / 1e6
    serial = a.serial_scan_ms
    edges = ((scans[0]["s"] - t_begin) + (t_end - covered)) / nb / 1e6
    print(f"step (first worker call to last return) / {nb} = {step:.4f} ms; serial scan {serial:.4f} ms; "
          f"difference {step - serial:.4f} ms, of which")
    print(f"  (1) scans longer than the serial scan: {durs - serial:+.4f} ms (mean in-flight scan {durs:.4f} ms), "
          f"less {overlap / nb / 1e6:.4f} ms counted twice where scans run side by side")
    print(f"  (2) idle gaps between scans: {gaps / nb / 1e6:.4f} ms")
    print(f"  (3) run edges: {edges:.4f} ms (first scan starts {(scans[0]['s'] - t_begin) / 1e3:.1f} us after the "
          f"first call, last return {(t_end - covered) / 1e3:.1f} us after the last scan's end)")


if __name__ == "__main__":
    main()
