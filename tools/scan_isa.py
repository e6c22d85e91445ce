"""Static figures of every scan kernel (profiles/r*/scan_isa.txt), read from
the compiler's gfx950 assembly of csrc/scan.hip (the Makefile's flags).

Per kernel: instructions, static VALU, v_mbcnt, returning LDS atomics, global
atomics, v_readlane_b32 (all, and those inside the tile loop: the largest
outermost loop of the kernel), v_min_f64, vector global loads inside the tile
loop, VGPRs, SGPRs, LDS bytes, the compiler's occupancy and scratch bytes.

    python tools/scan_isa.py [scan.hip]      # default: the package's csrc/scan.hip"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spaced-kmer-sketching_amd")


def assembly(src):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "scan.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-mllvm", "-amdgpu-atomic-optimizer-strategy=None",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(src),
                        "--cuda-device-only", "-S", src, "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def kernels(text):
    for m in re.finditer(r"^(_ZN3sks\S*scan_kernel\S*):.*\n", text, re.M):
        name = m.group(1)
        body = text[m.end():text.index(".Lfunc_end", m.end())]
        meta = text[text.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        notes = text[text.index("; Kernel info:", text.index(".Lfunc_end", m.end())):][:4000]
        yield name, body, meta, notes


def figures(name, body, meta, notes):
    ins = collections.Counter()
    loop_of, cur = collections.Counter(), None
    in_loop = collections.defaultdict(collections.Counter)
    # the outermost loop of every loop header: a nested header's label line
    # names it ("Parent Loop BBx_y Depth=1"), an outermost one is its own
    root = {}
    for m in re.finditer(r"^\.L(BB\w+):\s*; (?:Parent Loop (BB\w+) Depth=1|=>This Loop Header: Depth=1)", body, re.M):
        root[m.group(1)] = m.group(2) or m.group(1)
    for line in body.splitlines():
        s = line.strip()
        lab = re.match(r"(?:\.L(BB\w+)|; %bb\.\d+):", s)
        if lab:
            m = re.search(r"in Loop: Header=(BB\w+) ", s)
            cur = root.get(m.group(1)) if m else root.get(lab.group(1))
            continue
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        op = s.split()[0]
        ins[op] += 1
        if cur:
            loop_of[cur] += 1
            in_loop[cur][op] += 1
    tile_loop = in_loop[loop_of.most_common(1)[0][0]] if loop_of else collections.Counter()
    count = lambda c, pred: sum(n for op, n in c.items() if pred(op))
    meta_of = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, meta).group(1))
    note_of = lambda key: int(re.search(r"; %s: (\d+)" % key, notes).group(1))
    short = re.search(r"scan_kernel(_wide)?I\w+?E(?=EvNS)", name).group(0)
    return (f"{short} ins {sum(ins.values())} valu {count(ins, lambda o: o.startswith('v_'))}"
            f" mbcnt {count(ins, lambda o: o.startswith('v_mbcnt'))}"
            f" ds_add_rtn {count(ins, lambda o: o.startswith('ds_add_rtn'))}"
            f" gatomic {count(ins, lambda o: o.startswith('global_atomic'))}"
            f" readlane {ins['v_readlane_b32']} readlane_in_tile_loop {tile_loop['v_readlane_b32']}"
            f" gload_in_tile_loop {count(tile_loop, lambda o: o.startswith('global_load'))}"
            f" min_f64 {count(ins, lambda o: o.startswith('v_min_f64'))}"
            f" vgpr {meta_of('next_free_vgpr')} sgpr {meta_of('next_free_sgpr')}"
            f" lds {meta_of('group_segment_fixed_size')} occ {note_of('Occupancy')}"
            f" scratch {meta_of('private_segment_fixed_size')}")


if __name__ == "__main__":
    src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(PKG, "csrc", "scan.hip")
    for k in kernels(assembly(os.path.abspath(src))):
        print(figures(*k))
