"""The pre-filter scan's candidate list at tile edges and segment changes,
against the oracle, bit-exactly (per-segment sketch, size and window count).

scan_kernel<frac, 0, PRE = 1> queues its candidates per wave, finishes them 64
at a time and finishes the last 0..63 of a tile at that tile's end, to the
tile's segment.  Carrying that rest into the next tile instead (drained only
where the segment changes and after the last tile) was built and measured in
round 10 and did not pay, so the per-tile finish stays;
these are the cases such a carry has to pass, and the per-tile finish passes
them now.  A candidate finished to the wrong segment shows as a size mismatch
on two neighbouring segments; one lost or finished twice as a size or content
mismatch (sizes and windows are compared as well as the sorted sketches).

One stream: segments of 0, W - 1 and W bases (no tile work, one window), of
TILE - 1, TILE and TILE + 1 windows (a tile edge followed by a tile of one
window or of none), of 2 TILE + 17 windows, one whose first tile holds a single
N in its last wave (a checked walk appends to the list, clean walks follow in
the next tiles), and a last one that ends mid-tile with candidates pending.
c = 2, 8, 16 pass 1/2, 1/8, 1/16 of the windows to the list, c = 48 and
c = 1000 pass 1/16 and 1/8 and leave a divisor to the finish.  Forced grids of
1 and 2 workgroups make one workgroup walk every tile and every segment
change; the static tile ranges (SKS_SCAN_STATIC) and chunks of one tile
(SKS_SCAN_MIN_CHUNK=1) are read once per process, so they run in a child
process (this file as a script).  The bottom-s build of the same stream runs
the kernels without the list.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the child process: the paths tests/conftest.py sets up
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "spaced-kmer-sketching_amd"), os.path.join(_root, "oracle"),
               os.path.join(_root, "tests")):
        sys.path.insert(0, _p)

import pyoracle as O
import sksffi
import synth

pytestmark = pytest.mark.gpu

TILE = 4096
W, K = 31, 21
CS = [2, 8, 16, 48, 1000]
GRIDS = [0, 1, 2]  # 0: the default grid


def carry_genomes():
    n_of = lambda windows: windows + W - 1  # bases of a segment with that many windows
    out = [b"", synth.bases(W - 1, seed=41).tobytes(), synth.bases(W, seed=42).tobytes(),
           synth.bases(n_of(TILE - 1), seed=43).tobytes(), synth.bases(n_of(TILE), seed=44).tobytes(),
           synth.bases(n_of(TILE + 1), seed=45).tobytes(), synth.bases(n_of(2 * TILE + 17), seed=46).tobytes()]
    g = synth.bases(3 * TILE + 5, seed=47)
    g[TILE - 96] = ord("N")  # word 250 of the first tile: its last wave (words 192..255) walks checked
    out.append(g.tobytes())
    out.append(synth.bases(TILE + 1800, seed=48).tobytes())  # ends mid-tile, candidates pending
    return out


def stream_of(genomes):
    stream = b"".join(g + b"\n" for g in genomes)
    offs = [0]
    for g in genomes:
        offs.append(offs[-1] + len(g) + 1)
    return stream, offs


def check_stream(torch, ctx, genomes, kind, param, oracle):
    """Build on the device and compare every segment with oracle[(i, kind, param)]."""
    stream, offs = stream_of(genomes)
    dev = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
    assert dev.data_ptr() % 16 == 0  # the segment offsets are alignments
    k = sksffi.SKS_FRAC_MOD if kind == "frac" else sksffi.SKS_BOTTOM_S
    ss = ctx.sketch_build(dev.data_ptr(), len(stream), offs, W, O.mask(W, K, 0), k, param)
    sizes, wins = ss.sizes(), ss.windows()
    for i, g in enumerate(genomes):
        want, nw = oracle(i, kind, param)
        where = (i, len(g), kind, param)
        assert int(wins[i]) == nw, where
        assert int(sizes[i]) == len(want), where
        assert np.array_equal(ss.sketch(i), want), where
    return sizes


def make_oracle(genomes):
    cache = {}

    def oracle(i, kind, param):
        key = (i, kind, param)
        if key not in cache:
            cache[key] = O.sketch(O.cut_runs(genomes[i]), W, O.mask(W, K, 0), kind, param)
        return cache[key]
    return oracle


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.set_scan_grid(0)
    c.close()


@pytest.fixture(scope="module")
def genomes():
    out = carry_genomes()
    _, offs = stream_of(out)
    al = {o % 16 for o in offs[:-1]}
    assert 0 in al and len(al) > 2, sorted(al)  # the register pack and the pack through LDS
    return out


@pytest.fixture(scope="module")
def oracle(genomes):
    return make_oracle(genomes)


def test_stream_shape(genomes):
    """The segments are the ones the cases above name."""
    wins = [max(0, len(g) - W + 1) for g in genomes]
    assert wins[:7] == [0, 0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 17]
    assert genomes[7].count(b"N") == 1 and 3 * 1024 <= genomes[7].index(b"N") < TILE
    assert 0 < len(genomes[8]) % TILE < TILE - W


@pytest.mark.parametrize("grid", GRIDS, ids=["default", "grid1", "grid2"])
@pytest.mark.parametrize("c", CS)
def test_carry(gpu, genomes, oracle, c, grid):
    torch, ctx = gpu
    ctx.set_scan_grid(grid)
    try:
        sizes = check_stream(torch, ctx, genomes, "frac", c, oracle)
    finally:
        ctx.set_scan_grid(0)
    if c == 2:  # every other window: the lists fill and are finished throughout
        assert int(sizes[6]) > 0.45 * (2 * TILE + 17)


@pytest.mark.parametrize("grid", GRIDS, ids=["default", "grid1", "grid2"])
def test_bottom_s_same_stream(gpu, genomes, oracle, grid):
    """The kernels without a candidate list, on the same stream."""
    torch, ctx = gpu
    ctx.set_scan_grid(grid)
    try:
        check_stream(torch, ctx, genomes, "bottom", 300, oracle)
    finally:
        ctx.set_scan_grid(0)


@pytest.mark.parametrize("var", ["SKS_SCAN_STATIC", "SKS_SCAN_MIN_CHUNK"])
def test_carry_tile_order_knobs(var):
    """Static tile ranges, and dynamic chunks of one tile (every tile a new
    chunk): c = 8 and c = 1000 at the default grid and at 1 and 2 workgroups,
    in a fresh process that reads the variable once."""
    env = dict(os.environ)
    env[var] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "carry child ok" in r.stdout


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available()
    gs = carry_genomes()
    orc = make_oracle(gs)
    cx = sksffi.Context(0)
    for c_ in (8, 1000):
        for grid_ in GRIDS:
            cx.set_scan_grid(grid_)
            check_stream(torch, cx, gs, "frac", c_, orc)
    cx.set_scan_grid(0)
    cx.close()
    print("carry child ok")
