"""The narrow scan's tile geometry and prefetch addressing, against the oracle,
bit-exactly (per-segment sketch, size and window count; list mode row by row).

scan_kernel keeps one segment cursor with the segment's begin, end and tile
prefixes in scalar registers, reloaded only when the cursor moves; a tile whose
last 16-byte vector ends inside the segment ("interior") is prefetched from a
scalar base plus the lane's constant offset, only a segment's last tile(s) go
through load_vec's per-lane bounds.  What can go wrong is a stale cache after a
segment change, a tile taken for interior that is not (bytes past the
segment's end become visible), or a wrong base at an alignment other than 0.

One stream, no separators between most segments (a segment's neighbours are
valid bases, so a byte read past seg_end or before the segment and not masked
shows as extra windows or k-mers), inside a larger allocation that goes on
with 8 KB of valid bases after the stream and has 16 before it:

* churn: 40 segments of 1..300 bases, some empty, some of W - 1 and W bases;
  segments of TILE - 1, TILE, TILE + 1 and 2 TILE + 17 windows (a tile edge,
  then a tile of one window, then a segment change);
* boundary: segments of TILE + d - shift bytes that start at residue `shift`
  mod 16, every residue 0..15, so the segment ends d bytes past its last tile's
  aligned base: d = 1, 15, 16, 17, and d = 16 kLoadVecs - TILE - 1, + 0, + 1
  (79, 80, 81: the tile before the last is the last tail tile, exactly
  interior, interior by one byte); a segment of exactly 2 TILE bytes (d = 0:
  the segment ends on the tile edge);
* an N in the last wave of a segment's first tile and an N in the halo words of
  a tile (checked and clean walks alternate within the segment).

The stream is handed over at pointer offsets 0, 1, 5 and 15 from a 16-byte
boundary (every residue moves with it; offsets other than 0 pack through LDS).
FracMinHash c = 1 (plain kernel), c = 8 and c = 1000 (pre-filter kernel),
bottom-s s = 64, w = 32 (the compare-and-select build) and list mode; the
default grid and forced grids of 1 and 2; static ranges and chunks of one tile
in a child process (this file as a script), as test_scan_candidate_carry does.
A second stream puts segments just past 2^31 and 2^32 bytes (zero-filled
fillers before them): the cached 64-bit values travel to the scalar registers
in halves.
"""
import os
import re
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
LOAD_VECS = 261  # scan.hip kLoadVecs: 16-byte vectors prefetched per tile
W, K = 31, 21
D_EDGE = 16 * LOAD_VECS - TILE  # 80: seg_end - last tile's base at which the tile before it turns interior
DS = [1, 15, 16, 17, D_EDGE - 1, D_EDGE, D_EDGE + 1]
ALIGNS = [0, 1, 5, 15]
GRIDS = [0, 1, 2]  # 0: the default grid
PAD_BEFORE, PAD_AFTER = 16, 8192
# (kind, parameter, window): c = 1 plain kernel, c = 8 / 1000 pre-filter kernel, bottom-s, FMIN = 0 build
CONFIGS = [("frac", 1, W), ("frac", 8, W), ("frac", 1000, W), ("bottom", 64, W), ("frac", 8, 32)]


def geometry_segments():
    """[(bytes, ends_with_separator)]; the stream is their concatenation."""
    n_of = lambda windows: windows + W - 1
    rng = np.random.default_rng(7)
    segs = []
    for i in range(40):  # churn: the segment cursor moves at every tile
        n = int(rng.integers(1, 301))
        if i % 9 == 3:
            n = 0
        elif i % 9 == 5:
            n = W - 1
        elif i % 9 == 7:
            n = W
        segs.append((synth.bases(n, seed=100 + i).tobytes(), i % 4 == 0))
    for j, wins in enumerate((TILE - 1, TILE, TILE + 1, 2 * TILE + 17)):
        segs.append((synth.bases(n_of(wins), seed=150 + j).tobytes(), j % 2 == 0))
    g = synth.bases(3 * TILE + 5, seed=160)
    g[TILE - 96] = ord("N")  # word 250 of the first tile: its last wave walks checked
    segs.append((g.tobytes(), False))
    g = synth.bases(2 * TILE + 900, seed=161)
    g[TILE + 10] = ord("N")  # first word after tile 0: its halo, and tile 1's first wave
    segs.append((g.tobytes(), False))
    segs.append((synth.bases(2 * TILE, seed=162).tobytes(), False))  # ends on the tile edge
    # boundary: start residue `shift`, end d bytes past the last tile's aligned base
    pos = sum(len(b) + (1 if sep else 0) for b, sep in segs)
    for shift in range(16):
        fill = (shift - pos) % 16
        if fill:  # a short segment of its own (a tile without a window) moves the residue
            segs.append((synth.bases(fill, seed=200 + shift).tobytes(), False))
            pos += fill
        d = DS[shift % len(DS)] if shift else D_EDGE
        if d <= shift:
            d = D_EDGE + 1
        n = TILE + d - shift
        segs.append((synth.bases(n, seed=220 + shift).tobytes(), False))
        pos += n
    for d in DS:  # every d at residue 0 and at residue 5
        for shift in (0, 5):
            fill = (shift - pos) % 16
            if fill:
                segs.append((synth.bases(fill, seed=300 + d + shift).tobytes(), False))
                pos += fill
            n = TILE + d - shift
            if n <= TILE:
                continue
            segs.append((synth.bases(n, seed=320 + 2 * d + shift).tobytes(), False))
            pos += n
    return segs


def stream_of(segs):
    stream = b"".join(b + (b"\n" if sep else b"") for b, sep in segs)
    offs = [0]
    for b, sep in segs:
        offs.append(offs[-1] + len(b) + (1 if sep else 0))
    assert offs[-1] == len(stream)
    return stream, offs


def device_stream(torch, stream, align):
    """The stream at `align` bytes past a 16-byte boundary, valid bases around it."""
    before = synth.bases(PAD_BEFORE + align, seed=901).tobytes()
    after = synth.bases(PAD_AFTER, seed=902).tobytes()
    dev = torch.frombuffer(bytearray(before + stream + after), dtype=torch.uint8).to("cuda:0")
    assert dev.data_ptr() % 16 == 0
    return dev, dev.data_ptr() + len(before)


def make_oracle(stream, offs):
    cache = {}

    def oracle(i, kind, param, w):
        key = (i, kind, param, w)
        if key not in cache:
            cache[key] = O.sketch(O.cut_runs(stream[offs[i]:offs[i + 1]]), w, O.mask(w, K, 0), kind, param)
        return cache[key]
    return oracle


def check_build(torch, ctx, stream, offs, oracle, kind, param, w, align):
    dev, ptr = device_stream(torch, stream, align)
    k = sksffi.SKS_FRAC_MOD if kind == "frac" else sksffi.SKS_BOTTOM_S
    ss = ctx.sketch_build(ptr, len(stream), offs, w, O.mask(w, K, 0), k, param)
    sizes, wins = ss.sizes(), ss.windows()
    for i in range(len(offs) - 1):
        want, nw = oracle(i, kind, param, w)
        where = (i, offs[i] % 16, offs[i + 1] - offs[i], kind, param, w, align)
        assert int(wins[i]) == nw, where
        assert int(sizes[i]) == len(want), where
        assert np.array_equal(ss.sketch(i), want), where
    ss.free()
    del dev


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.set_scan_grid(0)
    c.close()


@pytest.fixture(scope="module")
def case():
    stream, offs = stream_of(geometry_segments())
    return stream, offs, make_oracle(stream, offs)


def test_stream_shape(case):
    """The stream holds the cases the header names, and the oracle keeps
    something of every multi-tile segment at every setting used."""
    stream, offs, oracle = case
    lens = [b - a for a, b in zip(offs[:-1], offs[1:])]
    assert 0 in lens and W - 1 in lens and W in lens
    multi = [i for i, n in enumerate(lens) if n > TILE]
    assert {offs[i] % 16 for i in multi} == set(range(16))
    # seg_end - (last tile's aligned base) of the one-tile-and-a-bit segments
    ds = {(n - TILE) + offs[i] % 16 for i, n in enumerate(lens) if TILE < n < TILE + 128}
    assert set(DS) <= ds, sorted(ds)
    assert any(n == 2 * TILE for n in lens)
    assert stream.count(b"N") == 2
    for kind, param, w in CONFIGS:
        for i in multi:
            assert len(oracle(i, kind, param, w)[0]) > 0, (i, kind, param, w)


@pytest.mark.parametrize("grid", GRIDS, ids=["default", "grid1", "grid2"])
@pytest.mark.parametrize("kind,param,w", CONFIGS, ids=["c1", "c8", "c1000", "bottom64", "w32"])
def test_geometry(gpu, case, kind, param, w, grid):
    torch, ctx = gpu
    stream, offs, oracle = case
    ctx.set_scan_grid(grid)
    try:
        check_build(torch, ctx, stream, offs, oracle, kind, param, w, 0)
    finally:
        ctx.set_scan_grid(0)


@pytest.mark.parametrize("align", ALIGNS[1:])
@pytest.mark.parametrize("kind,param,w", CONFIGS, ids=["c1", "c8", "c1000", "bottom64", "w32"])
def test_pointer_alignment(gpu, case, kind, param, w, align):
    """The same stream at 1, 5 and 15 bytes past a 16-byte boundary, at the
    default grid and with one workgroup walking every tile."""
    torch, ctx = gpu
    stream, offs, oracle = case
    for grid in (0, 1):
        ctx.set_scan_grid(grid)
        try:
            check_build(torch, ctx, stream, offs, oracle, kind, param, w, align)
        finally:
            ctx.set_scan_grid(0)


@pytest.mark.parametrize("kind,param", [("frac", 8), ("bottom", 64)], ids=["c8", "bottom64"])
def test_offsets_past_2_31_and_2_32(gpu, kind, param):
    """Segments that begin past 2^31 and past 2^32 bytes: the cached begin, end
    and tile prefixes are moved to scalar registers half by half, and a low half
    with bit 31 set must not spill into the high one (a fault, not a wrong
    answer: it shows only at this size).  Two fillers of zero bytes (no window)
    put a group of segments at each offset; only the groups meet the oracle."""
    torch, ctx = gpu
    groups = [[synth.bases(n, seed=700 + 10 * g + i).tobytes() for i, n in enumerate((2 * TILE + 77, 150, TILE + D_EDGE))]
              for g in range(2)]
    starts = [(1 << 31) + 3 * TILE + 5, (1 << 32) + 7 * TILE + 11]
    total = starts[1] + sum(len(b) for b in groups[1])
    dev = torch.zeros(total + PAD_AFTER, dtype=torch.uint8, device="cuda:0")
    offs = [0]
    for g, at in enumerate(starts):
        offs.append(at)  # the filler before the group ends where the group begins
        blob = b"".join(groups[g])
        dev[at:at + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda:0")
        for b in groups[g]:
            offs.append(offs[-1] + len(b))
    assert offs[-1] == total and len(offs) == 9
    seg_bytes = dict(zip((1, 2, 3, 5, 6, 7), groups[0] + groups[1]))  # 0 and 4 are the fillers
    k = sksffi.SKS_FRAC_MOD if kind == "frac" else sksffi.SKS_BOTTOM_S
    ss = ctx.sketch_build(dev.data_ptr(), total, offs, W, O.mask(W, K, 0), k, param)
    sizes, wins = ss.sizes(), ss.windows()
    for i in range(len(offs) - 1):
        if i not in seg_bytes:
            assert int(wins[i]) == 0 and int(sizes[i]) == 0, i
            continue
        want, nw = O.sketch(O.cut_runs(seg_bytes[i]), W, O.mask(W, K, 0), kind, param)
        assert len(want) > 0
        assert int(wins[i]) == nw, (i, offs[i])
        assert int(sizes[i]) == len(want), (i, offs[i])
        assert np.array_equal(ss.sketch(i), want), (i, offs[i])
    ss.free()
    del dev


def expected_list(stream, offs, w, m, c):
    """Oracle rows of every segment with their stream positions."""
    pos, bits, counts = [], [], []
    for g in range(len(offs) - 1):
        seg = stream[offs[g]:offs[g + 1]]
        runs = O.cut_runs(seg)
        starts = [mm.start() for mm in re.finditer(rb"[ACGTacgt]+", seg)]
        assert len(starts) == len(runs)
        rows = O.kmer_list(runs, w, m, c)
        counts.append(len(rows))
        for r in rows:
            pos.append(offs[g] + starts[int(r[4])] + int(r[5]))
            bits.append([int(x) for x in r[:4]])
    return np.array(pos, np.uint64), np.array(bits, np.uint64).reshape(-1, 4), counts


@pytest.mark.parametrize("align", [0, 5])
def test_list_mode(gpu, case, align):
    """sks_kmer_list_build on the stream: the list kernel emits window start
    bytes from the tile's win0, so a wrong win0 shows in the positions."""
    torch, ctx = gpu
    stream, offs, _ = case
    m = O.mask(W, K, 0)
    dev, ptr = device_stream(torch, stream, align)
    pos, bits, counts = ctx.kmer_list(ptr, len(stream), offs, W, m, 8)
    wpos, wbits, wcounts = expected_list(stream, offs, W, m, 8)
    assert list(counts) == wcounts
    assert np.array_equal(pos, wpos)
    assert np.array_equal(bits, wbits)
    del dev


@pytest.mark.parametrize("var", ["SKS_SCAN_STATIC", "SKS_SCAN_MIN_CHUNK"])
def test_tile_order_knobs(var):
    """Static tile ranges, and dynamic chunks of one tile (every tile a new
    chunk): c = 8, c = 1000 and bottom-s at the default grid and at 1 and 2
    workgroups, pointer offsets 0 and 5, in a fresh process that reads the
    variable once."""
    env = dict(os.environ)
    env[var] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "geometry child ok" in r.stdout


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available()
    st, of = stream_of(geometry_segments())
    orc = make_oracle(st, of)
    cx = sksffi.Context(0)
    for kind_, param_, w_ in (("frac", 8, W), ("frac", 1000, W), ("bottom", 64, W)):
        for grid_ in GRIDS:
            cx.set_scan_grid(grid_)
            for align_ in (0, 5):
                check_build(torch, cx, st, of, orc, kind_, param_, w_, align_)
    cx.set_scan_grid(0)
    cx.close()
    print("geometry child ok")
