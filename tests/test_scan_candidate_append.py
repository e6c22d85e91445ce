"""The pre-filter scan's candidate append and every scan's queue-full direct
path against the oracle, bit-exactly (sketch, sizes, windows; list mode:
positions in order and all four bit fields).

scan_kernel<frac, 0, PRE = 1> appends a window that passes the low-bits
pre-filter to its wave's candidate list at the slot a returning LDS atomic on
the wave's cursor hands out; a scalar count follows the cursor, the list is
finished 64 at a time, the rest (0..63 candidates) moves to the front and one
lane resets the cursor to 16 * rest.  The cursor is zeroed per tile.  scan.hip
is built without the compiler's atomic optimizer, so where it wants one global
atomic per wave — the direct write of a survivor that finds the LDS queue full
— it aggregates by hand (wave_aggregated_inc), in the narrow and the wide
kernel, in every mode.

Cursor cases: c = 2 passes every other window (~32 candidates per wave-window:
a finish nearly every other window, with every rest value), c = 4, 8, 16 pass
1/4, 1/8 and 1/16 (four bits are the pre-filter's limit), c = 48 = 16 * 3 and
c = 1000 = 8 * 125 pass 1/16 and 1/8 and leave a divisor to the finish, and the
lists cross 64 at every point of a tile.  A forced grid of 1 or 2 workgroups
makes one workgroup walk every tile, so the cursor's reset crosses tiles,
chunks and segment changes.

Direct-path cases: three tiles whose every window survives (or every other
one), thousands per tile against queues of 512 (frac, bottom-s), 2048 (list)
and 1024 (wide) entries.
"""
import re

import numpy as np
import pytest

import pyoracle as O
import sksffi
import synth

pytestmark = pytest.mark.gpu

TILE = 4096
W, K = 31, 21


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.set_scan_grid(0)
    c.close()


@pytest.fixture
def scan_grid(gpu):
    """set(g) forces the scan grid; the default is back when the test returns,
    however it returns."""
    _, ctx = gpu
    try:
        yield ctx.set_scan_grid
    finally:
        ctx.set_scan_grid(0)


def _stream(genomes):
    stream = b"".join(g + b"\n" for g in genomes)
    offs = [0]
    for g in genomes:
        offs.append(offs[-1] + len(g) + 1)
    return stream, offs


def _upload(torch, stream):
    d = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
    assert d.data_ptr() % 16 == 0  # segment offsets below are alignments
    return d


_oracle_cache = {}


def _oracle(g, w, m, kind, param, flavour=0):
    key = (g, w, m, kind, param, flavour)
    if key not in _oracle_cache:
        _oracle_cache[key] = O.sketch(O.cut_runs(g), w, m, kind, param, 1, flavour)
    return _oracle_cache[key]


def _check(gpu, genomes, w, m, kind, param, flavour=0):
    torch, ctx = gpu
    stream, offs = _stream(genomes)
    dev = _upload(torch, stream)
    k = sksffi.SKS_FRAC_MOD if kind == "frac" else sksffi.SKS_BOTTOM_S
    ss = ctx.sketch_build(dev.data_ptr(), len(stream), offs, w, m, k, param, 1, flavour)
    sizes, wins = ss.sizes(), ss.windows()
    for i, g in enumerate(genomes):
        want, nw = _oracle(g, w, m, kind, param, flavour)
        where = (i, len(g), w, kind, param, flavour)
        assert int(wins[i]) == nw, where
        assert int(sizes[i]) == len(want), where
        assert np.array_equal(ss.sketch(i), want), where
    return sizes


# ---- the cursor and the finish -------------------------------------------------------------
@pytest.fixture(scope="module")
def cursor_genomes():
    """Nothing, one base short of a window, one window; one clean tile; three
    tiles with a single N in the second (its wave takes the checked loop, the
    neighbours the unrolled one); ~40 kb with lower case.  The segment offsets
    fall on alignments 0, 1, 0, 0, 15 and 14 modulo 16: the register pack and
    the pack through LDS."""
    out = [b"", synth.bases(W - 1, seed=21).tobytes(), synth.bases(W, seed=22).tobytes(),
           synth.bases(TILE + 30, seed=23).tobytes()]
    g = synth.bases(3 * TILE - 2, seed=24)
    g[TILE + 1500] = ord("N")
    out.append(g.tobytes())
    g = synth.bases(40013, seed=25)
    idx = np.random.default_rng(3).integers(0, len(g), len(g) // 7)
    g[idx] = g[idx] | 0x20
    out.append(g.tobytes())
    _, offs = _stream(out)
    assert [o % 16 for o in offs[:-1]] == [0, 1, 0, 0, 15, 14]
    return out


@pytest.mark.parametrize("c", [2, 4, 8, 16, 48, 1000])
def test_candidate_cursor(gpu, scan_grid, cursor_genomes, c):
    m = O.mask(W, K, 0)
    sizes = _check(gpu, cursor_genomes, W, m, "frac", c)
    if c == 2:  # ~32 candidates per wave-window: the lists fill and are finished throughout
        assert int(sizes[5]) > 15000
    for grid in (1, 2):
        scan_grid(grid)
        _check(gpu, cursor_genomes, W, m, "frac", c)


# ---- the direct path, every mode -----------------------------------------------------------
@pytest.fixture(scope="module")
def three_tiles():
    """Exactly three tiles with the separator, no invalid byte: 4096 windows per
    full tile."""
    return [synth.bases(3 * TILE - 1, seed=31).tobytes()]


@pytest.mark.parametrize("c", [2, 1], ids=["prefilter_c2", "plain_c1"])
def test_direct_path_frac(gpu, three_tiles, c):
    """c = 2: ~2048 survivors per tile out of the candidate finish; c = 1: 4096
    out of the keep-mask loop; both against the 512-entry queue."""
    sizes = _check(gpu, three_tiles, W, O.mask(W, K, 0), "frac", c)
    assert int(sizes[0]) > 0.9 * 3 * TILE / c  # distinct k-mers: nearly one per surviving window


def test_direct_path_bottom_s_keeps_everything(gpu, three_tiles):
    """s at least the window count: the threshold passes every window."""
    s = 3 * TILE
    sizes = _check(gpu, three_tiles, W, O.mask(W, K, 0), "bottom", s)
    assert 3 * TILE - 200 < int(sizes[0]) <= 3 * TILE - W


def test_direct_path_wide(gpu, three_tiles):
    """w = 45 at c = 1: scan_kernel_wide, 4096 survivors per tile against 1024."""
    sizes = _check(gpu, three_tiles, 45, O.mask(45, 30, 2), "frac", 1)
    assert int(sizes[0]) > 3 * TILE - 200


def test_direct_path_list_mode(gpu, three_tiles):
    """sks_kmer_list_build at c = 1: 4096 positions per tile against the
    2048-entry queue; positions in order and the four bit fields."""
    torch, ctx = gpu
    m = O.mask(W, K, 1)
    stream, offs = _stream(three_tiles)
    dev = _upload(torch, stream)
    pos, bits, counts = ctx.kmer_list(dev.data_ptr(), len(stream), offs, W, m, 1)
    seg = stream[offs[0]:offs[1]]
    runs = O.cut_runs(seg)
    starts = np.array([mm.start() for mm in re.finditer(rb"[ACGTacgt]+", seg)], np.uint64)
    assert len(starts) == len(runs) == 1
    rows = O.kmer_list(runs, W, m, 1)
    assert list(counts) == [len(rows)] == [3 * TILE - 1 - W + 1]
    assert np.array_equal(pos, starts[rows[:, 4].astype(np.int64)] + rows[:, 5])
    assert np.array_equal(bits, rows[:, :4])
