"""The narrow scan's lane layout against the oracle, bit-exactly (sketch, sizes,
windows; list mode: positions and both bit fields).

scan_kernel's lane (g, r) owns the 16 window starts 16 (16 g + m) + r of a
4096-start tile: a window's F and R share a 32-bit word with the lane's previous
window, both funnel shifts are per-lane constants derived from r and w, validity
is read from the invalid map at word 16 g + m, bit r, and the clean / checked
choice is made per wave (1024 starts).  Tiles that start on a 16-byte boundary
are packed from the prefetch registers, the others through LDS.  The cases sit
at the edges of exactly these units — word (16 bases), lane group (256), wave
(1024), tile (4096), chunk (3 to 16 tiles) — at the smallest sizes that reach
them; c = 1 keeps every window, so every window's canonical k-mer is compared.
"""
import re

import numpy as np
import pytest

import pyoracle as O
import sksffi
import synth

pytestmark = pytest.mark.gpu

TILE = 4096
# (w, k): contiguous and spaced masks; w <= 16 shifts F by a whole word and a
# part, w = 32 not at all
WINDOWS = [(1, 1), (2, 2), (15, 15), (15, 11), (16, 16), (16, 11), (17, 17), (17, 11), (21, 21),
           (21, 15), (31, 31), (31, 21), (32, 32), (32, 20)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.close()


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


def _check(gpu, genomes, w, m, kind, param, flavour=0):
    torch, ctx = gpu
    stream, offs = _stream(genomes)
    dev = _upload(torch, stream)
    k = sksffi.SKS_FRAC_MOD if kind == "frac" else sksffi.SKS_BOTTOM_S
    ss = ctx.sketch_build(dev.data_ptr(), len(stream), offs, w, m, k, param, 1, flavour)
    sizes, wins = ss.sizes(), ss.windows()
    for i, g in enumerate(genomes):
        want, nw = _oracle(g, w, m, kind, param, flavour)
        assert int(wins[i]) == nw, (i, len(g), w, kind, param, flavour)
        assert int(sizes[i]) == len(want), (i, len(g), w, kind, param, flavour)
        assert np.array_equal(ss.sketch(i), want), (i, len(g), w, kind, param, flavour)


_oracle_cache = {}


def _oracle(g, w, m, kind, param, flavour):
    key = (g, w, m, kind, param, flavour)
    if key not in _oracle_cache:
        _oracle_cache[key] = O.sketch(O.cut_runs(g), w, m, kind, param, 1, flavour)
    return _oracle_cache[key]


def _lengths(w):
    """Segment lengths around a word, a lane group, a wave, a tile and a chunk."""
    return [15, 16, 17, 255, 256, 257, 256 + w - 1, 1023, 1024 + w - 1, TILE - 1, TILE, TILE + 1,
            TILE + w - 1, 3 * TILE - 1, 3 * TILE + 1, 16 * TILE + w]


@pytest.mark.parametrize("w,k", WINDOWS)
def test_window_sizes_and_segment_lengths(gpu, w, k):
    """Every window size class over segments that end just before, at and just
    after each unit, all in one build (consecutive tiles change segment, and the
    segments start at every kind of misalignment).  c = 1: all windows kept."""
    genomes = [synth.bases(L, seed=300 + i).tobytes() for i, L in enumerate(_lengths(w))]
    _check(gpu, genomes, w, O.mask(w, k, 5), "frac", 1)


def test_segment_start_misalignment(gpu):
    """A 2-tile-and-a-bit genome starting at every offset 0..15 modulo 16 (the
    first genome is 16 k + i bases and its separator one more): offset 0 packs
    from the prefetch registers, multiples of 4 and the rest through LDS.  The
    first genome starts at 0 and is itself longer than a tile once.  c = 1 and the
    pre-filter kernel (c = 2)."""
    w, k = 31, 21
    m = O.mask(w, k, 0)
    body = synth.bases(2 * TILE + 77, seed=41)
    body[5000] = ord("N")
    body = body.tobytes()
    seen = set()
    for i in range(16):
        first = synth.bases(48 + i + (TILE if i == 3 else 0), seed=42).tobytes()
        seen.add((len(first) + 1) % 16)
        for c in (1, 2):
            _check(gpu, [first, body], w, m, "frac", c)
    assert seen == set(range(16))


def _n_positions(w):
    pos = {16 * 5, 16 * 5 + 15,            # a word's first and last base
           255, 256, 3 * 256 - 1, 3 * 256,  # a lane group's last and first base
           1023, 1024, 3071, 3072,          # a wave's last and first base
           TILE - w, TILE - 1,              # the tile's last w bases
           TILE, TILE + w - 2,              # the next tile's first w - 1 bases: the halo decides
           2 * TILE - 1, 2 * TILE}
    return sorted(p for p in pos if p >= 0)


@pytest.mark.parametrize("w,k", [(31, 21), (17, 17), (2, 2)])
def test_single_invalid_byte(gpu, w, k):
    """One N in an otherwise clean 3-tile genome, at the edges of each unit:
    the wave holding it (and the one before, whose windows reach it) takes the
    checked loop, the others the unrolled one, in the same launch.  Non-PRE
    (c = 1) and pre-filter (c = 2) kernels."""
    m = O.mask(w, k, 1)
    clean = synth.bases(3 * TILE, seed=77)
    for p in _n_positions(w):
        g = clean.copy()
        g[p] = ord("N")
        g = g.tobytes()
        for c in (1, 2):
            _check(gpu, [g], w, m, "frac", c)


@pytest.fixture(scope="module")
def mode_genomes():
    rng = np.random.default_rng(9)
    out = []
    for i, L in enumerate([0, 30, 257, TILE + 30, 3 * TILE + 1, 16 * TILE + 31, 70001]):
        g = synth.bases(L, seed=500 + i)
        if L > 1000:
            g[rng.integers(0, L, 3)] = ord("N")
            idx = rng.integers(0, L, L // 10)
            g[idx] = g[idx] | 0x20  # lower case
        out.append(g.tobytes())
    return out


@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("c", [1, 7, 1000])
def test_frac_modes(gpu, mode_genomes, c, flavour):
    """FracMinHash with c = 1 and 7 (keep-mask loop) and 1000 (even: the
    pre-filter kernel for the boost-mix flavour), both hash flavours."""
    w, k = 31, 21
    _check(gpu, mode_genomes, w, O.mask(w, k, 0), "frac", c, flavour)


@pytest.mark.parametrize("flavour", [0, 1])
def test_bottom_s(gpu, mode_genomes, flavour):
    w, k = 31, 21
    _check(gpu, mode_genomes, w, O.mask(w, k, 0), "bottom", 1000, flavour)


@pytest.mark.parametrize("w,k,c", [(31, 21, 1), (16, 11, 1), (21, 21, 3)])
def test_list_mode_positions(gpu, mode_genomes, w, k, c):
    """sks_kmer_list_build: the list-mode scan emits window start positions, so
    the lane -> start map itself is checked, in order, with both bit fields."""
    torch, ctx = gpu
    genomes = mode_genomes[:5]
    stream, offs = _stream(genomes)
    m = O.mask(w, k, 1)
    dev = _upload(torch, stream)
    pos, bits, counts = ctx.kmer_list(dev.data_ptr(), len(stream), offs, w, m, c)
    wpos, wbits, wcounts = [], [], []
    for g in range(len(genomes)):
        seg = stream[offs[g]:offs[g + 1]]
        runs = O.cut_runs(seg)
        starts = [mm.start() for mm in re.finditer(rb"[ACGTacgt]+", seg)]
        assert len(starts) == len(runs)
        rows = O.kmer_list(runs, w, m, c)
        wcounts.append(len(rows))
        for r in rows:
            wpos.append(offs[g] + starts[int(r[4])] + int(r[5]))
            wbits.append([int(x) for x in r[:4]])
    assert list(counts) == wcounts
    assert np.array_equal(pos, np.array(wpos, np.uint64))
    assert np.array_equal(bits, np.array(wbits, np.uint64).reshape(-1, 4))
