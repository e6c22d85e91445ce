"""The 128-bit scan (scan_kernel_wide, 32 < w <= 64) at its layout edges, every
statically partitioned scan under forced grids, and the post-processing under
caller-made masks — all bit-exact against the oracle (sketch, sizes, windows;
list mode: positions in order and all four bit fields).

The wide kernel's lane t owns the 16 consecutive window starts 16 t + j of a
4096-start tile: F is the 128 big-endian bits from its word shifted right by
fshift = 128 - 2 w (0..62: across or inside a 64-bit half, and 32 at w = 48),
validity is bits [j, j + w) of an 80-bit invalid map held as a 64-bit and a
16-bit part, and a tile reads a 64-base halo of the next one.  Its workgroups
walk static ranges of tiles (as list mode does at both widths): the grid is
16 x the resident workgroups, so a build under ~16 Mb gives every workgroup one
tile, and only Context.set_scan_grid makes a small build walk several — the
prefetch cursor, the publish of the previous segment's survivors and windows at
a segment change, and the queue carried over a tile boundary.  c = 1 keeps
every window, so every window's canonical k-mer is compared.
"""
import re

import numpy as np
import pytest

import pyoracle as O
import sksffi
import synth

pytestmark = pytest.mark.gpu

TILE = 4096
# (w, k): fshift 62, 48, 34, 32, 30, 2, 0; contiguous and spaced masks
WIDE_WINDOWS = [(33, 33), (33, 20), (40, 21), (47, 47), (48, 48), (48, 30), (49, 25), (63, 63),
                (63, 30), (64, 64), (64, 40)]


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
    """Each genome plus a separator; None is a segment of zero bytes (no tile)."""
    stream = b"".join(g + b"\n" for g in genomes if g is not None)
    offs = [0]
    for g in genomes:
        offs.append(offs[-1] + (len(g) + 1 if g is not None else 0))
    return stream, offs


def _upload(torch, stream):
    d = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
    assert d.data_ptr() % 16 == 0  # segment offsets below are alignments
    return d


_oracle_cache = {}


def _oracle(g, w, m, kind, param, flavour):
    key = (g, w, m, kind, param, flavour)
    if key not in _oracle_cache:
        _oracle_cache[key] = O.sketch(O.cut_runs(g or b""), w, m, kind, param, 1, flavour)
    return _oracle_cache[key]


def _build(gpu, genomes, w, m, kind, param, flavour=0):
    """-> (sizes, windows, [sketch])."""
    torch, ctx = gpu
    stream, offs = _stream(genomes)
    dev = _upload(torch, stream)
    k = sksffi.SKS_FRAC_MOD if kind == "frac" else sksffi.SKS_BOTTOM_S
    ss = ctx.sketch_build(dev.data_ptr(), len(stream), offs, w, m, k, param, 1, flavour)
    assert ss.elem_words == (2 if w > 32 else 1)
    return ss.sizes().copy(), ss.windows().copy(), [ss.sketch(i) for i in range(len(genomes))]


def _check(gpu, genomes, w, m, kind, param, flavour=0):
    sizes, wins, sk = _build(gpu, genomes, w, m, kind, param, flavour)
    for i, g in enumerate(genomes):
        want, nw = _oracle(g, w, m, kind, param, flavour)
        where = (i, len(g or b""), w, kind, param, flavour)
        assert int(wins[i]) == nw, where
        assert int(sizes[i]) == len(want), where
        assert np.array_equal(sk[i], want), where
    return sizes, wins, sk


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[2]) == len(b[2]) and
            all(np.array_equal(x, y) for x, y in zip(a[2], b[2])))


# ---- A. window classes x segment lengths ---------------------------------------------------
def _lengths(w):
    """Nothing, one window short, one window; around a word, a lane's 16 starts
    times 16, a quarter tile, a tile and several tiles."""
    return [0, w - 1, w, 15, 16, 17, 255, 256, 257, 1023, 1024 + w - 1, TILE - 1, TILE, TILE + 1,
            TILE + w - 1, 3 * TILE - 1, 3 * TILE + 1, 16 * TILE + w]


def _length_genomes(w):
    return [synth.bases(L, seed=300 + i).tobytes() for i, L in enumerate(_lengths(w))]


@pytest.mark.parametrize("w,k", WIDE_WINDOWS)
def test_window_sizes_and_segment_lengths(gpu, w, k):
    """Every fshift class over segments that end just before, at and just after
    each unit, all in one build: consecutive tiles change segment and the
    segments start at many misalignments.  c = 1: all windows kept."""
    _check(gpu, _length_genomes(w), w, O.mask(w, k, 5), "frac", 1)


@pytest.mark.parametrize("w,k", [(33, 20), (48, 30), (64, 64)])
def test_window_sizes_and_segment_lengths_legacy_hash(gpu, w, k):
    _check(gpu, _length_genomes(w), w, O.mask(w, k, 5), "frac", 1, 1)


# ---- B. segment-start misalignment ---------------------------------------------------------
@pytest.mark.parametrize("w,k", [(45, 30), (64, 40)])
def test_segment_start_misalignment(gpu, w, k):
    """A 2-tile-and-a-bit genome with one N starting at every offset 0..15 modulo
    16 (the first genome is 16 n + i bases and its separator one more): the wide
    kernel packs every tile through LDS at byte offset `shift`, a dword index and
    a funnel shift.  The first genome is itself longer than a tile once."""
    m = O.mask(w, k, 0)
    body = synth.bases(2 * TILE + 77, seed=41)
    body[5000] = ord("N")
    body = body.tobytes()
    seen = set()
    for i in range(16):
        first = synth.bases(48 + i + (TILE if i == 3 else 0), seed=42).tobytes()
        seen.add((len(first) + 1) % 16)
        for c in (1, 50):
            _check(gpu, [first, body], w, m, "frac", c)
    assert seen == set(range(16))


# ---- C. one invalid byte at each edge ------------------------------------------------------
def _n_positions(w):
    return sorted({80, 95,                        # a word's first and last base
                   16 * 7 + 63, 16 * 7 + 64,      # lane 7's invalid map: bit 63 of inv_lo, bit 0 of inv_hi
                   16 * 7 + 79,                   # the map's last bit
                   TILE - w, TILE - 1,            # the tile's last w bases
                   TILE, TILE + w - 2,            # the next tile's first w - 1: the halo decides
                   TILE + 63,                     # the last halo base
                   2 * TILE - 1, 2 * TILE})


@pytest.mark.parametrize("w,k", [(33, 33), (48, 30), (64, 64)])
def test_single_invalid_byte(gpu, w, k):
    """One N in an otherwise clean 3-tile genome at the edges of each unit, then
    two N exactly w apart (w - 1 bases between them: no valid window there) and
    w + 1 apart (w bases: exactly one)."""
    m = O.mask(w, k, 1)
    clean = synth.bases(3 * TILE, seed=77)
    total = 3 * TILE - w + 1
    for p in _n_positions(w):
        g = clean.copy()
        g[p] = ord("N")
        g = g.tobytes()
        assert _oracle(g, w, m, "frac", 1, 0)[1] == total - (min(p, total - 1) - max(p - w + 1, 0) + 1)
        _check(gpu, [g], w, m, "frac", 1)
    for first in (1000, TILE - 20):  # inside a tile, and across the tile edge
        for gap, between in ((w, 0), (w + 1, 1)):
            g = clean.copy()
            g[first] = g[first + gap] = ord("N")
            g = g.tobytes()
            want_windows = (first - w + 1) + between + (3 * TILE - (first + gap + 1) - w + 1)
            assert _oracle(g, w, m, "frac", 1, 0)[1] == want_windows
            _check(gpu, [g], w, m, "frac", 1)


# ---- D. forced scan grids ------------------------------------------------------------------
GRIDS = [1, 2, 3, 7]


@pytest.fixture(scope="module")
def grid_genomes():
    """42 tiles in 15 segments (a segment is the genome and its separator):
    3 1 0 1 1 1 9 1 2 6 1 8 1 4 3 tiles — empty, zero bytes, shorter than w, under a
    tile, exactly one tile (4095 + separator), one base more (a second tile
    holding only the separator), exactly 4 tiles, and 2 to 9 tiles.  Grid 2 splits
    at tile 21 (inside the 6-tile segment), grid 3 at 14 and 28 (inside the 9-
    and the 8-tile ones), grid 7 every 6 tiles: ranges begin and end mid-segment
    and span up to five whole segments.  The long segments hold N and lower case."""
    lens = [2 * TILE + 100, 0, None, 30, 3000, TILE - 1, 9 * TILE - 50, 700, TILE, 5 * TILE + 1234, 44,
            7 * TILE + 9, 1500, 4 * TILE - 1, 2 * TILE + 2000]
    rng = np.random.default_rng(12)
    out = []
    for i, L in enumerate(lens):
        if L is None:
            out.append(None)
            continue
        g = synth.bases(L, seed=700 + i)
        if L > 1000 and i % 2 == 0:
            g[rng.integers(0, L, 3)] = ord("N")
            idx = rng.integers(0, L, L // 10)
            g[idx] = g[idx] | 0x20
        out.append(g.tobytes())
    tiles = [(len(g) + 1 + TILE - 1) // TILE if g is not None else 0 for g in out]
    assert tiles == [3, 1, 0, 1, 1, 1, 9, 1, 2, 6, 1, 8, 1, 4, 3]
    return out


_default_grid = {}


def _check_grids(gpu, scan_grid, genomes, w, m, kind, param):
    """The oracle's result at every forced grid, and the default grid's."""
    key = (w, m, kind, param)
    if key not in _default_grid:
        _default_grid[key] = _check(gpu, genomes, w, m, kind, param)
    for g in GRIDS:
        scan_grid(g)
        assert _same(_check(gpu, genomes, w, m, kind, param), _default_grid[key]), g


@pytest.mark.parametrize("w,k", [(45, 30), (64, 64)])
@pytest.mark.parametrize("kind,param", [("frac", 1), ("frac", 50), ("bottom", 300)])
def test_forced_grid_wide(gpu, scan_grid, grid_genomes, w, k, kind, param):
    """scan_kernel_wide walking 42, 21, 14 and 6 tiles per workgroup.  c = 1: a
    full tile's 4096 survivors against the 1024-entry queue, so the direct
    writes run on every tile between flushes; c = 50: ~80 per tile, under half
    the queue, so survivors and window counts are carried over tile boundaries
    and published at the segment change; bottom-s: the three-column queue."""
    _check_grids(gpu, scan_grid, grid_genomes, w, O.mask(w, k, 2), kind, param)


@pytest.mark.parametrize("kind,param", [("frac", 1), ("frac", 2), ("frac", 1000), ("bottom", 300)])
def test_forced_grid_narrow_dynamic(gpu, scan_grid, grid_genomes, kind, param):
    """The narrow kernels' dynamic chunks of 3 tiles with 1, 2, 3 and 7 workgroups
    grabbing all 14: c = 1, the pre-filter kernel (even c) and bottom-s."""
    _check_grids(gpu, scan_grid, grid_genomes, 31, O.mask(31, 21, 2), kind, param)


def test_forced_grid_single_genome_bottom(gpu, scan_grid):
    """build_bottom_single: one narrow genome of 6 tiles scanned by one workgroup."""
    g = synth.bases(6 * TILE - 10, seed=731)
    g[10000] = ord("N")
    genomes = [g.tobytes()]
    m = O.mask(31, 21, 2)
    want = _check(gpu, genomes, 31, m, "bottom", 300)
    scan_grid(1)
    assert _same(_check(gpu, genomes, 31, m, "bottom", 300), want)


_list_oracle = {}


def _list_want(genomes, w, m, c):
    key = (w, m, c)
    if key not in _list_oracle:
        stream, offs = _stream(genomes)
        pos, bits, counts = [], [], []
        for g in range(len(genomes)):
            seg = stream[offs[g]:offs[g + 1]]
            runs = O.cut_runs(seg)
            starts = np.array([mm.start() for mm in re.finditer(rb"[ACGTacgt]+", seg)], np.uint64)
            assert len(starts) == len(runs)
            rows = O.kmer_list(runs, w, m, c)
            counts.append(len(rows))
            if len(rows):
                pos.append(np.uint64(offs[g]) + starts[rows[:, 4].astype(np.int64)] + rows[:, 5])
                bits.append(rows[:, :4])
        _list_oracle[key] = (np.concatenate(pos), np.concatenate(bits), counts)
    return _list_oracle[key]


@pytest.mark.parametrize("w,k,c", [(31, 21, 1), (45, 30, 3)])
def test_forced_grid_list_mode(gpu, scan_grid, grid_genomes, w, k, c):
    """sks_kmer_list_build uses static tile ranges at both widths: window start
    positions in order and the four bit fields, at the default and every forced
    grid."""
    torch, ctx = gpu
    m = O.mask(w, k, 1)
    stream, offs = _stream(grid_genomes)
    dev = _upload(torch, stream)
    wpos, wbits, wcounts = _list_want(grid_genomes, w, m, c)
    assert len(wpos) > 10 * TILE
    for g in [0] + GRIDS:
        scan_grid(g)
        pos, bits, counts = ctx.kmer_list(dev.data_ptr(), len(stream), offs, w, m, c)
        assert list(counts) == wcounts, g
        assert np.array_equal(pos, wpos), g
        assert np.array_equal(bits, wbits), g


# ---- E. wide bottom-s and retries ----------------------------------------------------------
@pytest.fixture(scope="module")
def bottom_genomes():
    rng = np.random.default_rng(5)
    out = []
    for i, L in enumerate([0, 10, 64, 500, 9000, 60000]):
        g = synth.bases(L, seed=900 + i)
        if L >= 500:
            g[rng.integers(0, L, max(1, L // 3000))] = ord("N")
        out.append(g.tobytes())
    return out


@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("w,k", [(33, 33), (45, 30), (64, 40), (64, 64)])
def test_bottom_s_wide(gpu, bottom_genomes, w, k, flavour):
    """Wide bottom-s (three-column compaction, the index-permutation sort by
    (fmh, hi, lo), out_hi) from s = 1 to s above every genome's windows."""
    genomes = list(bottom_genomes)
    genomes[2] = genomes[2][:w]  # exactly one window
    m = O.mask(w, k, 4)
    for s in (1, 10, 1000, 20000):
        _check(gpu, genomes, w, m, "bottom", s, flavour)


@pytest.fixture(scope="module")
def many_genomes():
    return [synth.bases(2000 + 517 * (i % 41), seed=800 + i % 7, mut_seed=1200 + i,
                        mut_rate=0.01 * (i % 5)).tobytes() for i in range(300)]


@pytest.mark.parametrize("s,flavour", [(1, 0), (200, 0), (200, 1), (1500, 0)])
def test_bottom_s_wide_many_genomes(gpu, many_genomes, s, flavour):
    """300 genomes in one wide bottom-s build, related and unrelated, lengths
    around the candidate margin."""
    _check(gpu, many_genomes, 45, O.mask(45, 30, 2), "bottom", s, flavour)


@pytest.mark.parametrize("s", [30, 5000])
def test_bottom_s_wide_threshold_retry_mixed_passes(gpu, s):
    """A periodic genome (37 distinct windows) between two ordinary ones: it has
    fewer than s distinct candidates under the first threshold, so its
    threshold is raised while the others finish in the first pass, and the set is
    assembled from several passes in segment order with two words per element."""
    _, ctx = gpu
    unit = synth.bases(37, seed=4).tobytes()
    genomes = [synth.bases(50000, seed=5).tobytes(), unit * 4000, synth.bases(30000, seed=6).tobytes()]
    _check(gpu, genomes, 45, O.mask(45, 30, 0), "bottom", s)
    assert ctx.timings()["scan_launches"] > 1


def test_frac_wide_capacity_overflow_retry(gpu):
    """A homopolymer's 300 000 windows are one k-mer.  At c = 1 a genome's survivor
    region is capped at its length + 1, more than its windows, so that build
    cannot overflow (one scan launch, measured) and is only compared with the
    oracle.  At a c that divides the fmh of that k-mer (5 for this mask) all
    299 961 windows survive where 1/c were expected, the region of ~66 000
    overflows, and the genome is scanned again with the counted capacity: the
    launch count is asserted there."""
    _, ctx = gpu
    w = k = 40
    m = O.mask(w, k, 0)
    genomes = [b"A" * 300000, synth.bases(100000, seed=8).tobytes()]
    _check(gpu, genomes, w, m, "frac", 1)
    f = O.frac_min_hash(0, m, w)  # the canonical k-mer of A...A / T...T is 0
    c = next(d for d in range(2, 1000) if f % d == 0)
    sizes, _, _ = _check(gpu, genomes, w, m, "frac", c)
    assert int(sizes[0]) == 1
    assert ctx.timings()["scan_launches"] > 1


# ---- F. caller-made masks and the tag boundary ---------------------------------------------
@pytest.fixture(scope="module")
def mask_genomes():
    one = synth.bases(9000, seed=17)
    one[4000] = ord("N")
    five = [synth.bases(L, seed=950 + i).tobytes() for i, L in enumerate([0, 70, 3000, 5200, 9000])]
    return [one.tobytes()], five


@pytest.mark.parametrize("name,w,m", synth.caller_masks(), ids=[c[0] for c in synth.caller_masks()])
def test_caller_masks(gpu, mask_genomes, name, w, m):
    """Masks the seeded generator never makes (tests/test_oracle.py cross-checks
    the oracle on them against the reference-style port): the post-processing
    takes its sort widths and the tagged / segmented choice from the mask's
    words.  One genome (no tag) and five (one tagged device-wide sort)."""
    for genomes in mask_genomes:
        for flavour in (0, 1):
            _check(gpu, genomes, w, m, "frac", 1, flavour)
            _check(gpu, genomes, w, m, "bottom", 500, flavour)


@pytest.fixture(scope="module")
def tag_genomes():
    return [synth.bases(2900 + 7 * i, seed=1000 + i % 9, mut_seed=1100 + i, mut_rate=0.02 * (i % 3)).tobytes()
            for i in range(65)]


@pytest.mark.parametrize("n", [64, 65])
def test_tag_boundary_wide(gpu, tag_genomes, n):
    """w = 64, highest mask position 60: the high word's keys take 58 bits, so 64
    genomes (6 tag bits, 64 in all) sort tagged in one device-wide sort and 65
    (7 bits) take the segmented sorts."""
    m = synth.positions_mask(range(0, 61, 2))
    assert (m >> 64).bit_length() == 58
    _check(gpu, tag_genomes[:n], 64, m, "frac", 7)


@pytest.mark.parametrize("n", [64, 65])
def test_tag_boundary_narrow(gpu, tag_genomes, n):
    """w = 32, 29 positions (31 clear): packed keys take 58 bits, so 64 genomes
    sort tagged and 65 take the two stable passes for keys too wide for a tag."""
    m = synth.positions_mask(p for p in range(31) if p not in (7, 19))
    assert bin(m).count("1") == 58 and m >> 62 == 0
    _check(gpu, tag_genomes[:n], 32, m, "frac", 7)
