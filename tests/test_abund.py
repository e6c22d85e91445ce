"""K-mer abundances: sks_sketch_build_counted, sks_sketch_set_abund_trim,
sks_sketch_set_abund_totals and sks_abund_pairs.

The abundance of an element is its multiplicity in the ordered k-mer list of its
segment, so every expected value comes from the CPU oracle's list
(pyoracle.kmer_list) through np.unique(return_counts=True), whose distinct rows
must be the oracle's sketch.  Everything is an integer and compared bit for bit.
Sequences are made on the host (synth.bases) and uploaded as bytes, segments
separated by '\\n' so that no window spans two."""
import ctypes as C

import numpy as np
import pytest

import pyoracle as O
import sksffi
import synth

gpu_test = pytest.mark.gpu

FRAC, BOTTOM = sksffi.SKS_FRAC_MOD, sksffi.SKS_BOTTOM_S
SHAPES = {"narrow": (31, 21), "wide": (45, 30)}
LIMITS = [(0, None), (1, 1), (2, None), (2, 3), (5, 2), (3000, None)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.close()


def revcomp(b):
    return bytes(b)[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def varied_segment():
    """One segment whose k-mers occur 1, 2, 3 and 4 times (one piece on the other
    strand) and, in the homopolymer and the dinucleotide repeat, thousands of times."""
    G = synth.bases(12000, 50).tobytes()
    return (G + G[1000:4000] + revcomp(G[2000:3500]) + G[2500:3000] + b"N" + b"A" * 3000 + G[5000:5400]
            + b"AC" * 1500)


class Segments:
    """Byte strings as the segments of one device buffer, '\\n' after each."""

    def __init__(self, torch, ctx, segs):
        self.ctx, self.segs = ctx, [bytes(s) for s in segs]
        self.offs = [0]
        for s in self.segs:
            self.offs.append(self.offs[-1] + len(s) + 1)
        host = b"".join(s + b"\n" for s in self.segs)
        self.dev = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()

    def plain(self, w, mask, c, flavour=0, kind=FRAC):
        return self.ctx.sketch_build(self.dev.data_ptr(), self.offs[-1], self.offs, w, mask, kind, c, flavour=flavour)

    def counted(self, w, mask, c, flavour=0, lo=1, hi=None, kind=FRAC):
        return self.ctx.sketch_build_counted(self.dev.data_ptr(), self.offs[-1], self.offs, w, mask, kind, c,
                                             flavour=flavour, min_abund=lo, max_abund=hi)

    def oracle(self, w, mask, c, flavour=0):
        """Per segment (elements (n, 2) = (lo, hi), abundances uint32, windows)."""
        out = []
        for s in self.segs:
            runs = O.cut_runs(s)
            rows = O.kmer_list(runs, w, mask, c, flavour=flavour).reshape(-1, 6)
            u, cnt = np.unique(rows[:, [3, 2]], axis=0, return_counts=True)
            want, nw = O.sketch(runs, w, mask, "frac", c, flavour=flavour)
            elems = np.ascontiguousarray(u[:, ::-1]).astype(np.uint64).reshape(-1, 2)
            assert np.array_equal(elems, want), "the list's distinct rows are the oracle's sketch"
            out.append((elems, cnt.astype(np.uint32), nw))
        return out


def _select(want, lo, hi):
    """numpy's selection from the oracle's counts by the keep rule."""
    out = []
    for elems, cnt, nw in want:
        keep = (cnt >= max(lo, 1)) & (cnt <= (0xFFFFFFFF if hi is None else hi))
        out.append((elems[keep], cnt[keep], nw))
    return out


def _check_counted(ss, want):
    assert ss.has_abund() == 1 and ss.n == len(want)
    sizes, windows, starts = ss.sizes(), ss.windows(), ss.starts()
    at = 0
    for g, (elems, cnt, nw) in enumerate(want):
        assert sizes[g] == len(elems) and starts[g] == at and windows[g] == nw, (g, sizes[g], len(elems))
        assert np.array_equal(ss.sketch(g), elems), g
        assert np.array_equal(ss.abund(g), cnt), g
        at += len(elems)
    totals = ss.abund_totals()
    assert totals.dtype == np.uint64
    assert totals.tolist() == [int(cnt.astype(np.uint64).sum()) for _, cnt, _ in want]


def _same_counted(got, want):
    assert got.has_abund() == 1 and want.has_abund() == 1
    assert got.n == want.n and got.info() == want.info()
    for f in ("sizes", "windows", "starts"):
        assert np.array_equal(getattr(got, f)(), getattr(want, f)()), f
    for i in range(want.n):
        assert np.array_equal(got.sketch(i), want.sketch(i)), i
        assert np.array_equal(got.abund(i), want.abund(i)), i


def _same_plain(got, want):
    assert got.n == want.n and got.elem_words == want.elem_words
    for f in ("sizes", "windows", "starts"):
        assert np.array_equal(getattr(got, f)(), getattr(want, f)()), f
    for i in range(want.n):
        assert np.array_equal(got.sketch(i), want.sketch(i)), i


def test_null_arguments_without_gpu():
    """Null arguments of every new entry point are refused before any device is touched."""
    lib = sksffi.lib()
    E = sksffi.SKS_E_ARG
    x = C.c_void_p(8)  # never dereferenced: a null argument is found first
    mask = (C.c_uint64 * 2)(3, 0)
    pol = sksffi.Policy(FRAC, 0, 1, 1)
    off = (C.c_uint64 * 2)(0, 0)
    for ctx, m, p, out_null in [(None, mask, C.byref(pol), False), (x, None, C.byref(pol), False),
                                (x, mask, None, False), (x, mask, C.byref(pol), True)]:
        out = C.c_void_p(12345)
        rc = lib.sks_sketch_build_counted(ctx, None, 0, off, 1, 1, m, p, 1, 0xFFFFFFFF,
                                          None if out_null else C.byref(out))
        assert rc == E and b"null" in lib.sks_last_error()
        assert out_null or out.value is None
    assert lib.sks_sketch_set_has_abund(None) == 0
    assert lib.sks_sketch_set_device_abund(None) is None
    buf = (C.c_uint64 * 1)()
    assert lib.sks_sketch_set_abund_copy(None, 0, buf) == E and b"null" in lib.sks_last_error()
    assert lib.sks_sketch_set_abund_totals(None, buf) == E and b"null" in lib.sks_last_error()
    for ctx, s, out_null in [(None, x, False), (x, None, False), (x, x, True)]:
        out = C.c_void_p(12345)
        rc = lib.sks_sketch_set_abund_trim(ctx, s, 1, 0xFFFFFFFF, None if out_null else C.byref(out))
        assert rc == E and b"null" in lib.sks_last_error()
        assert out_null or out.value is None
    for ctx, a, b in [(None, x, x), (x, None, x), (x, x, None)]:
        assert lib.sks_abund_pairs(ctx, a, b, None, None, 0, None, None) == E
        assert b"null" in lib.sks_last_error()


@gpu_test
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_counts_really_vary(gpu, shape):
    """A segment with repeats on both strands, a homopolymer and a dinucleotide
    repeat: the oracle's counts hold 1, 2, 3, 4 and a value >= 1000, and the
    device's elements and abundances are the oracle's, at c = 1 and c = 5, both flavours."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    S = Segments(torch, ctx, [varied_segment()])
    for flavour in (0, 1):
        for c in (1, 5):
            want = S.oracle(w, mask, c, flavour)
            values = set(want[0][1].tolist())
            print(shape, flavour, c, sorted((v, int((want[0][1] == v).sum())) for v in values))
            assert {1, 2, 3, 4} <= values
            if c == 1:
                assert max(values) >= 1000
            _check_counted(S.counted(w, mask, c, flavour), want)


def _with_repeats(g):
    g = g.tobytes()
    return g + g[len(g) // 3: len(g) // 2] + revcomp(g[: len(g) // 5])


ROUTES = [  # name, w, mask, segment lengths: every sort route of choose_post_path
    ("one_segment_segmented", 31, lambda: sksffi.mask_generate(31, 21, 0), [20000]),
    ("five_segments_tagged", 31, lambda: sksffi.mask_generate(31, 21, 0), [20000, 5, 15000, 30, 18000]),
    ("three_segments_two_pass", 32, lambda: sksffi.mask_contiguous(32), [9000, 31, 7000]),
    ("three_segments_wide_tagged", 45, lambda: sksffi.mask_generate(45, 30, 0), [9000, 44, 7000]),
    ("three_segments_wide_segmented", 64, lambda: sksffi.mask_contiguous(64), [9000, 63, 7000]),
    ("caller_mask", synth.caller_masks()[4][1], lambda: synth.caller_masks()[4][2], [9000, 4, 7000]),
]


@gpu_test
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_equals_the_plain_build(gpu, route):
    """min <= 1 and no limit: elements, sizes, starts and windows are the plain
    build's on every sort route, and the abundances are the oracle's."""
    torch, ctx = gpu
    _, w, mk, lengths = route
    mask = mk()
    S = Segments(torch, ctx, [_with_repeats(synth.bases(L, 60 + i)) if L >= 1000 else synth.bases(L, 60 + i).tobytes()
                              for i, L in enumerate(lengths)])
    c = 7
    for flavour in (0, 1):
        plain = S.plain(w, mask, c, flavour)
        want = S.oracle(w, mask, c, flavour)
        for lo in (0, 1):
            got = S.counted(w, mask, c, flavour, lo=lo)
            assert ctx.last_build_path() == 0  # SKS_BUILD_PATH_GENERAL
            assert got.info() == plain.info()
            _same_plain(got, plain)
            _check_counted(got, want)
        if len(lengths) > 1:
            assert 0 in plain.sizes().tolist()


@gpu_test
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_limits(gpu, shape):
    """The limited build equals numpy's selection from the oracle's counts and the
    trim of the unlimited build; a maximum below the minimum gives empty sketches."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    S = Segments(torch, ctx, [varied_segment(), b"ACGT", _with_repeats(synth.bases(6000, 71))])
    c = 1
    want = S.oracle(w, mask, c)
    full = S.counted(w, mask, c)
    for lo, hi in LIMITS:
        got = S.counted(w, mask, c, lo=lo, hi=hi)
        sel = _select(want, lo, hi)
        _check_counted(got, sel)
        _same_counted(ctx.abund_trim(full, lo, hi), got)
        if (lo, hi) == (5, 2):
            assert got.sizes().tolist() == [0, 0, 0]
        if (lo, hi) == (2, None):
            assert 0 < got.sizes()[0] < full.sizes()[0]
    assert np.array_equal(full.windows(), S.plain(w, mask, c).windows())


@gpu_test
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_second_scan_pass(gpu, shape):
    """A homopolymer whose one k-mer passes the FracMinHash test: every window
    survives, the record region overflows and the segment is scanned again; its
    abundances are placed next to those of the first pass's segments."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    c, n = 3, 40000
    assert O.frac_min_hash(0, mask, w, 1, 0) % c == 0, "precondition: the poly-A k-mer (0) is kept"
    S = Segments(torch, ctx, [_with_repeats(synth.bases(5000, 81)), b"A" * n, _with_repeats(synth.bases(7000, 82))])
    got = S.counted(w, mask, c)
    assert ctx.timings()["scan_launches"] >= 2
    want = S.oracle(w, mask, c)
    assert len(want[1][0]) == 1 and want[1][1].tolist() == [n - w + 1]
    assert got.sizes()[1] == 1 and got.abund(1).tolist() == [n - w + 1]
    _check_counted(got, want)
    _same_plain(got, S.plain(w, mask, c))
    _check_counted(S.counted(w, mask, c, lo=2), _select(want, 2, None))


@gpu_test
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_chunk_edges(gpu, shape):
    """Sketches of 1, 63, 64, 65, 1023, 1024, 1025 and 2049 elements whose first
    half has abundance 2: build, trim at (2, none) and (1, 1), totals."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    segs = []
    for i, n in enumerate([1, 63, 64, 65, 1023, 1024, 1025, 2049]):
        g = synth.bases(w - 1 + n, 90 + i).tobytes()
        segs.append(g + b"N" + g[: len(g) // 2])
    S = Segments(torch, ctx, segs)
    want = S.oracle(w, mask, 1)
    assert [len(e) for e, _, _ in want] == [1, 63, 64, 65, 1023, 1024, 1025, 2049]
    assert all(set(cnt.tolist()) <= {1, 2} for _, cnt, _ in want) and 2 in want[-1][1].tolist()
    full = S.counted(w, mask, 1)
    _check_counted(full, want)
    for lo, hi in ((2, None), (1, 1)):
        sel = _select(want, lo, hi)
        _check_counted(S.counted(w, mask, 1, lo=lo, hi=hi), sel)
        _check_counted(ctx.abund_trim(full, lo, hi), sel)


def _rows(sketch):
    return set(map(tuple, sketch.tolist()))


@gpu_test
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_weighted_pairs(gpu, shape):
    """shared and weight of 5000 shuffled pairs, duplicates included, against
    numpy on the sketches' rows; shared also against sks_intersect_pairs."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    c = 2
    G, H = synth.bases(12000, 50).tobytes(), synth.bases(30000, 51).tobytes()
    sample_segs = [varied_segment(), H + H[5000:9000] + revcomp(H[100:2100]), synth.bases(300, 52).tobytes(), b""]
    ref_segs = [G[:3000], synth.bases(12000, 50, mut_seed=9, mut_rate=0.02).tobytes(),
                G + H + synth.bases(60000, 53).tobytes(), b"", H[10000:20000], synth.bases(300, 52).tobytes()[:200]]
    SS, RS = Segments(torch, ctx, sample_segs), Segments(torch, ctx, ref_segs)
    samples, refs = SS.counted(w, mask, c), RS.plain(w, mask, c)
    sizes_s, sizes_r = samples.sizes().tolist(), refs.sizes().tolist()
    assert sizes_s[3] == 0 and sizes_r[3] == 0
    assert sizes_r[2] > 20 * sizes_s[2] > 0 and sizes_s[0] > 3 * sizes_r[0] > 0  # both walking directions

    def expect(aset, bset, pairs):
        a_rows = [aset.sketch(i).tolist() for i in range(aset.n)]
        a_ab = [aset.abund(i).astype(np.uint64) for i in range(aset.n)]
        b_rows = [_rows(bset.sketch(j)) for j in range(bset.n)]
        table = {}
        for i in range(aset.n):
            for j in range(bset.n):
                hit = np.array([tuple(r) in b_rows[j] for r in a_rows[i]], dtype=bool)
                table[(i, j)] = (int(hit.sum()), int(a_ab[i][hit].sum()) if len(hit) else 0)
        return (np.array([table[p][0] for p in pairs], dtype=np.int32),
                np.array([table[p][1] for p in pairs], dtype=np.uint64), table)

    rng = np.random.default_rng(5)
    for aset, bset in ((samples, refs), (samples, samples)):
        combos = [(i, j) for i in range(aset.n) for j in range(bset.n)]
        order = list(rng.permutation(len(combos))) + list(rng.integers(0, len(combos), 7))
        pairs = [combos[i] for i in order]
        pairs = (pairs * (5000 // len(pairs) + 1))[:5000]
        want_shared, want_weight, table = expect(aset, bset, pairs)
        a = np.array([p[0] for p in pairs], dtype=np.int32)
        b = np.array([p[1] for p in pairs], dtype=np.int32)
        shared, weight = ctx.abund_pairs(aset, bset, a, b)
        assert shared.dtype == np.int32 and weight.dtype == np.uint64
        assert np.array_equal(shared, want_shared)
        assert np.array_equal(weight, want_weight)
        assert any(v[1] > v[0] > 0 for v in table.values())  # a weight that is not just the count
        # sks_intersect_pairs over one set holding both sides
        both = aset if bset is aset else ctx.concat([SS.plain(w, mask, c), bset])
        shift = 0 if bset is aset else aset.n
        d_a = torch.from_numpy(a).to("cuda:0")
        d_b = torch.from_numpy(b + shift).to("cuda:0")
        d_out = torch.zeros(len(pairs), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        data, starts, szs = both.device_ptrs()
        ctx.intersect_pairs(data, starts, szs, both.elem_words, d_a.data_ptr(), d_b.data_ptr(), len(pairs),
                            d_out.data_ptr())
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), shared)
    # no pairs; one index out of range on either side
    shared, weight = ctx.abund_pairs(samples, refs, [], [])
    assert len(shared) == 0 and len(weight) == 0
    shared, weight = ctx.abund_pairs(samples, refs, [0, samples.n, 1, 0], [1, 0, refs.n, 0])
    _, _, table = expect(samples, refs, [])
    assert shared.tolist() == [table[(0, 1)][0], -1, -1, table[(0, 0)][0]]
    assert weight.tolist() == [table[(0, 1)][1], 0, 0, table[(0, 0)][1]]


@gpu_test
def test_rules(gpu):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    c = 4
    S = Segments(torch, ctx, [_with_repeats(synth.bases(6000, 31)), _with_repeats(synth.bases(4000, 32))])
    T = Segments(torch, ctx, [_with_repeats(synth.bases(5000, 33))])
    counted, plain = S.counted(w, mask, c), S.plain(w, mask, c)
    # bottom-s cannot count
    with pytest.raises(sksffi.SksError, match="policy kind") as e:
        S.counted(w, mask, 100, kind=BOTTOM)
    assert e.value.code == sksffi.SKS_E_UNSUPPORTED
    # a set without abundances
    assert plain.has_abund() == 0
    for call in (lambda: ctx.abund_trim(plain, 2), lambda: ctx.abund_pairs(plain, counted, [0], [0]),
                 lambda: plain.abund(0), lambda: plain.abund_totals()):
        with pytest.raises(sksffi.SksError, match="abundance") as e:
            call()
        assert e.value.code == sksffi.SKS_E_ARG
    # refs need none
    shared, _ = ctx.abund_pairs(counted, plain, [0, 1], [0, 1])
    assert shared.tolist() == plain.sizes().tolist()
    # mismatched sets name the field
    other_w = T.plain(29, sksffi.mask_generate(29, 21, 0), c)
    other_mask = T.plain(w, sksffi.mask_generate(w, k, 1), c)
    other_c = T.plain(w, mask, c + 1)
    for refs, field in ((other_w, "window"), (other_mask, "mask"), (other_c, "param")):
        with pytest.raises(sksffi.SksError, match=field) as e:
            ctx.abund_pairs(counted, refs, [0], [0])
        assert e.value.code == sksffi.SKS_E_ARG
    # concat: all or none
    with pytest.raises(sksffi.SksError, match="abundance") as e:
        ctx.concat([counted, T.plain(w, mask, c)])
    assert e.value.code == sksffi.SKS_E_ARG
    tc = T.counted(w, mask, c)
    cat = ctx.concat([counted, tc])
    assert cat.has_abund() == 1 and cat.n == 3
    for i, (src, j) in enumerate([(counted, 0), (counted, 1), (tc, 0)]):
        assert np.array_equal(cat.sketch(i), src.sketch(j)) and np.array_equal(cat.abund(i), src.abund(j))
    assert ctx.concat([plain, T.plain(w, mask, c)]).has_abund() == 0
    # every other set-producing call takes a counted set and returns a plain one
    for call in (lambda s: ctx.downsample(s, 2 * c), lambda s: ctx.merge([s], [[0, 1], [1]]),
                 lambda s: ctx.subtract(s, s, [1, sksffi.FILTER_NONE]), lambda s: ctx.tally([s], [[0, 1]], 1, 1)):
        got, want = call(counted), call(plain)
        assert got.has_abund() == 0
        _same_plain(got, want)
