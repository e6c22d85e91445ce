"""sks_sketch_set_merge: grouped unions of the sketches of device sketch sets.

An element is a masked canonical k-mer kept on its own hash, so the union of
the parts' sketches is the sketch of the parts taken together: most tests pin
the result bit for bit against sks_sketch_build of the same bytes with coarser
segment boundaries, the others against numpy's sorted unique of the members'
elements.  Sequences are synthetic (sks_synth_bases), segments separated by
'\\n' so that no window spans two parts."""
import ctypes as C

import numpy as np
import pytest

import sksffi

gpu_test = pytest.mark.gpu

FRAC, BOTTOM = sksffi.SKS_FRAC_MOD, sksffi.SKS_BOTTOM_S
SHAPES = {"narrow": (31, 21), "wide": (45, 30)}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.close()


class Genomes:
    """Segments of the given lengths in one device buffer, '\\n' after each:
    segment g from seed + g, or as specs[g] says, a (seed, mut_seed, rate) triple
    or a list of (length, seed, pos_offset) pieces laid end to end."""

    def __init__(self, torch, ctx, lengths, seed=7, specs=None):
        self.ctx = ctx
        self.offs = [0]
        for L in lengths:
            self.offs.append(self.offs[-1] + L + 1)
        self.dev = torch.full((self.offs[-1],), ord("\n"), dtype=torch.uint8, device="cuda:0")
        for g, L in enumerate(lengths):
            spec = specs[g] if specs else (seed + g, 0, 0.0)
            if isinstance(spec, list):
                at = self.offs[g]
                for n, s, pos in spec:
                    ctx.synth_bases(self.dev.data_ptr() + at, n, s, 0, 0.0, pos)
                    at += n
                assert at == self.offs[g] + L
            else:
                ctx.synth_bases(self.dev.data_ptr() + self.offs[g], L, *spec)
        torch.cuda.synchronize()

    def build(self, w, mask, kind, param, flavour=0, nonce=1, seg_off=None):
        return self.ctx.sketch_build(self.dev.data_ptr(), self.offs[-1], self.offs if seg_off is None else seg_off,
                                     w, mask, kind, param, nonce=nonce, flavour=flavour)

    def build_joined(self, groups, w, mask, kind, param, flavour=0):
        """One segment per group of consecutive segments (groups cover all, in order)."""
        cuts = [0]
        for g in groups:
            assert g == list(range(g[0], g[-1] + 1)) and self.offs[g[0]] == cuts[-1]
            cuts.append(self.offs[g[-1] + 1])
        assert cuts[-1] == self.offs[-1]
        return self.build(w, mask, kind, param, flavour, seg_off=cuts)


def _same_sets(got, want):
    assert got.n == want.n and got.elem_words == want.elem_words
    assert np.array_equal(got.sizes(), want.sizes())
    assert np.array_equal(got.windows(), want.windows())
    assert np.array_equal(got.starts(), want.starts())
    for i in range(want.n):
        assert np.array_equal(got.sketch(i), want.sketch(i)), i


def _union(parts):
    """np.unique of the concatenated (size, 2) = (lo, hi) sketches, ordered by (hi, lo)."""
    if not parts:
        return np.zeros((0, 2), dtype=np.uint64)
    rows = np.concatenate(parts)
    return np.unique(rows[:, ::-1], axis=0)[:, ::-1]


def _sources(sets):
    """(sketches, windows) of the source sketches in concat order."""
    return [s.sketch(i) for s in sets for i in range(s.n)], [int(x) for s in sets for x in s.windows()]


def _check_against_numpy(ctx, sets, groups):
    sk, win = _sources(sets)
    got = ctx.merge(sets, groups)
    assert got.n == len(groups) and got.names() is None
    sizes, windows, starts = got.sizes(), got.windows(), got.starts()
    at = 0
    for g, members in enumerate(groups):
        want = _union([sk[i] for i in members])
        assert sizes[g] == len(want) and starts[g] == at, (g, sizes[g], len(want))
        assert np.array_equal(got.sketch(g), want), g
        assert windows[g] == sum(win[i] for i in members), g
        at += len(want)
    return got, sk


JOIN_GROUPS = [[0, 1, 2], [3], [4, 5], [6, 7]]


def _join_lengths(w):
    return [40000, 5, 25000, 300, 33000, w, 20000, 15000]


def test_null_arguments_without_gpu():
    """Null arguments are refused before any device is touched."""
    lib = sksffi.lib()
    off = (C.c_uint32 * 2)(0, 0)
    one = (C.c_void_p * 1)(None)
    for ctx, sets in [(None, None), (None, one), (C.c_void_p(8), None)]:
        out = C.c_void_p(12345)
        assert lib.sks_sketch_set_merge(ctx, sets, 1, off, None, 1, C.byref(out)) == sksffi.SKS_E_ARG
        assert b"null" in lib.sks_last_error()
        assert out.value is None
    assert lib.sks_sketch_set_merge(None, None, 1, off, None, 1, None) == sksffi.SKS_E_ARG
    assert b"null" in lib.sks_last_error()


@gpu_test
@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("shape", ["narrow", "wide"])
@pytest.mark.parametrize("kind,param", [(FRAC, 10), (BOTTOM, 512)])
def test_equals_build_of_joined_segments(gpu, shape, flavour, kind, param):
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    G = Genomes(torch, ctx, _join_lengths(w))
    src = G.build(w, mask, kind, param, flavour)
    assert src.elem_words == (1 if shape == "narrow" else 2)
    assert src.sizes()[1] == 0 and src.windows()[5] == 1
    got = ctx.merge([src], JOIN_GROUPS)
    want = G.build_joined(JOIN_GROUPS, w, mask, kind, param, flavour)
    _same_sets(got, want)
    assert got.info() == want.info()
    if kind == BOTTOM:
        sizes = got.sizes().tolist()
        assert sizes[0] == 512 and sizes[2] == 512 and sizes[3] == 512  # cut
        assert 0 < sizes[1] < 512 and np.array_equal(got.sketch(1), src.sketch(3))  # kept whole


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_halo_chunks_equal_whole_genome(gpu, shape):
    """One genome cut into chunks that overlap by w - 1 bases: every window lies in
    exactly one chunk, so the chunks' merged sketch is the genome's.  The genome
    repeats itself (bases 36000.. are bases 12000..36000 again), so chunks share
    k-mers and the merge has real duplicates to drop."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    L, n_chunks, seed, fold, back = 60000, 5, 77, 36000, 24000

    def pieces(b, e):
        """Genome bases [b, e) as (length, seed, pos_offset) pieces of the seed's sequence."""
        if e <= fold:
            return [(e - b, seed, b)]
        if b >= fold:
            return [(e - b, seed, b - back)]
        return [(fold - b, seed, b), (e - fold, seed, fold - back)]

    whole = Genomes(torch, ctx, [L], specs=[pieces(0, L)])
    step = L // n_chunks
    begin = [i * step for i in range(n_chunks)]
    end = [min(b + step + w - 1, L) for b in begin]
    chunks = Genomes(torch, ctx, [e - b for b, e in zip(begin, end)], specs=[pieces(b, e) for b, e in zip(begin, end)])
    for i, (b, e) in enumerate(zip(begin, end)):  # the chunks are the genome's own bases
        assert torch.equal(chunks.dev[chunks.offs[i]:chunks.offs[i] + e - b], whole.dev[b:e])
    parts = chunks.build(w, mask, FRAC, 7)
    got = ctx.merge([parts], [list(range(n_chunks))])
    want = whole.build(w, mask, FRAC, 7)
    _same_sets(got, want)
    assert got.windows()[0] == L - w + 1 and int(parts.windows().sum()) == L - w + 1
    assert int(parts.sizes().sum()) > int(got.sizes()[0]) > 0  # real duplicates were dropped


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_host_union_arbitrary_groups(gpu, shape):
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    lengths = [20000, 15000, 5, 18000]
    sets = []
    for s, (n, rate) in enumerate([(4, 0.0), (4, 0.01), (3, 0.05)]):
        specs = [(50 + g, 900 + 10 * s + g if rate else 0, rate) for g in range(n)]
        sets.append(Genomes(torch, ctx, lengths[:n], specs=specs).build(w, mask, FRAC, 5))
    assert sets[0].sizes()[2] == 0 and sets[1].sizes()[2] == 0
    groups = [[0, 4, 8],                             # one genome's three versions, one per set
              [1, 5, 0],                             # source 0 again, in a second group
              [3, 3, 7],                             # a member twice
              [],                                    # no members
              [2, 6],                                # only empty sketches
              [10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]]    # everything, backwards
    got, sk = _check_against_numpy(ctx, sets, groups)
    sizes = got.sizes().tolist()
    assert 0 < sizes[0] < sum(len(sk[i]) for i in groups[0])
    assert sizes[0] > max(len(sk[i]) for i in groups[0])
    assert sizes[2] == len(_union([sk[3], sk[7]])) and sizes[3] == 0 and sizes[4] == 0
    # the order of the members does not matter
    again = ctx.merge(sets, [g[::-1] for g in groups])
    _same_sets(again, got)


EDGE_N = [1, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 20000]


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_tile_edges(gpu, shape):
    """c = 1 keeps every window, so a segment of w - 1 + n bases gives a sketch of
    exactly n elements: runs and unions that end at, just before and just after
    the tile size, a sketch merged with an identical copy (every element a
    duplicate, duplicates across every tile boundary), and 1 + 20000."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    lengths = [w - 1 + n for n in EDGE_N]
    a = Genomes(torch, ctx, lengths, seed=300).build(w, mask, FRAC, 1)
    b = Genomes(torch, ctx, lengths, seed=300).build(w, mask, FRAC, 1)
    # precondition: no duplicate masked k-mer within a segment
    assert a.sizes().tolist() == EDGE_N and b.sizes().tolist() == EDGE_N
    n = len(EDGE_N)
    groups = [[i, i + 1] for i in range(n - 1)] + [[i, n + i] for i in range(n)] + [[0, n - 1], [n - 1, 0]]
    got, _ = _check_against_numpy(ctx, [a, b], groups)
    assert got.sizes()[n - 1:2 * n - 1].tolist() == EDGE_N  # a sketch and its copy


@gpu_test
def test_many_members(gpu):
    """Groups of 33, 100, 9 and 1 members: an odd run is carried in several rounds."""
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [200] * 300, seed=1000).build(w, mask, FRAC, 2)
    groups = [list(range(0, 33)), list(range(33, 133)), list(range(133, 142)), [142]]
    got, _ = _check_against_numpy(ctx, [src], groups)
    assert got.sizes().min() > 0


def _fmh(sketch, mask, w, flavour, nonce=1):
    return [sksffi.frac_min_hash(int(lo) | (int(hi) << 64), mask, w, nonce, flavour) for lo, hi in sketch]


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_bottom_s_of_different_s(gpu, shape):
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    G1 = Genomes(torch, ctx, [30000, 20000], specs=[(60, 0, 0.0), (61, 0, 0.0)])
    G2 = Genomes(torch, ctx, [30000, 20000], specs=[(60, 700, 0.02), (61, 701, 0.05)])
    big, small = G1.build(w, mask, BOTTOM, 512), G2.build(w, mask, BOTTOM, 200)
    groups = [[0, 2], [1, 3], [0, 1, 2, 3], [3]]
    for sets in ([big, small], [small, big]):
        got = ctx.merge(sets, groups)
        assert got.info()["param"] == 200 and got.info()["kind"] == BOTTOM
        at200 = [G.build(w, mask, BOTTOM, 200) for G in ((G1, G2) if sets[0] is big else (G2, G1))]
        sk, win = _sources(at200)
        for g, members in enumerate(groups):
            union = _union([sk[i] for i in members])
            h = _fmh(union, mask, w, 0)
            order = sorted(range(len(union)), key=lambda i: (h[i], int(union[i, 1]), int(union[i, 0])))[:200]
            want = union[sorted(order)]
            assert len(want) == 200
            assert np.array_equal(got.sketch(g), want), g
            assert got.windows()[g] == sum(win[i] for i in members)
        _same_sets(got, ctx.merge(at200, groups))


@gpu_test
@pytest.mark.parametrize("kind,param", [(FRAC, 10), (BOTTOM, 512)])
def test_sources_untouched_and_freed(gpu, kind, param):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    G = Genomes(torch, ctx, _join_lengths(w))
    src = G.build(w, mask, kind, param)
    before = [src.sketch(i).tobytes() for i in range(src.n)]
    sizes_before = src.sizes().copy()
    got = ctx.merge([src], JOIN_GROUPS)
    assert np.array_equal(src.sizes(), sizes_before) and src.info()["param"] == param
    assert [src.sketch(i).tobytes() for i in range(src.n)] == before
    src.free()
    _same_sets(got, G.build_joined(JOIN_GROUPS, w, mask, kind, param))


@gpu_test
def test_persist_names_search(gpu, tmp_path):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    lengths = _join_lengths(w)
    r_specs = [(200 + g, 0, 0.0) for g in range(len(lengths))]
    RG = Genomes(torch, ctx, lengths, specs=r_specs)
    src = RG.build(w, mask, FRAC, 10)
    src.set_names([f"part {i}" for i in range(src.n)])
    merged = ctx.merge([src], JOIN_GROUPS)
    assert merged.names() is None and not merged.info()["has_names"]
    names = [f"genome {g}" for g in range(len(JOIN_GROUPS))]
    merged.set_names(names)
    path = tmp_path / "merged.sks"
    merged.save(path)
    back = ctx.load_sketches(path)
    _same_sets(back, merged)
    assert back.info() == merged.info() and back.names() == names
    # queries: mutated copies of parts 0, 2, 4 and 6, and an unrelated one
    q_specs = [(200, 31, 0.01), (202, 32, 0.03), (204, 33, 0.0), (206, 34, 0.05), (999, 0, 0.0)]
    Q = Genomes(torch, ctx, [lengths[0], lengths[2], lengths[4], lengths[6], 20000], specs=q_specs).build(
        w, mask, FRAC, 10)
    direct = RG.build_joined(JOIN_GROUPS, w, mask, FRAC, 10)
    got, want = ctx.search(Q, back), ctx.search(Q, direct)
    assert len(want) >= 4 and (want["containment"] < 1.0).any()
    for f in sksffi.HIT_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f


@gpu_test
def test_refusals(gpu):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    G = Genomes(torch, ctx, [3000, 2000])
    base = G.build(w, mask, FRAC, 10)
    lib = sksffi.lib()

    def raw(sets, n_sets, off, mem):
        arr = (C.c_void_p * max(len(sets), 1))(*[s.h for s in sets])
        goff = (C.c_uint32 * len(off))(*off)
        members = (C.c_uint32 * max(len(mem), 1))(*mem)
        out = C.c_void_p(12345)
        rc = lib.sks_sketch_set_merge(ctx.h, arr, n_sets, goff, members, len(off) - 1, C.byref(out))
        return rc, out.value, lib.sks_last_error()

    others = [
        (b"window", G.build(33, sksffi.mask_generate(33, k, 0), FRAC, 10)),
        (b"mask", G.build(w, sksffi.mask_generate(w, k, 1), FRAC, 10)),
        (b"policy kind", G.build(w, mask, BOTTOM, 10)),
        (b"flavour", G.build(w, mask, FRAC, 10, flavour=1)),
        (b"nonce", G.build(w, mask, FRAC, 10, nonce=2)),
        (b"policy param", G.build(w, mask, FRAC, 20)),
    ]
    assert sksffi.mask_generate(w, k, 1) != mask
    for field, other in others:
        for sets in ([base, other], [other, base]):
            rc, out, msg = raw(sets, 2, [0, 2], [0, 2])
            assert rc == sksffi.SKS_E_ARG and out is None, field
            assert field in msg, (field, msg)
    # a member index out of range, named in the message
    rc, out, msg = raw([base], 1, [0, 2], [1, 2])
    assert rc == sksffi.SKS_E_ARG and out is None and b"member index 2" in msg, msg
    rc, out, msg = raw([base, base], 2, [0, 1, 2], [3, 4])
    assert rc == sksffi.SKS_E_ARG and out is None and b"member index 4" in msg, msg
    # group_off that decreases, or does not start at 0
    rc, out, msg = raw([base], 1, [0, 2, 1], [0, 1])
    assert rc == sksffi.SKS_E_ARG and out is None and b"group_off" in msg, msg
    rc, out, msg = raw([base], 1, [1, 2], [0, 1])
    assert rc == sksffi.SKS_E_ARG and out is None and b"group_off" in msg, msg
    # no sets, a null set, null group_off / members
    rc, out, msg = raw([], 0, [0, 1], [0])
    assert rc == sksffi.SKS_E_ARG and out is None and b"no sets" in msg, msg
    out = C.c_void_p(12345)
    assert lib.sks_sketch_set_merge(ctx.h, (C.c_void_p * 1)(None), 1, (C.c_uint32 * 2)(0, 0), None, 1,
                                    C.byref(out)) == sksffi.SKS_E_ARG
    assert out.value is None and b"null" in lib.sks_last_error()
    arr = (C.c_void_p * 1)(base.h)
    out = C.c_void_p(12345)
    assert lib.sks_sketch_set_merge(ctx.h, arr, 1, None, None, 1, C.byref(out)) == sksffi.SKS_E_ARG
    assert out.value is None and b"null" in lib.sks_last_error()
    out = C.c_void_p(12345)
    assert lib.sks_sketch_set_merge(ctx.h, arr, 1, (C.c_uint32 * 2)(0, 1), None, 1, C.byref(out)) == sksffi.SKS_E_ARG
    assert out.value is None and b"null" in lib.sks_last_error()
    assert lib.sks_sketch_set_merge(ctx.h, arr, 1, (C.c_uint32 * 2)(0, 1), (C.c_uint32 * 1)(0), 1,
                                    None) == sksffi.SKS_E_ARG
    with pytest.raises(sksffi.SksError, match="member index 7") as e:
        ctx.merge([base], [[0], [7]])
    assert e.value.code == sksffi.SKS_E_ARG
    # what is allowed: no groups at all, and the plain case
    assert ctx.merge([base], []).n == 0
    assert ctx.merge([base, base], [[0, 2]]).sizes()[0] == base.sizes()[0]
