"""sks_sketch_set_downsample: a coarser copy of a device sketch set, made from
the set's own elements (FracMinHash 1/c -> 1/c', bottom-s -> bottom-s').

The result must be bit-identical to what sks_sketch_build gives for the same
bytes at the coarser parameter, so most tests compare against a direct build;
two compare against the rule itself, evaluated on the host with
sksffi.frac_min_hash over the source sketch's elements (independent of the
scan).  Sequences are synthetic (sks_synth_bases), segments separated by '\\n'.
The bottom-s tie rule (equal hashes of different k-mers) cannot be constructed
and is not tested."""
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
    """Segments of the given lengths (segment g from seed + g, or a (seed,
    mut_seed, rate) triple) in one device buffer, '\\n' after each."""

    def __init__(self, torch, ctx, lengths, seed=7, specs=None):
        self.ctx = ctx
        self.offs = [0]
        for L in lengths:
            self.offs.append(self.offs[-1] + L + 1)
        self.dev = torch.full((self.offs[-1],), ord("\n"), dtype=torch.uint8, device="cuda:0")
        for g, L in enumerate(lengths):
            s, ms, rate = specs[g] if specs else (seed + g, 0, 0.0)
            ctx.synth_bases(self.dev.data_ptr() + self.offs[g], L, s, ms, rate)
        torch.cuda.synchronize()

    def build(self, w, mask, kind, param, flavour=0):
        return self.ctx.sketch_build(self.dev.data_ptr(), self.offs[-1], self.offs, w, mask, kind, param,
                                     flavour=flavour)


def _same_sets(got, want):
    assert got.n == want.n and got.elem_words == want.elem_words
    assert np.array_equal(got.sizes(), want.sizes())
    assert np.array_equal(got.windows(), want.windows())
    assert np.array_equal(got.starts(), want.starts())
    for i in range(want.n):
        assert np.array_equal(got.sketch(i), want.sketch(i)), i


def _info_but_param(ss):
    i = ss.info()
    i.pop("param")
    return i


def _fmh(sketch, mask, w, flavour, nonce=1):
    """frac_min_hash of every element of a sketch ((size, 2) lo, hi), on the host."""
    return [sksffi.frac_min_hash(int(lo) | (int(hi) << 64), mask, w, nonce, flavour) for lo, hi in sketch]


def _lengths(w):
    return [40000, 5, 25000, 300, 33000, w]


@gpu_test
@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("shape", ["narrow", "wide"])
@pytest.mark.parametrize("kind,param,coarser", [(FRAC, 10, [10, 20, 50, 1000]), (BOTTOM, 512, [512, 400, 200, 1])])
def test_equals_direct_build(gpu, shape, flavour, kind, param, coarser):
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    G = Genomes(torch, ctx, _lengths(w))
    src = G.build(w, mask, kind, param, flavour)
    assert src.elem_words == (1 if shape == "narrow" else 2)
    assert src.sizes()[1] == 0 and src.windows()[5] == 1
    if kind == BOTTOM:
        assert src.sizes()[3] < 400  # the 300-base segment is kept whole at s' = 400
    for p in coarser:
        got = ctx.downsample(src, p)
        want = G.build(w, mask, kind, p, flavour)
        _same_sets(got, want)
        assert got.info()["param"] == p and want.info()["param"] == p
        assert _info_but_param(got) == _info_but_param(src)
        if kind == BOTTOM and p == 400:
            assert np.array_equal(got.sketch(3), src.sketch(3))


@gpu_test
@pytest.mark.parametrize("shape,flavour", [("narrow", 0), ("wide", 1)])
def test_host_hash_rule(gpu, shape, flavour):
    """The kept elements are exactly those with frac_min_hash % c' == 0, in order."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, _lengths(w)).build(w, mask, FRAC, 10, flavour)
    hashes = [np.array(_fmh(src.sketch(i), mask, w, flavour), dtype=object) for i in range(src.n)]
    for p in (20, 50, 1000):
        got = ctx.downsample(src, p)
        for i in range(src.n):
            keep = np.array([h % p == 0 for h in hashes[i]], dtype=bool)
            assert np.array_equal(got.sketch(i), src.sketch(i)[keep]), (p, i)
        assert got.sizes().sum() > 0


EDGE_N = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 20000]


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_chunk_edges(gpu, shape):
    """c = 1 keeps every window, so a segment of w - 1 + n bases gives a sketch of
    exactly n elements: sketch boundaries at, just before and just after every
    power-of-two chunk size, and one sketch spanning many workgroups."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [w - 1 + n for n in EDGE_N], seed=300).build(w, mask, FRAC, 1)
    # precondition: no duplicate masked k-mer within a segment
    assert src.sizes().tolist() == EDGE_N
    sk = [src.sketch(i) for i in range(src.n)]
    hashes = [np.array(_fmh(s, mask, w, 0), dtype=object) for s in sk]
    for p in (2, 3, 7):
        got = ctx.downsample(src, p)
        sizes = got.sizes()
        for i in range(src.n):
            keep = np.array([h % p == 0 for h in hashes[i]], dtype=bool)
            assert sizes[i] == keep.sum(), (p, i)
            assert np.array_equal(got.sketch(i), sk[i][keep]), (p, i)


@gpu_test
def test_large_multiples(gpu):
    """Parameters with 32 and more trailing zero bits (the divisibility test's high
    word) and the largest one: the host rule decides, nothing else is kept."""
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [30000, 2000], seed=40).build(w, mask, FRAC, 1)
    sk = [src.sketch(i) for i in range(src.n)]
    hashes = [_fmh(s, mask, w, 0) for s in sk]
    for p in (2**20, 2**32, 3 * 2**32, 5 * 2**40, 2**63, 2**64 - 1):
        got = ctx.downsample(src, p)
        assert got.info()["param"] == p
        for i in range(src.n):
            keep = np.array([h % p == 0 for h in hashes[i]], dtype=bool)
            assert np.array_equal(got.sketch(i), sk[i][keep]), (p, i)


@gpu_test
def test_many_small_sketches(gpu):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    G = Genomes(torch, ctx, [200] * 300, seed=1000)
    src = G.build(w, mask, FRAC, 2)
    got = ctx.downsample(src, 6)
    _same_sets(got, G.build(w, mask, FRAC, 6))
    assert 0 < got.sizes().sum() < src.sizes().sum()


@gpu_test
@pytest.mark.parametrize("kind,param,p", [(FRAC, 10, 50), (BOTTOM, 512, 200)])
def test_source_untouched_result_independent(gpu, kind, param, p):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    G = Genomes(torch, ctx, _lengths(w))
    src = G.build(w, mask, kind, param)
    before = [src.sketch(i).tobytes() for i in range(src.n)]
    sizes_before = src.sizes().copy()
    got = ctx.downsample(src, p)
    assert np.array_equal(src.sizes(), sizes_before) and src.info()["param"] == param
    assert [src.sketch(i).tobytes() for i in range(src.n)] == before
    src.free()
    _same_sets(got, G.build(w, mask, kind, p))


@gpu_test
def test_names_and_persistence(gpu, tmp_path):
    torch, ctx = gpu
    w, k = SHAPES["wide"]
    mask = sksffi.mask_generate(w, k, 0)
    G = Genomes(torch, ctx, _lengths(w))
    src = G.build(w, mask, FRAC, 10)
    assert ctx.downsample(src, 20).names() is None
    names = [f"genome {i}" for i in range(src.n)]
    src.set_names(names)
    got = ctx.downsample(src, 50)
    assert got.names() == names and got.info()["has_names"]
    path = tmp_path / "small.sks"
    got.save(path)
    back = ctx.load_sketches(path)
    _same_sets(back, got)
    assert back.info() == got.info() and back.info()["param"] == 50
    assert back.names() == names


@gpu_test
def test_search_across_scales(gpu):
    """Queries at 1/10 against references at 1/50: refused as they are, and after
    downsampling the queries the hits equal those of queries built at 1/50."""
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    rates = [0.0, 0.005, 0.01, 0.02, 0.03, 0.05]
    q_specs = [(100 + i % 4, 1000 + i, rates[i % 6]) for i in range(12)]
    r_specs = [(100 + (i + 1) % 5, 2000 + i, rates[(i + 2) % 6]) for i in range(20)]
    r_specs[3] = q_specs[0]
    QG = Genomes(torch, ctx, [20000 + 997 * i for i in range(12)], specs=q_specs)
    RG = Genomes(torch, ctx, [20000 + 613 * i for i in range(20)], specs=r_specs)
    Q, Q50 = QG.build(w, mask, FRAC, 10), QG.build(w, mask, FRAC, 50)
    R = RG.build(w, mask, FRAC, 50)
    with pytest.raises(sksffi.SksError, match="policy param") as e:
        ctx.search(Q, R)
    assert e.value.code == sksffi.SKS_E_ARG
    got = ctx.search(ctx.downsample(Q, 50), R)
    want = ctx.search(Q50, R)
    assert len(want) > 12 and len(np.unique(want["shared"])) > 5
    assert (want["containment"] == 1.0).any() and (want["containment"] < 1.0).any()
    for f in sksffi.HIT_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f


@gpu_test
def test_refusals(gpu):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    G = Genomes(torch, ctx, [3000, 2000])
    frac, bottom = G.build(w, mask, FRAC, 10), G.build(w, mask, BOTTOM, 64)
    lib = sksffi.lib()
    for ss, p, msg in [(frac, 15, b"policy param"), (frac, 5, b"policy param"), (frac, 0, b"param"),
                       (bottom, 0, b"param"), (bottom, 65, b"policy param")]:
        out = C.c_void_p(12345)
        assert lib.sks_sketch_set_downsample(ctx.h, ss.h, p, C.byref(out)) == sksffi.SKS_E_ARG, p
        assert out.value is None, p
        assert msg in lib.sks_last_error(), p
    with pytest.raises(sksffi.SksError, match="policy param") as e:
        ctx.downsample(frac, 15)
    assert e.value.code == sksffi.SKS_E_ARG
    assert lib.sks_sketch_set_downsample(ctx.h, frac.h, 20, None) == sksffi.SKS_E_ARG


def test_null_arguments_without_gpu():
    """Null arguments are refused before any device is touched."""
    lib = sksffi.lib()
    out = C.c_void_p(12345)
    assert lib.sks_sketch_set_downsample(None, None, 10, C.byref(out)) == 1
    assert b"null" in lib.sks_last_error()
    assert out.value is None
