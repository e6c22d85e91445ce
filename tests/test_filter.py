"""sks_sketch_set_filter: every sketch of a device sketch set without (SUBTRACT)
or within (INTERSECT) a sketch of a second set.

The reference is numpy on host copies of the sketches: rows as (hi, lo),
membership by np.isin on a structured view, the kept rows in source order.
Sequences are synthetic (sks_synth_bases); c = 1 keeps every window, so a
segment of w - 1 + n bases gives a sketch of exactly n elements."""
import ctypes as C
import gc

import numpy as np
import pytest

import sksffi

gpu_test = pytest.mark.gpu

FRAC, BOTTOM = sksffi.SKS_FRAC_MOD, sksffi.SKS_BOTTOM_S
SUB, AND = sksffi.SKS_FILTER_SUBTRACT, sksffi.SKS_FILTER_INTERSECT
NONE = sksffi.FILTER_NONE
SHAPES = {"narrow": (31, 21), "wide": (45, 30)}
KINDS = {"subtract": SUB, "intersect": AND}
CHUNK = 1024               # kFilterChunk
STAGE_NARROW = 16384 // 8  # kFilterStageBytes (csrc/filter_plan.hpp) in narrow elements


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    # no sketch set of this module is left to a later garbage collection: freeing a
    # set waits for the device, which a later test may not expect in its middle
    gc.collect()
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

    def build(self, w, mask, kind, param, flavour=0, nonce=1):
        return self.ctx.sketch_build(self.dev.data_ptr(), self.offs[-1], self.offs, w, mask, kind, param,
                                     nonce=nonce, flavour=flavour)


ROW = np.dtype([("hi", "<u8"), ("lo", "<u8")])


def _rows(sketch):
    """A (size, 2) = (lo, hi) sketch as a structured (hi, lo) array."""
    out = np.empty(len(sketch), dtype=ROW)
    out["hi"], out["lo"] = sketch[:, 1], sketch[:, 0]
    return out


def _expected(src, filt, kind):
    """The rows of sketch `src` kept against sketch `filt` (None: no filter), in order."""
    if filt is None:
        return src
    found = np.isin(_rows(src), _rows(filt)) if len(src) and len(filt) else np.zeros(len(src), dtype=bool)
    return src[found != (kind == SUB)]


def _sketches(s):
    return [s.sketch(i) for i in range(s.n)]


def _check(ctx, src, filt, filter_of, kind, src_sk=None, filt_sk=None):
    """ctx.filter against numpy: sizes, starts, elements, windows and info.  Returns
    (result, its sketches)."""
    src_sk = _sketches(src) if src_sk is None else src_sk
    filt_sk = _sketches(filt) if filt_sk is None else filt_sk
    got = ctx.filter(src, filt, kind, filter_of)
    fo = [0] * src.n if filter_of is None else list(filter_of)
    assert got.n == src.n and got.elem_words == src.elem_words
    sizes, starts = got.sizes(), got.starts()
    out, at = [], 0
    for i in range(src.n):
        want = _expected(src_sk[i], None if fo[i] == NONE else filt_sk[fo[i]], kind)
        assert sizes[i] == len(want) and starts[i] == at, (i, sizes[i], len(want), starts[i], at)
        have = got.sketch(i)
        assert np.array_equal(have, want), i
        out.append(have)
        at += len(want)
    assert np.array_equal(got.windows(), src.windows())
    assert got.info() == src.info()
    return got, out


def _total(sk):
    return sum(len(s) for s in sk)


def _refusal(call):
    """(status, message) of the SksError `call` raises.  The exception is not kept: its
    traceback would hold the caller's frame, and with it every sketch set there, in a
    reference cycle until some later garbage collection."""
    try:
        call()
    except sksffi.SksError as err:
        return err.code, str(err)
    raise AssertionError("no SksError was raised")


@gpu_test
@pytest.mark.parametrize("kind", ["subtract", "intersect"])
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_against_numpy(gpu, shape, kind):
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [40000, 5, 25000, 300, 33000, w]).build(w, mask, FRAC, 10)
    # mutated copies of sources 0, 2 and 4, exact copies of sources 1 and 5, an unrelated genome
    f_specs = [(7, 900, 0.005), (8, 0, 0.0), (9, 901, 0.02), (12, 0, 0.0), (11, 902, 0.05), (500, 0, 0.0)]
    filt = Genomes(torch, ctx, [40000, 5, 25000, w, 33000, 20000], specs=f_specs).build(w, mask, FRAC, 10)
    assert src.elem_words == (1 if shape == "narrow" else 2)
    assert src.sizes()[1] == 0 and src.sizes()[0] > 3 * CHUNK
    filter_of = [0, 1, 2, NONE, 4, 3]
    src_sk = _sketches(src)
    got, out = _check(ctx, src, filt, filter_of, KINDS[kind], src_sk)
    kept = _total(out) - len(out[3])
    assert 0 < kept < _total(src_sk) - len(src_sk[3])  # some kept and some dropped
    assert out[3].tobytes() == src_sk[3].tobytes() and len(out[3]) > 0
    # the unrelated genome shares nothing
    other = ctx.filter(src, filt, KINDS[kind], [5] * 6)
    assert int(other.sizes().sum()) == (_total(src_sk) if kind == "subtract" else 0)


EDGE_N = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 5000]


@gpu_test
@pytest.mark.parametrize("kind", ["subtract", "intersect"])
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_chunk_edges(gpu, shape, kind):
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    lengths = [w - 1 + n for n in EDGE_N]
    src = Genomes(torch, ctx, lengths, seed=300).build(w, mask, FRAC, 1)
    assert src.sizes().tolist() == EDGE_N  # no duplicate masked k-mer within a segment
    f_specs = [(300 + g, 950 + g, 0.02) for g in range(len(EDGE_N))]
    filt = Genomes(torch, ctx, lengths, specs=f_specs).build(w, mask, FRAC, 1)
    src_sk = _sketches(src)
    got, out = _check(ctx, src, filt, list(range(len(EDGE_N))), KINDS[kind], src_sk)
    assert 0 < _total(out) < _total(src_sk)


@gpu_test
@pytest.mark.parametrize("shape,filter_bases", [("narrow", 2_000_000), ("wide", 500_000)])
def test_range_far_above_the_stage(gpu, shape, filter_bases):
    """A small sample against a large filter: every chunk brackets far more filter
    elements than the stage holds.  The filter's sequence contains the inner 20000
    bases of source 0 as a piece, so source 0's windows inside that piece are
    shared and those outside are not (the intersection is a proper part)."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [30000] * 3, specs=[[(30000, 40, 0)], (41, 0, 0.0), (42, 0, 0.0)]).build(
        w, mask, FRAC, 10)
    head = (filter_bases - 20000) // 2
    pieces = [(head, 900, 0), (20000, 40, 5000), (filter_bases - 20000 - head, 901, 0)]
    filt = Genomes(torch, ctx, [filter_bases], specs=[pieces]).build(w, mask, FRAC, 10)
    src_sk, filt_sk = _sketches(src), _sketches(filt)
    chunks = max((len(s) + CHUNK - 1) // CHUNK for s in src_sk)  # of one source: each spans the whole filter
    assert len(filt_sk[0]) / chunks > 4 * STAGE_NARROW
    for kind in (SUB, AND):
        got, out = _check(ctx, src, filt, [0, 0, 0], kind, src_sk, filt_sk)
        if kind == AND:
            assert 0 < len(out[0]) < len(src_sk[0]) and len(out[0]) > len(src_sk[0]) // 2
            assert len(out[1]) < 3 and len(out[2]) < 3  # unrelated: nearly empty


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_sparse_filter_dense_source(gpu, shape):
    """The reverse: most chunks of the long source bracket an empty range."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [2_000_000], specs=[[(2_000_000, 60, 0)]]).build(w, mask, FRAC, 10)
    filt = Genomes(torch, ctx, [3000], specs=[[(3000, 60, 1_000_000)]]).build(w, mask, FRAC, 10)
    src_sk, filt_sk = _sketches(src), _sketches(filt)
    assert len(src_sk[0]) > 100 * CHUNK and 0 < len(filt_sk[0]) < CHUNK
    for kind in (SUB, AND):
        got, out = _check(ctx, src, filt, None, kind, src_sk, filt_sk)
        if kind == AND:
            assert np.array_equal(out[0], filt_sk[0])  # the filter is a part of the source


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_one_element_filter(gpu, shape):
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [3000], specs=[[(3000, 70, 0)]]).build(w, mask, FRAC, 1)
    filt = Genomes(torch, ctx, [w], specs=[[(w, 70, 700)]]).build(w, mask, FRAC, 1)
    assert filt.sizes().tolist() == [1] and src.sizes().tolist() == [3000 - w + 1]
    src_sk, filt_sk = _sketches(src), _sketches(filt)
    got, out = _check(ctx, src, filt, [0], SUB, src_sk, filt_sk)
    assert got.sizes().tolist() == [3000 - w]
    got, out = _check(ctx, src, filt, [0], AND, src_sk, filt_sk)
    assert got.sizes().tolist() == [1] and np.array_equal(out[0], filt_sk[0])


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_self_and_empties(gpu, shape):
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [20000, 5, 3000, 1500]).build(w, mask, FRAC, 5)
    n = src.n
    src_sk = _sketches(src)
    assert src.sizes()[1] == 0 and src.sizes()[0] > CHUNK
    # the set against itself
    got, out = _check(ctx, src, src, list(range(n)), SUB, src_sk, src_sk)
    assert got.sizes().tolist() == [0] * n
    got, out = _check(ctx, src, src, list(range(n)), AND, src_sk, src_sk)
    assert [o.tobytes() for o in out] == [s.tobytes() for s in src_sk]
    assert np.array_equal(got.starts(), src.starts())
    # an empty filter sketch (sketch 1): SUBTRACT copies, INTERSECT empties; the empty source stays empty
    got, out = _check(ctx, src, src, [1] * n, SUB, src_sk, src_sk)
    assert [o.tobytes() for o in out] == [s.tobytes() for s in src_sk] and got.sizes()[1] == 0
    got, out = _check(ctx, src, src, [1] * n, AND, src_sk, src_sk)
    assert got.sizes().tolist() == [0] * n
    got, out = _check(ctx, src, src, [0, 0, 0, 0], AND, src_sk, src_sk)
    assert got.sizes()[1] == 0 and got.sizes()[0] == src.sizes()[0]
    # a set of no sketches
    none = ctx.merge([src], [])
    assert none.n == 0
    for kind in (SUB, AND):
        got = ctx.filter(none, src, kind, [])
        assert got.n == 0 and got.info() == none.info()


@gpu_test
def test_filter_of_none(gpu):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [20000, 15000, 300]).build(w, mask, FRAC, 5)
    two = Genomes(torch, ctx, [20000, 15000], specs=[(7, 77, 0.01), (8, 78, 0.03)]).build(w, mask, FRAC, 5)
    one = ctx.merge([two], [[0, 1]])
    assert one.n == 1
    for kind in (SUB, AND):
        a, out_a = _check(ctx, src, one, None, kind)
        b, out_b = _check(ctx, src, one, [0, 0, 0], kind)
        assert [o.tobytes() for o in out_a] == [o.tobytes() for o in out_b]
        assert 0 < _total(out_a) < int(src.sizes().sum())
        code, msg = _refusal(lambda: ctx.filter(src, two, kind, None))
        assert code == sksffi.SKS_E_ARG and "filter_of" in msg, msg


@gpu_test
@pytest.mark.parametrize("kind", ["subtract", "intersect"])
def test_many_small_sketches(gpu, kind):
    """300 one-chunk sketches with changing filters: the chunk-to-sketch map.  Filter
    j is the union of the 300 segments mutated at rate j's."""
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    n = 300
    src = Genomes(torch, ctx, [200] * n, seed=1000).build(w, mask, FRAC, 2)
    rates = [0.0, 0.002, 0.005, 0.01, 0.02, 0.04, 0.08]
    mutated = [Genomes(torch, ctx, [200] * n, specs=[(1000 + g, 2000 + 7 * g + j, r) for g in range(n)]).build(
        w, mask, FRAC, 2) for j, r in enumerate(rates)]
    filt = ctx.merge(mutated, [list(range(j * n, (j + 1) * n)) for j in range(7)])
    assert filt.n == 7 and src.sizes().min() > 0
    src_sk = _sketches(src)
    got, out = _check(ctx, src, filt, [i % 7 for i in range(n)], KINDS[kind], src_sk)
    assert 0 < _total(out) < _total(src_sk)


@gpu_test
def test_identities_with_existing_calls(gpu):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [40000, 5, 25000, 300]).build(w, mask, FRAC, 10)
    filt = Genomes(torch, ctx, [40000, 25000, 300], specs=[(7, 31, 0.01), (9, 32, 0.03), (600, 0, 0.0)]).build(
        w, mask, FRAC, 10)
    n, filter_of = src.n, [0, 2, 1, 2]
    S, I = ctx.subtract(src, filt, filter_of), ctx.intersect(src, filt, filter_of)
    # the two parts together are the source
    both = ctx.merge([S, I], [[i, n + i] for i in range(n)])
    assert np.array_equal(both.sizes(), src.sizes()) and np.array_equal(both.starts(), src.starts())
    for i in range(n):
        assert np.array_equal(both.sketch(i), src.sketch(i)), i
    assert 0 < int(I.sizes().sum()) < int(src.sizes().sum())
    # the intersection's sizes are the pair counts
    cat = ctx.concat([src, filt])
    data, starts, sizes = cat.device_ptrs()
    a = torch.arange(n, dtype=torch.int32, device="cuda:0")
    b = torch.tensor([n + f for f in filter_of], dtype=torch.int32, device="cuda:0")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    ctx.intersect_pairs(data, starts, sizes, cat.elem_words, a.data_ptr(), b.data_ptr(), n, counts.data_ptr())
    torch.cuda.synchronize()
    assert counts.cpu().numpy().tolist() == I.sizes().tolist()
    # gather: what its rounds leave unexplained is the query without the reported references
    n_ref = 20
    refs = Genomes(torch, ctx, [8000] * n_ref, seed=3000).build(w, mask, FRAC, 10)
    mix = [(4000, 3003, 1000), (4000, 3007, 0), (3000, 3012, 2000), (5000, 777, 0)]
    query = Genomes(torch, ctx, [16000], specs=[mix]).build(w, mask, FRAC, 10)
    hits, unexplained = ctx.gather(query, 0, refs, min_shared=1, max_rounds=0)
    assert {3, 7, 12} <= set(hits["ref"].tolist())
    assert 0 < unexplained < int(query.sizes()[0])
    reported = ctx.merge([refs], [[int(r) for r in hits["ref"]]])
    assert ctx.subtract(query, reported).sizes().tolist() == [unexplained]
    everything = ctx.merge([refs], [list(range(n_ref))])
    assert ctx.subtract(query, everything).sizes().tolist() == [unexplained]


@gpu_test
def test_refusals(gpu):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    G = Genomes(torch, ctx, [3000, 2000])
    base = G.build(w, mask, FRAC, 10)
    lib = sksffi.lib()

    def raw(src, filt, filter_of, kind):
        fo = None if filter_of is None else (C.c_uint32 * max(len(filter_of), 1))(*filter_of)
        out = C.c_void_p(12345)
        rc = lib.sks_sketch_set_filter(ctx.h, src.h, filt.h, fo, kind, C.byref(out))
        return rc, out.value, lib.sks_last_error()

    ww, wk = SHAPES["wide"]
    others = [
        ((b"window", b"mask"), G.build(ww, sksffi.mask_generate(ww, wk, 0), FRAC, 10)),
        ((b"policy param",), G.build(w, mask, FRAC, 20)),
        ((b"policy kind",), G.build(w, mask, BOTTOM, 10)),
        ((b"nonce",), G.build(w, mask, FRAC, 10, nonce=2)),
        ((b"flavour",), G.build(w, mask, FRAC, 10, flavour=1)),
    ]
    for fields, other in others:
        for src, filt in ((base, other), (other, base)):
            for kind in (SUB, AND):
                rc, out, msg = raw(src, filt, [0, 0], kind)
                assert rc == sksffi.SKS_E_ARG and out is None, fields
                assert any(f in msg for f in fields), (fields, msg)
    # two bottom-s sets that agree in everything
    bottom = G.build(w, mask, BOTTOM, 10)
    rc, out, msg = raw(bottom, bottom, [0, 1], SUB)
    assert rc == sksffi.SKS_E_ARG and out is None and b"policy kind" in msg, msg
    # a filter_of entry equal to the filters' number of sketches, named with its position
    rc, out, msg = raw(base, base, [0, 2], SUB)
    assert rc == sksffi.SKS_E_ARG and out is None and b"filter_of[1] = 2" in msg, msg
    code, msg = _refusal(lambda: ctx.filter(base, base, AND, [2, NONE]))
    assert code == sksffi.SKS_E_ARG and "filter_of[0] = 2" in msg, msg
    # an unknown kind
    for kind in (2, -1):
        rc, out, msg = raw(base, base, [0, 1], kind)
        assert rc == sksffi.SKS_E_ARG and out is None and b"kind" in msg, msg
    # what is allowed
    assert ctx.filter(base, base, SUB, [NONE, NONE]).sizes().tolist() == base.sizes().tolist()


@gpu_test
@pytest.mark.parametrize("kind", ["subtract", "intersect"])
def test_sources_untouched_result_independent(gpu, kind):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [40000, 5, 25000]).build(w, mask, FRAC, 10)
    filt = Genomes(torch, ctx, [40000, 25000], specs=[(7, 41, 0.01), (9, 42, 0.03)]).build(w, mask, FRAC, 10)
    src_sk, filt_sk = _sketches(src), _sketches(filt)
    before = [s.tobytes() for s in src_sk + filt_sk]
    sizes_before = (src.sizes().copy(), filt.sizes().copy())
    filter_of = [0, 1, 1]
    got = ctx.filter(src, filt, KINDS[kind], filter_of)
    assert np.array_equal(src.sizes(), sizes_before[0]) and np.array_equal(filt.sizes(), sizes_before[1])
    assert [s.tobytes() for s in _sketches(src) + _sketches(filt)] == before
    info, windows = src.info(), src.windows().copy()
    src.free()
    filt.free()
    assert got.info() == info and np.array_equal(got.windows(), windows)
    for i in range(3):
        assert np.array_equal(got.sketch(i), _expected(src_sk[i], filt_sk[filter_of[i]], KINDS[kind])), i
    assert 0 < int(got.sizes().sum()) < _total(src_sk)


@gpu_test
def test_names_and_persistence(gpu, tmp_path):
    torch, ctx = gpu
    w, k = SHAPES["wide"]
    mask = sksffi.mask_generate(w, k, 0)
    src = Genomes(torch, ctx, [20000, 300, 15000]).build(w, mask, FRAC, 10)
    filt = Genomes(torch, ctx, [20000], specs=[(7, 51, 0.02)]).build(w, mask, FRAC, 10)
    names = ["sample a", "sample b", "sample c"]
    src.set_names(names)
    filt.set_names(["host"])
    for kind in (SUB, AND):
        got, out = _check(ctx, src, filt, None, kind)
        assert got.names() == names and got.info()["has_names"]
        path = tmp_path / f"kept{kind}.sks"
        got.save(path)
        back = ctx.load_sketches(path)
        assert back.info() == got.info() == src.info() and back.names() == names
        assert np.array_equal(back.sizes(), got.sizes()) and np.array_equal(back.windows(), src.windows())
        for i in range(src.n):
            assert np.array_equal(back.sketch(i), out[i]), i
