"""sks_sketch_set_tally: per group of source sketches, the k-mers held by
min_count .. max_count of the listed members, and by how many.

The reference is numpy: np.unique(return_counts=True) over the members'
concatenated sketches, on the (hi, lo) order for wide elements; the identities
pin the call against merge, intersect and subtract.  Everything is compared bit
for bit.  Sequences are synthetic (sks_synth_bases), mutated copies of the same
genomes so that the counts really vary."""
import ctypes as C

import numpy as np
import pytest

import sksffi
from test_merge import EDGE_N, SHAPES, Genomes, _same_sets, _sources, gpu  # noqa: F401

gpu_test = pytest.mark.gpu

FRAC, BOTTOM = sksffi.SKS_FRAC_MOD, sksffi.SKS_BOTTOM_S
NO_LIMIT = sksffi.TALLY_NO_LIMIT


def _counted(parts):
    """(values, counts): the distinct rows of the concatenated (size, 2) = (lo, hi)
    sketches, ordered by (hi, lo), and how many of the parts' rows equal each."""
    if sum(len(p) for p in parts) == 0:
        return np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    rows = np.concatenate(parts)
    u, cnt = np.unique(rows[:, ::-1], axis=0, return_counts=True)
    return u[:, ::-1], cnt.astype(np.uint32)


def _within(counted, lo, hi):
    u, cnt = counted
    hi = NO_LIMIT if hi is None else hi
    keep = (cnt >= max(1 if lo is None else lo, 1)) & (cnt <= hi)
    return u[keep], cnt[keep]


def _per_group(v, g):
    return v if v is None or np.isscalar(v) else v[g]


def _check(ctx, sets, groups, lo, hi, counted, win=None):
    """Context.tally with counts against the reference; lo / hi: None, a scalar or
    one value per group.  counted[g] = _counted of group g's members."""
    got, mult = ctx.tally(sets, groups, lo, hi, counts=True)
    assert got.n == len(groups) and got.names() is None
    sizes, starts, windows = got.sizes(), got.starts(), got.windows()
    at = 0
    for g in range(len(groups)):
        want, cnt = _within(counted[g], _per_group(lo, g), _per_group(hi, g))
        assert sizes[g] == len(want) and starts[g] == at, (g, lo, hi, sizes[g], len(want))
        assert np.array_equal(got.sketch(g), want), (g, lo, hi)
        assert np.array_equal(mult[at:at + len(want)], cnt), (g, lo, hi)
        if win is not None:
            assert windows[g] == sum(win[i] for i in groups[g]), g
        at += len(want)
    assert len(mult) == at
    # without d_counts: the same set
    _same_sets(ctx.tally(sets, groups, lo, hi), got)
    return got


def _raw(lib, ctx, sets, n_sets, off, mem, lo=None, hi=None, d_counts=None, cap=0):
    arr = (C.c_void_p * max(len(sets), 1))(*[s.h for s in sets])
    goff = (C.c_uint32 * len(off))(*off)
    members = (C.c_uint32 * max(len(mem), 1))(*mem)
    lo = None if lo is None else (C.c_uint32 * len(lo))(*lo)
    hi = None if hi is None else (C.c_uint32 * len(hi))(*hi)
    out = C.c_void_p(12345)
    rc = lib.sks_sketch_set_tally(ctx.h, arr, n_sets, goff, members, len(off) - 1, lo, hi, C.byref(out),
                                  d_counts, cap)
    return rc, out.value, lib.sks_last_error()


def test_null_arguments_without_gpu():
    """Null arguments are refused before any device is touched."""
    lib = sksffi.lib()
    off = (C.c_uint32 * 2)(0, 0)
    one = (C.c_void_p * 1)(None)
    for ctx, sets in [(None, None), (None, one), (C.c_void_p(8), None)]:
        out = C.c_void_p(12345)
        assert lib.sks_sketch_set_tally(ctx, sets, 1, off, None, 1, None, None, C.byref(out), None,
                                        0) == sksffi.SKS_E_ARG
        assert b"null" in lib.sks_last_error() and b"sks_sketch_set_tally" in lib.sks_last_error()
        assert out.value is None
    assert lib.sks_sketch_set_tally(None, None, 1, off, None, 1, None, None, None, None, 0) == sksffi.SKS_E_ARG
    assert b"null" in lib.sks_last_error()


def _three_sets(torch, ctx, w, mask):
    """Three sets of 4, 4 and 3 sketches: the same genomes at 0, 1 and 5 % substitutions."""
    lengths = [20000, 15000, 5, 18000]
    sets = []
    for s, (n, rate) in enumerate([(4, 0.0), (4, 0.01), (3, 0.05)]):
        specs = [(50 + g, 900 + 10 * s + g if rate else 0, rate) for g in range(n)]
        sets.append(Genomes(torch, ctx, lengths[:n], specs=specs).build(w, mask, FRAC, 5))
    assert sets[0].sizes()[2] == 0 and sets[1].sizes()[2] == 0
    return sets


GROUPS = [[0, 4, 8],                             # one genome's three versions, one per set
          [1, 5, 0, 9, 4],                       # two genomes' versions mixed
          [3, 3, 7],                             # a member twice
          [],                                    # no members
          [2, 6],                                # only empty sketches
          [10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]]    # everything, backwards


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_against_numpy_arbitrary_groups(gpu, shape):
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    sets = _three_sets(torch, ctx, w, mask)
    sk, win = _sources(sets)
    counted = [_counted([sk[i] for i in g]) for g in GROUPS]
    # the counts really vary: group 0 has values held by 1, 2 and 3 members, group 2 by 1, 2 and 3
    assert set(counted[0][1].tolist()) == {1, 2, 3} and set(counted[2][1].tolist()) == {1, 2, 3}
    m = [len(g) for g in GROUPS]
    lows = {"1": lambda n: 1, "2": lambda n: 2, "m-1": lambda n: max(n - 1, 0), "m": lambda n: n,
            "m+1": lambda n: n + 1}
    highs = {"1": lambda n: 1, "m-1": lambda n: max(n - 1, 0), "m": lambda n: n, "NULL": None,
             "max": lambda n: NO_LIMIT}
    for lo_of in lows.values():
        for hi_of in highs.values():
            lo = [lo_of(n) for n in m]
            hi = None if hi_of is None else [hi_of(n) for n in m]
            got = _check(ctx, sets, GROUPS, lo, hi, counted, win)
            assert got.info() == {**sets[0].info(), "n": len(GROUPS), "has_names": False}
    # min_count NULL is 1 everywhere; 0 is 1 too; scalars
    _same_sets(_check(ctx, sets, GROUPS, None, None, counted, win), ctx.tally(sets, GROUPS, 1))
    _check(ctx, sets, GROUPS, 0, NO_LIMIT, counted, win)
    _check(ctx, sets, GROUPS, None, 2, counted, win)
    _check(ctx, sets, GROUPS, 2, None, counted, win)
    # something is kept and something dropped by each side of the limits
    got = ctx.tally(sets, GROUPS, 2, 2)
    union = ctx.tally(sets, GROUPS)
    assert 0 < got.sizes()[0] < union.sizes()[0] and got.sizes()[3] == 0 and got.sizes()[4] == 0
    # the order of the members does not matter
    back = [g[::-1] for g in GROUPS]
    a, ma = ctx.tally(sets, GROUPS, 2, 3, counts=True)
    b, mb = ctx.tally(sets, back, 2, 3, counts=True)
    _same_sets(a, b)
    assert np.array_equal(ma, mb)
    # core(): ceil(fraction * members), at least 1
    _same_sets(ctx.core(sets, GROUPS, 0.9), ctx.tally(sets, GROUPS, [3, 5, 3, 1, 2, 10]))
    _same_sets(ctx.core(sets, GROUPS, 0.5), ctx.tally(sets, GROUPS, [2, 3, 2, 1, 1, 6]))


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_identities_with_merge_and_filter(gpu, shape):
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    sets = _three_sets(torch, ctx, w, mask)
    # min 1, no max: the merge, windows included
    _same_sets(ctx.tally(sets, GROUPS), ctx.merge(sets, GROUPS))
    _same_sets(ctx.tally(sets, GROUPS, 1, NO_LIMIT), ctx.merge(sets, GROUPS))
    # pairs [a, b]: (2, 2) is the intersection, (1, 1) the two differences together
    a, b = sets[0], sets[1]
    n = a.n
    pairs = [[i, n + i] for i in range(n)]
    same = list(range(n))
    both = ctx.tally([a, b], pairs, 2, 2)
    inter = ctx.intersect(a, b, same)
    assert both.sizes().max() > 0
    assert np.array_equal(both.sizes(), inter.sizes())
    for i in range(n):
        assert np.array_equal(both.sketch(i), inter.sketch(i)), i
    one = ctx.tally([a, b], pairs, 1, 1)
    diff = ctx.merge([ctx.subtract(a, b, same), ctx.subtract(b, a, same)], pairs)
    assert one.sizes().max() > 0
    assert np.array_equal(one.sizes(), diff.sizes())
    for i in range(n):
        assert np.array_equal(one.sketch(i), diff.sketch(i)), i


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_chunk_edges(gpu, shape):
    """c = 1 keeps every window, so a segment of w - 1 + n bases gives a sketch of
    exactly n elements.  Each is grouped with one and with two identical copies:
    runs of 2 and of 3 equal values lie across every chunk boundary at every
    offset the lengths allow; every lo, hi in 1..4."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    lengths = [w - 1 + n for n in EDGE_N]
    abc = [Genomes(torch, ctx, lengths, seed=300).build(w, mask, FRAC, 1) for _ in range(3)]
    assert all(s.sizes().tolist() == EDGE_N for s in abc)  # no duplicate masked k-mer within a segment
    n = len(EDGE_N)
    groups = [[i, n + i] for i in range(n)] + [[i, n + i, 2 * n + i] for i in range(n)]
    sk, _ = _sources(abc)
    counted = [_counted([sk[i] for i in g]) for g in groups]
    assert all(len(c[0]) == EDGE_N[g % n] and (c[1] == len(groups[g])).all() for g, c in enumerate(counted))
    for lo in range(1, 5):
        for hi in range(1, 5):
            got = _check(ctx, abc, groups, lo, hi, counted)
            pairs_kept, triples_kept = lo <= 2 <= hi, lo <= 3 <= hi
            assert got.sizes()[:n].tolist() == [v if pairs_kept else 0 for v in EDGE_N]
            assert got.sizes()[n:].tolist() == [v if triples_kept else 0 for v in EDGE_N]


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_runs_longer_than_a_chunk(gpu, shape):
    """1100 copies of one 3-element sketch: three runs of 1100 equal values over the
    1024-element chunk boundaries, the threshold reads a whole chunk ahead."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    m = 1100
    src = Genomes(torch, ctx, [w + 2] * m, specs=[(77, 0, 0.0)] * m).build(w, mask, FRAC, 1)
    assert src.sizes().tolist() == [3] * m
    one = src.sketch(0)
    everyone = list(range(m))
    groups = [everyone] * 6
    lo = [m, m + 1, 1, 1, 1, m]
    hi = [NO_LIMIT, NO_LIMIT, m - 1, m, NO_LIMIT, m]
    got, mult = ctx.tally([src], groups, lo, hi, counts=True)
    assert got.sizes().tolist() == [3, 0, 0, 3, 3, 3]
    for g in (0, 3, 4, 5):
        assert np.array_equal(got.sketch(g), one), g
    assert mult.tolist() == [m] * 12
    assert got.windows().tolist() == [3 * m] * 6
    _same_sets(ctx.tally([src], groups, lo, hi), got)
    # max_count alone (min_count NULL)
    assert ctx.tally([src], groups[:2], None, [m - 1, m]).sizes().tolist() == [0, 3]


@gpu_test
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_bounds_are_the_groups_own(gpu, shape):
    """What lies behind a group's run (the next group's run in the scratch column,
    the next sketch of the source set) is not counted, whatever it holds."""
    torch, ctx = gpu
    w, k = SHAPES[shape]
    mask = sksffi.mask_generate(w, k, 0)
    sets = _three_sets(torch, ctx, w, mask)
    members = [0, 4, 8]
    m = len(members)
    twice = [members, members]
    union = ctx.merge(sets, twice)
    assert union.sizes()[0] > 0
    assert ctx.tally(sets, twice, m + 1).sizes().tolist() == [0, 0]
    _same_sets(ctx.tally(sets, twice, None, m), union)
    # two identical segments of exactly w bases: one-element sketches side by side in the source set
    src = Genomes(torch, ctx, [w, w, w], specs=[(91, 0, 0.0)] * 3).build(w, mask, FRAC, 1)
    assert src.sizes().tolist() == [1, 1, 1]
    x = src.sketch(0)
    assert np.array_equal(src.sketch(1), x) and np.array_equal(src.sketch(2), x)
    assert ctx.tally([src], [[0]], 2).sizes().tolist() == [0]
    got, mult = ctx.tally([src], [[0]], None, 1, counts=True)
    assert got.sizes().tolist() == [1] and np.array_equal(got.sketch(0), x) and mult.tolist() == [1]
    got, mult = ctx.tally([src], [[0], [1], [2]], 1, 1, counts=True)
    assert got.sizes().tolist() == [1, 1, 1] and mult.tolist() == [1, 1, 1]
    # and the same value in consecutive merged runs: [x, x] [x, x]
    assert ctx.tally([src], [[0, 1], [1, 2]], 3).sizes().tolist() == [0, 0]
    got, mult = ctx.tally([src], [[0, 1], [1, 2]], None, 2, counts=True)
    assert got.sizes().tolist() == [1, 1] and mult.tolist() == [2, 2]
    assert ctx.tally([src], [[0, 1], [1, 2]], 1, 1).sizes().tolist() == [0, 0]


@gpu_test
def test_counts_capacity(gpu):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    sets = _three_sets(torch, ctx, w, mask)
    lib = sksffi.lib()
    off, mem = [0, 3, 5], [0, 4, 8, 1, 5]
    want, want_mult = ctx.tally(sets, [[0, 4, 8], [1, 5]], 2, counts=True)
    total = int(want.sizes().sum())
    assert total > 0
    buf = torch.zeros(total, dtype=torch.int32, device="cuda:0")
    rc, out, msg = _raw(lib, ctx, sets, 3, off, mem, [2, 2], None, C.c_void_p(buf.data_ptr()), total - 1)
    assert rc == sksffi.SKS_E_LENGTH and out is None and b"d_counts" in msg, msg
    rc, out, msg = _raw(lib, ctx, sets, 3, off, mem, [2, 2], None, C.c_void_p(buf.data_ptr()), total)
    assert rc == sksffi.SKS_OK and out is not None
    got = sksffi.SketchSet(C.c_void_p(out))
    ctx.synchronize()
    _same_sets(got, want)
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), want_mult)
    # without d_counts the capacity is not looked at
    rc, out, msg = _raw(lib, ctx, sets, 3, off, mem, [2, 2], None, None, 0)
    assert rc == sksffi.SKS_OK
    _same_sets(sksffi.SketchSet(C.c_void_p(out)), want)


@gpu_test
def test_refusals(gpu):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    G = Genomes(torch, ctx, [3000, 2000])
    base = G.build(w, mask, FRAC, 10)
    lib = sksffi.lib()

    def raw(sets, n_sets, off, mem):
        return _raw(lib, ctx, sets, n_sets, off, mem)

    bottom = G.build(w, mask, BOTTOM, 10)
    others = [
        (b"window", G.build(33, sksffi.mask_generate(33, k, 0), FRAC, 10)),
        (b"mask", G.build(w, sksffi.mask_generate(w, k, 1), FRAC, 10)),
        (b"policy kind", bottom),
        (b"flavour", G.build(w, mask, FRAC, 10, flavour=1)),
        (b"nonce", G.build(w, mask, FRAC, 10, nonce=2)),
        (b"policy param", G.build(w, mask, FRAC, 20)),
    ]
    for field, other in others:
        for sets in ([base, other], [other, base]):
            rc, out, msg = raw(sets, 2, [0, 2], [0, 2])
            assert rc == sksffi.SKS_E_ARG and out is None, field
            assert field in msg and b"sks_sketch_set_tally" in msg, (field, msg)
    # bottom-s sets only: refused too, naming the policy kind
    for sets, n in (([bottom], 1), ([bottom, bottom], 2)):
        rc, out, msg = raw(sets, n, [0, 1], [0])
        assert rc == sksffi.SKS_E_ARG and out is None and b"policy kind" in msg, msg
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
    # no sets, a null set, null group_off / members / out
    rc, out, msg = raw([], 0, [0, 1], [0])
    assert rc == sksffi.SKS_E_ARG and out is None and b"no sets" in msg, msg
    out = C.c_void_p(12345)
    assert lib.sks_sketch_set_tally(ctx.h, (C.c_void_p * 1)(None), 1, (C.c_uint32 * 2)(0, 0), None, 1, None, None,
                                    C.byref(out), None, 0) == sksffi.SKS_E_ARG
    assert out.value is None and b"null" in lib.sks_last_error()
    arr = (C.c_void_p * 1)(base.h)
    out = C.c_void_p(12345)
    assert lib.sks_sketch_set_tally(ctx.h, arr, 1, None, None, 1, None, None, C.byref(out), None,
                                    0) == sksffi.SKS_E_ARG
    assert out.value is None and b"null" in lib.sks_last_error()
    out = C.c_void_p(12345)
    assert lib.sks_sketch_set_tally(ctx.h, arr, 1, (C.c_uint32 * 2)(0, 1), None, 1, None, None, C.byref(out), None,
                                    0) == sksffi.SKS_E_ARG
    assert out.value is None and b"null" in lib.sks_last_error()
    assert lib.sks_sketch_set_tally(ctx.h, arr, 1, (C.c_uint32 * 2)(0, 1), (C.c_uint32 * 1)(0), 1, None, None, None,
                                    None, 0) == sksffi.SKS_E_ARG
    with pytest.raises(sksffi.SksError, match="member index 7") as e:
        ctx.tally([base], [[0], [7]])
    assert e.value.code == sksffi.SKS_E_ARG
    with pytest.raises(ValueError, match="min_count"):
        ctx.tally([base], [[0], [1]], [1])
    # what is allowed: no groups at all, a max below the min (empty, no error), and the plain case
    assert ctx.tally([base], []).n == 0
    got, mult = ctx.tally([base], [], counts=True)
    assert got.n == 0 and len(mult) == 0
    assert ctx.tally([base], [[0, 1]], 2, 1).sizes().tolist() == [0]
    assert ctx.tally([base, base], [[0, 2]], 2, 2).sizes()[0] == base.sizes()[0]


@gpu_test
def test_sources_untouched_persist_search(gpu, tmp_path):
    torch, ctx = gpu
    w, k = SHAPES["narrow"]
    mask = sksffi.mask_generate(w, k, 0)
    sets = _three_sets(torch, ctx, w, mask)
    groups = [[0, 4, 8], [1, 5, 9], [3, 7]]
    sk, _ = _sources(sets)
    before = [s.tobytes() for s in sk]
    sizes_before = [s.sizes().copy() for s in sets]
    core, mult = ctx.tally(sets, groups, 2, counts=True)
    assert all(np.array_equal(s.sizes(), b) for s, b in zip(sets, sizes_before))
    assert [s.tobytes() for s in _sources(sets)[0]] == before
    queries = Genomes(torch, ctx, [20000, 15000, 18000, 20000],
                      specs=[(50, 31, 0.02), (51, 32, 0.0), (53, 33, 0.04), (999, 0, 0.0)]).build(w, mask, FRAC, 5)
    for s in sets:  # freeable right after the call
        s.free()
    counted = [_counted([sk[i] for i in g]) for g in groups]
    at = 0
    for g in range(len(groups)):
        want, cnt = _within(counted[g], 2, None)
        assert len(want) > 0 and np.array_equal(core.sketch(g), want)
        assert np.array_equal(mult[at:at + len(want)], cnt)
        at += len(want)
    core.set_names(["core a", "core b", "core c"])
    path = tmp_path / "core.sks"
    core.save(path)
    back = ctx.load_sketches(path)
    _same_sets(back, core)
    assert back.info() == core.info() and back.names() == ["core a", "core b", "core c"]
    got, want = ctx.search(queries, back), ctx.search(queries, core)
    assert len(want) >= 3 and (want["containment"] < 1.0).any()
    for f in sksffi.HIT_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f
