"""Greedy min-set cover of a query sketch on the device (sks_gather /
sks_gather_sets).

The expected hits come from the host greedy loop of tests/gather_ref.py over
Python sets of the sketches copied out of the device sets: ref, shared,
shared_new, ref_size, f_query_new, the number of hits and n_unexplained must be
exactly equal (integers, and one float64 division of integers); ani must be
bit-equal to the ani sks_search_sets reports for the same pair and within 1e-9
of sksffi.ani_from_counts (the comparison tests/test_search.py uses: the device
pow is within an ulp of the host's).

Sketched genomes are synthetic (sks_synth_bases) and laid out as in
tests/test_cluster.py: genome i belongs to family i % 8, whose first member is
the ancestor and whose later members descend from it at substitution rates 0.01
and 0.02; one segment is too short for any window.  The mixture is one segment
of two ancestors, a 0.01 and a 0.02 descendant of two further families (with
mutation seeds of their own and 31 kb long, longer than their ancestors, so the
longer siblings explain a few tail k-mers after the ancestor was taken) and
20 kb that matches nothing.  The seeds were chosen with the CPU oracle so that
the preconditions the tests assert hold."""
import ctypes as C

import numpy as np
import pytest

import sksffi
from cluster_ref import keys_of
from gather_ref import as_set, greedy

pytestmark = pytest.mark.gpu

N_FAM = 8
EMPTY = 5            # bases of a segment too short for any window: an empty sketch
EMPTY_AT = 77
LATE = (1, 9)        # the generations (i // 8) at rate 0.02; the others descend at 0.01
NOISE = (20000, 999, 0, 0.0)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.close()


def spec(i):
    """Genome i: (length, ancestor seed, mutation seed, rate)."""
    gen = i // N_FAM
    rate = 0.0 if gen == 0 else (0.02 if gen in LATE else 0.01)
    length = EMPTY if i == EMPTY_AT else 29000 + (i * 997) % 2001
    return (length, 300 + i % N_FAM, 7400 + i, rate)


# two ancestors, a fresh 0.01 descendant of family 4, a fresh 0.02 descendant of family 3, noise
MIXTURE = [spec(0), spec(1), (31000, 304, 9002, 0.01), (31000, 303, 9052, 0.02), NOISE]
MIXTURE_WIDE = [spec(0), (31000, 304, 9002, 0.01), (31000, 303, 9052, 0.02), NOISE]


def _build(torch, ctx, segments, w, mask, kind=sksffi.SKS_FRAC_MOD, param=50):
    """One sketch per segment; a segment is a list of genome specs separated by newlines."""
    offs = [0]
    for seg in segments:
        offs.append(offs[-1] + sum(L + 1 for L, _, _, _ in seg))
    dev = torch.full((offs[-1],), ord("\n"), dtype=torch.uint8, device="cuda:0")
    for s, seg in enumerate(segments):
        at = offs[s]
        for L, seed, mseed, rate in seg:
            ctx.synth_bases(dev.data_ptr() + at, L, seed, mseed, rate)
            at += L + 1
    torch.cuda.synchronize()
    return ctx.sketch_build(dev.data_ptr(), offs[-1], offs, w, mask, kind, param)


def _check(got, want):
    hits, un = got
    w_hits, w_un = want[0], want[1]
    assert hits.dtype == sksffi.GATHER_HIT_DTYPE
    assert len(hits) == len(w_hits), (hits["ref"].tolist(), w_hits["ref"].tolist())
    for f in ("ref", "shared", "shared_new", "ref_size", "f_query_new"):
        assert np.array_equal(hits[f], w_hits[f]), f
    assert np.abs(hits["ani"] - w_hits["ani"]).max(initial=0.0) <= 1e-9
    assert un == w_un


class Case:
    """A reference set, a one-sketch query set and the host's sets of both."""

    def __init__(self, torch, ctx, ref_specs, mixture, w, k):
        self.w, self.k = w, k
        self.mask = sksffi.mask_generate(w, k, 0)
        self.R = _build(torch, ctx, [[s] for s in ref_specs], w, self.mask)
        self.Q = _build(torch, ctx, [mixture], w, self.mask)
        self.refs = [as_set(x) for x in keys_of(self.R)]
        self.query = as_set(keys_of(self.Q)[0])

    def expected(self, min_shared=1, max_rounds=0):
        return greedy(self.query, self.refs, self.k, min_shared, max_rounds)


@pytest.fixture(scope="module")
def frac(gpu):
    torch, ctx = gpu
    return Case(torch, ctx, [spec(i) for i in range(130)], MIXTURE, 31, 21)


@pytest.fixture(scope="module")
def wide(gpu):
    torch, ctx = gpu
    return Case(torch, ctx, [spec(i) for i in range(70)], MIXTURE_WIDE, 45, 30)


class Arrays:
    """A query and references uploaded as the device-array form takes them;
    elements are u64 (elem_words 1) or (lo, hi) rows ordered by hi, then lo."""

    def __init__(self, torch, query, refs, ew):
        self.ew = ew
        shape = (0,) if ew == 1 else (0, 2)
        q = np.asarray(query, dtype=np.uint64).reshape((-1,) + shape[1:])
        rs = [np.asarray(r, dtype=np.uint64).reshape((-1,) + shape[1:]) for r in refs]
        sizes = np.array([len(r) for r in rs], dtype=np.uint32)
        starts = np.zeros(len(rs), dtype=np.uint64)
        starts[1:] = np.cumsum(sizes[:-1], dtype=np.uint64)
        flat = np.concatenate([r.reshape(-1) for r in rs] + [np.zeros(1, dtype=np.uint64)])
        self.keep = [torch.from_numpy(np.concatenate([q.reshape(-1), np.zeros(1, dtype=np.uint64)]).view(np.int64)).to("cuda:0"),
                     torch.from_numpy(flat.view(np.int64)).to("cuda:0"),
                     torch.from_numpy(np.concatenate([starts, [0]]).astype(np.uint64).view(np.int64)).to("cuda:0"),
                     torch.from_numpy(np.concatenate([sizes, [0]]).astype(np.uint32).view(np.int32)).to("cuda:0")]
        self.query = (self.keep[0].data_ptr(), len(q))
        self.side = (self.keep[1].data_ptr(), self.keep[2].data_ptr(), self.keep[3].data_ptr(), len(rs),
                     int(sizes.max(initial=0)), int(sizes.sum()))
        if ew == 1:
            self.q_set, self.r_sets = set(q.tolist()), [set(r.tolist()) for r in rs]
        else:
            self.q_set, self.r_sets = as_set(q), [as_set(r) for r in rs]


def closed_form():
    """Q = 1000 values 3 i + 7 (not a multiple of 64: the bitmap's tail word is
    live).  Reference i holds Q's positions [a, a + L) cut at 1000, j = i % 150,
    a = 41 j % 1000, L = 20 + 37 j % 90, and i % 7 values of its own above 10^7;
    references 150 .. 199 repeat the query part of 0 .. 49; i % 50 == 49 is empty."""
    Q = [3 * i + 7 for i in range(1000)]
    refs = []
    for i in range(200):
        if i % 50 == 49:
            refs.append([])
            continue
        j = i % 150
        a, L = (41 * j) % 1000, 20 + (37 * j) % 90
        refs.append(Q[a:min(1000, a + L)] + [10_000_000 + 10 * i + t for t in range(i % 7)])
    return Q, refs


# thr -> (rounds, candidates, rounds decided by the index tie-break, rounds with shared_new < shared, n_unexplained)
CLOSED_FORM_FACTS = {1: (15, 196, 9, 10, 0), 8: (13, 195, 7, 8, 3)}


@pytest.mark.parametrize("thr", [1, 8])
def test_closed_form_arrays(gpu, thr):
    torch, ctx = gpu
    Q, refs = closed_form()
    A = Arrays(torch, Q, refs, 1)
    want = greedy(A.q_set, A.r_sets, 21, thr)
    hits, un, info = want
    assert (len(hits), info["candidates"], info["ties"], info["partial"], un) == CLOSED_FORM_FACTS[thr]
    assert len(hits) >= 5 and info["ties"] >= 1 and info["candidates"] > len(hits)
    by_shared = sorted(range(len(hits)), key=lambda x: (-int(hits["shared"][x]), int(hits["ref"][x])))
    assert by_shared != list(range(len(hits))), "the hit order is the order by shared"
    got = ctx.gather_arrays(A.query, A.side, 1, 21, min_shared=thr)
    print("thr", thr, "got", got[0]["ref"].tolist(), "want", hits["ref"].tolist(), got[1], un)
    _check(got, want)


def test_long_lists(gpu):
    """Position lists of one, two and three scoring chunks (2048 positions a
    workgroup) beside short ones: lists of exactly 2048 and of 2049 positions,
    references overlapping across chunk borders, at the default group size and
    at one round per wait."""
    torch, ctx = gpu
    Q = [5 * i + 2 for i in range(10000)]
    spans = [(0, 5000), (3000, 8990), (0, 2048), (0, 2049), (8000, 9995), (4090, 4100), (9990, 10000), (2047, 2050),
             (6000, 6003), (9500, 9998)]
    refs = [Q[a:b] + [10_000_000 + 10 * i + t for t in range(i % 3)] for i, (a, b) in enumerate(spans)]
    A = Arrays(torch, Q, refs, 1)
    want = greedy(A.q_set, A.r_sets, 21, 2)
    assert want[0]["ref"].tolist() == [1, 0, 4, 6] and want[0]["shared_new"].tolist() == [5990, 3000, 1005, 5]
    assert want[0]["shared"].tolist() == [5990, 5000, 1995, 10] and want[1] == 0 and want[2]["candidates"] == 10
    _check(ctx.gather_arrays(A.query, A.side, 1, 21, min_shared=2), want)
    try:
        ctx.set_gather_rounds(1)
        _check(ctx.gather_arrays(A.query, A.side, 1, 21, min_shared=2), want)
    finally:
        ctx.set_gather_rounds(0)


def test_sketched_mixture(gpu, frac):
    _, ctx = gpu
    want = frac.expected(min_shared=3)
    hits, un, info = want
    assert len(frac.R.sizes()) == 130 and frac.R.sizes()[EMPTY_AT] == 0
    assert len(hits) >= 5 and un > 0
    assert info["candidates"] > len(hits), "no reference passes shared >= thr without being reported"
    assert (hits["shared_new"] < hits["shared"]).any()
    got = ctx.gather(frac.Q, 0, frac.R, min_shared=3)
    print("got", got[0]["ref"].tolist(), got[0]["shared_new"].tolist(), got[1], "want", hits["ref"].tolist(), un)
    _check(got, want)
    # the same doubles as the search reports for the pair (reference first: its size divides)
    pairs = ctx.search(frac.R, frac.Q, min_shared=1)
    by_ref = {int(h["query"]): h for h in pairs}
    for h in got[0]:
        s = by_ref[int(h["ref"])]
        assert int(s["shared"]) == int(h["shared"]) and int(s["query_size"]) == int(h["ref_size"])
        assert np.float64(s["ani"]).tobytes() == np.float64(h["ani"]).tobytes()
    _, ani = sksffi.ani_from_counts(got[0]["shared"], got[0]["ref_size"], frac.k)
    assert np.abs(got[0]["ani"] - ani).max() <= 1e-9


def test_forced_round_groups(gpu, frac):
    """One and two rounds per host wait give the default's hit array to the byte."""
    _, ctx = gpu
    base = ctx.gather(frac.Q, 0, frac.R, min_shared=3)
    assert len(base[0]) >= 5
    try:
        for rounds in (1, 2):
            ctx.set_gather_rounds(rounds)
            got = ctx.gather(frac.Q, 0, frac.R, min_shared=3)
            assert got[0].tobytes() == base[0].tobytes() and got[1] == base[1], rounds
    finally:
        ctx.set_gather_rounds(0)


def test_max_rounds_and_hit_cap(gpu, frac):
    torch, ctx = gpu
    every = frac.expected(min_shared=3)
    n = len(every[0])
    assert n >= 5
    first2 = frac.expected(min_shared=3, max_rounds=2)
    assert len(first2[0]) == 2 and np.array_equal(first2[0], every[0][:2]) and first2[1] > every[1]
    _check(ctx.gather(frac.Q, 0, frac.R, min_shared=3, max_rounds=2), first2)
    # a short buffer: SKS_E_LENGTH and still the exact count
    buf = torch.zeros(2 * 32, dtype=torch.uint8, device="cuda:0")
    rc, got_n, un = ctx.gather_sets_raw(frac.Q, 0, frac.R, 3, 0, buf.data_ptr(), 2)
    assert (rc, got_n, un) == (sksffi.SKS_E_LENGTH, n, every[1])
    assert b"capacity 2" in sksffi.lib().sks_last_error()
    # a size query, and n_unexplained may be NULL
    assert ctx.gather_sets_raw(frac.Q, 0, frac.R, 3, 0, 0, 0) == (sksffi.SKS_OK, n, every[1])
    assert ctx.gather_sets_raw(frac.Q, 0, frac.R, 3, 0, 0, 0, want_unexplained=False) == (sksffi.SKS_OK, n, None)
    big = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    assert ctx.gather_sets_raw(frac.Q, 0, frac.R, 3, 0, big.data_ptr(), n, want_unexplained=False) == \
        (sksffi.SKS_OK, n, None)
    ctx.synchronize()
    assert np.array_equal(big.cpu().numpy().view(sksffi.GATHER_HIT_DTYPE)["ref"], every[0]["ref"])


def test_wide_kmers(gpu, wide):
    """w=45 / k=30: 128-bit k-mers (elem_words 2), 70 references and a mixture of
    3, at the default group size and at one round per wait."""
    _, ctx = gpu
    assert wide.R.elem_words == 2 and wide.Q.elem_words == 2
    want = wide.expected(min_shared=1)
    assert len(want[0]) >= 3 and want[1] > 0 and want[2]["candidates"] > len(want[0])
    _check(ctx.gather(wide.Q, 0, wide.R), want)
    try:
        ctx.set_gather_rounds(1)
        _check(ctx.gather(wide.Q, 0, wide.R), want)
    finally:
        ctx.set_gather_rounds(0)


def test_wide_arrays_closed_form(gpu):
    """128-bit values from few distinct lo and hi words: many share lo and differ
    in hi, and the reverse, so a comparison of one word alone misplaces them.
    Q holds 65 of them (one more than a wavefront), 5 references."""
    torch, ctx = gpu
    los = [1, 5, 1 << 40, (1 << 64) - 3, 77]
    his = [0, 1, 2, 1 << 63, 9, (1 << 64) - 1, 12, 13, 14, 15, 16, 17, 18]
    grid = sorted(((hi, lo) for hi in his for lo in los))  # 65 values in (hi, lo) order
    assert len(grid) == 65
    Q = np.array([[lo, hi] for hi, lo in grid], dtype=np.uint64)

    def ref(pick, extra):
        rows = sorted([grid[i] for i in pick] + extra)
        return np.array([[lo, hi] for hi, lo in rows], dtype=np.uint64).reshape(-1, 2)
    refs = [ref(range(0, 40), [(3, 5)]),                 # (hi 3, lo 5): a lo of Q under a hi between two of Q's
            ref(range(30, 65), [(0, 6), (1 << 63, 2)]),
            ref(range(0, 65, 3), []),
            ref([], [(hi, 6) for hi in his]),              # every hi of Q with a lo Q lacks: shares nothing
            ref(range(10, 20), [(5, lo) for lo in los])]   # every lo of Q with a hi Q lacks
    A = Arrays(torch, Q, refs, 2)
    want = greedy(A.q_set, A.r_sets, 30, 1)
    assert want[0]["ref"].tolist() == [0, 1] and want[0]["shared_new"].tolist() == [40, 25] and want[1] == 0
    assert want[0]["shared"].tolist() == [40, 35] and want[2]["candidates"] == 4
    _check(ctx.gather_arrays(A.query, A.side, 2, 30), want)


def test_extremes(gpu, frac):
    torch, ctx = gpu
    # an empty query (a segment too short for a window)
    E = _build(torch, ctx, [[(EMPTY, 300, 0, 0.0)]], 31, frac.mask)
    assert E.sizes()[0] == 0
    hits, un = ctx.gather(E, 0, frac.R)
    assert len(hits) == 0 and un == 0
    # a query equal to reference 7, reference 90 being a copy of it
    specs = [spec(7) if i == 90 else spec(i) for i in range(130)]
    D = _build(torch, ctx, [[s] for s in specs], 31, frac.mask)
    Q7 = _build(torch, ctx, [[spec(7)]], 31, frac.mask)
    size = int(Q7.sizes()[0])
    assert size > 0 and D.sizes()[7] == size == D.sizes()[90]
    hits, un = ctx.gather(Q7, 0, D)
    assert len(hits) == 1 and un == 0
    assert (int(hits["ref"][0]), int(hits["shared"][0]), int(hits["shared_new"][0]), int(hits["ref_size"][0])) == \
        (7, size, size, size)
    assert hits["f_query_new"][0] == 1.0 and hits["ani"][0] == 1.0
    # min_shared above every shared: nothing, and everything unexplained
    top = int(frac.expected()[0]["shared"].max())
    hits, un = ctx.gather(frac.Q, 0, frac.R, min_shared=top + 1)
    assert len(hits) == 0 and un == len(frac.query)
    _check(ctx.gather(frac.Q, 0, frac.R, min_shared=top), frac.expected(min_shared=top))
    # a single-element query, held by references 1 and 2
    A = Arrays(torch, [50], [[1, 2, 3], [7, 50], [50, 51, 52], []], 1)
    want = greedy(A.q_set, A.r_sets, 21)
    assert want[0]["ref"].tolist() == [1] and want[1] == 0
    _check(ctx.gather_arrays(A.query, A.side, 1, 21), want)
    # one reference
    one = _build(torch, ctx, [[spec(0)]], 31, frac.mask)
    want = greedy(frac.query, [as_set(keys_of(one)[0])], 21)
    assert len(want[0]) == 1 and want[1] > 0
    _check(ctx.gather(frac.Q, 0, one), want)
    # thresholds below their lowest count as 1
    _check(ctx.gather(frac.Q, 0, frac.R, min_shared=-5), frac.expected(min_shared=1))


def test_order_independent(gpu, frac):
    """The same references in a permuted order: no round of this mixture is
    decided by the index, so the same references come out, renumbered."""
    torch, ctx = gpu
    want = frac.expected(min_shared=3)
    assert want[2]["ties"] == 0 and len(want[0]) >= 5
    perm = np.random.default_rng(5).permutation(130)  # new position p holds genome perm[p]
    P = _build(torch, ctx, [[spec(int(g))] for g in perm], 31, frac.mask)
    hits, un = ctx.gather(frac.Q, 0, P, min_shared=3)
    base, base_un = ctx.gather(frac.Q, 0, frac.R, min_shared=3)
    assert un == base_un and np.array_equal(perm[hits["ref"]], base["ref"])
    for f in ("shared", "shared_new", "ref_size", "f_query_new", "ani"):
        assert hits[f].tobytes() == base[f].tobytes(), f


def test_argument_errors(gpu, frac):
    torch, ctx = gpu
    L = sksffi.lib()
    tiny = [[(3000, 41, 0, 0.0)]]

    def refused(q_set, r_set, field):
        rc, n, _ = ctx.gather_sets_raw(q_set, 0, r_set, 1, 0, 0, 0)
        assert (rc, n) == (sksffi.SKS_E_ARG, 0)
        assert field.encode() in L.sks_last_error(), (field, L.sks_last_error())
    base = _build(torch, ctx, tiny, 31, frac.mask)
    refused(_build(torch, ctx, tiny, 33, sksffi.mask_generate(33, 21, 0)), base, "window")
    refused(_build(torch, ctx, tiny, 31, sksffi.mask_generate(31, 21, 1)), base, "mask")
    refused(_build(torch, ctx, tiny, 31, frac.mask, sksffi.SKS_FRAC_MOD, 100), base, "policy param")
    bottom = _build(torch, ctx, tiny, 31, frac.mask, sksffi.SKS_BOTTOM_S, 64)
    refused(bottom, bottom, "policy kind")
    refused(bottom, base, "policy kind")
    # q out of range, null sets, null n_hits
    rc, n, _ = ctx.gather_sets_raw(frac.Q, 1, frac.R, 1, 0, 0, 0)
    assert (rc, n) == (sksffi.SKS_E_ARG, 0) and b"out of range" in L.sks_last_error()
    assert ctx.gather_sets_raw(None, 0, frac.R, 1, 0, 0, 0)[:2] == (sksffi.SKS_E_ARG, 0)
    assert ctx.gather_sets_raw(frac.Q, 0, None, 1, 0, 0, 0)[:2] == (sksffi.SKS_E_ARG, 0)
    assert L.sks_gather_sets(ctx.h, frac.Q.h, 0, frac.R.h, 1, 0, None, 0, None, None) == sksffi.SKS_E_ARG
    # the array form
    Q, refs = closed_form()
    A = Arrays(torch, Q, refs, 1)
    assert ctx.gather_arrays_raw(A.query, A.side, 3, 21, 1, 0, 0, 0)[:2] == (sksffi.SKS_E_ARG, 0)
    assert ctx.gather_arrays_raw(A.query, A.side, 1, 0, 1, 0, 0, 0)[:2] == (sksffi.SKS_E_ARG, 0)
    assert ctx.gather_arrays_raw((0, 5), A.side, 1, 21, 1, 0, 0, 0)[:2] == (sksffi.SKS_E_ARG, 0)
    assert ctx.gather_arrays_raw(A.query, (A.side[0], 0, 0) + A.side[3:], 1, 21, 1, 0, 0, 0)[:2] == \
        (sksffi.SKS_E_ARG, 0)
    v = C.c_void_p
    assert L.sks_gather(ctx.h, v(A.query[0]), A.query[1], v(A.side[0]), v(A.side[1]), v(A.side[2]), A.side[3],
                        A.side[4], A.side[5], 1, 21, 1, 0, None, 0, None, None) == sksffi.SKS_E_ARG
    # >= 2^32 reference elements: refused before anything is launched
    assert ctx.gather_arrays_raw(A.query, A.side[:5] + (1 << 32,), 1, 21, 1, 0, 0, 0)[:2] == \
        (sksffi.SKS_E_UNSUPPORTED, 0)
    # sizes that add up to more than r_total: refused, nothing searched
    rc, n, _ = ctx.gather_arrays_raw(A.query, A.side[:5] + (A.side[5] - 1,), 1, 21, 1, 0, 0, 0)
    assert (rc, n) == (sksffi.SKS_E_ARG, 0) and b"r_total" in L.sks_last_error()
    # no query elements or no references: SKS_OK and no hits
    assert ctx.gather_arrays_raw((0, 0), A.side, 1, 21, 1, 0, 0, 0) == (sksffi.SKS_OK, 0, 0)
    assert ctx.gather_arrays_raw(A.query, (0, 0, 0, 0, 0, 0), 1, 21, 1, 0, 0, 0) == (sksffi.SKS_OK, 0, 1000)
    ctx.synchronize()
