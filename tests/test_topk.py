"""The k best references per query (sks_search_topk / sks_search_topk_sets).

The sets follow the recipe of tests/test_search.py (its helpers are used as
they are): 70 queries x 130 references, synthetic genomes of 20-40 kb from 8
ancestors at substitution rates 0 .. 0.05, FracMinHash 1/50 under the w=31/k=21
mask, one empty query and one empty reference: a partial last 64-sketch block on
both sides, three reference blocks, and about 16 related references per query.
Two references carry query 0's genome, in different 64-blocks, so a full tie on
(score, shared) is broken by index across a batch boundary.

The expectation is computed on the host from the sketches copied out of the
device sets: np.intersect1d per pair, a float64 division by the rank kind's
denominator, sksffi.ani_from_counts, and per query a lexsort by (-score,
-shared, ref).  Every field must be equal exactly but ani, which may differ by
1e-9 (the tolerance of tests/test_search.py and tests/test_scale.py, for the
reason given there: the device pow is within an ulp of the host's).  Thresholds
sit midway between adjacent distinct values, so no pair is decided by rounding."""
import ctypes as C

import numpy as np
import pytest

import sksffi
from test_search import EMPTY, LargeCase, _build, _keys, _shared, _spec, _threshold

pytestmark = pytest.mark.gpu

Q_, R_, M_ = sksffi.SKS_RANK_QUERY, sksffi.SKS_RANK_REF, sksffi.SKS_RANK_MAX
NOREF = 0xffffffff


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.close()


def _scores(shared, qsizes, rsizes, rank):
    """(denominator, score) matrices of a rank kind; score 0 where nothing is shared."""
    q = np.broadcast_to(qsizes[:, None], shared.shape)
    r = np.broadcast_to(rsizes[None, :], shared.shape)
    den = {Q_: q, R_: r, M_: np.minimum(q, r)}[rank].astype(np.int64)
    score = np.zeros(shared.shape, dtype=np.float64)
    nz = shared > 0
    score[nz] = shared[nz].astype(np.float64) / den[nz].astype(np.float64)
    return den, score


def _expected(shared, qsizes, rsizes, kmer, k, rank, min_score=0.0, min_shared=1, skip=False):
    """(hits[q_n, k], counts[q_n], eligible[q_n, r_n]) as the contract states them."""
    nq, nr = shared.shape
    den, score = _scores(shared, qsizes, rsizes, rank)
    elig = (shared >= max(min_shared, 1)) & (score >= min_score)
    if skip:
        elig &= ~np.eye(nq, nr, dtype=bool)
    hits = np.zeros((nq, k), dtype=sksffi.TOP_HIT_DTYPE)
    hits["query"] = np.arange(nq, dtype=np.uint32)[:, None]
    hits["ref"] = NOREF
    hits["rank"] = np.arange(k, dtype=np.uint32)[None, :]
    counts = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        r = np.nonzero(elig[q])[0]
        r = r[np.lexsort((r, -shared[q, r].astype(np.int64), -score[q, r]))][:k]
        n = len(r)
        counts[q] = n
        if n == 0:
            continue
        cont, ani = sksffi.ani_from_counts(shared[q, r], den[q, r], kmer)
        assert np.array_equal(cont, score[q, r])
        row = hits[q, :n]
        row["ref"], row["shared"], row["score"], row["ani"] = r, shared[q, r], score[q, r], ani
        row["query_size"], row["ref_size"] = qsizes[q], rsizes[r]
    return hits, counts, elig


def _check(got, want):
    hits, counts = got
    w_hits, w_counts, _ = want
    assert hits.dtype == sksffi.TOP_HIT_DTYPE and hits.shape == w_hits.shape
    assert np.array_equal(counts, w_counts)
    for f in ("query", "ref", "shared", "query_size", "ref_size", "rank", "score"):
        assert np.array_equal(hits[f], w_hits[f]), f
    assert np.abs(hits["ani"] - w_hits["ani"]).max(initial=0.0) <= 1e-9
    empty = hits[hits["ref"] == NOREF]
    for f in ("shared", "query_size", "ref_size", "score", "ani"):
        assert not empty[f].any(), f


class Case:
    def __init__(self, torch, ctx, nq, nr, w, k, kind, param, r_param=None):
        self.w, self.k = w, k
        self.mask = sksffi.mask_generate(w, k, 0)
        qs = [_spec(i, 0) for i in range(nq)]
        rs = [_spec(i, 3) for i in range(nr)]
        qs[7] = (EMPTY,) + qs[7][1:]              # an empty query sketch
        rs[nr - 30] = (EMPTY,) + rs[nr - 30][1:]  # and an empty reference
        self.twins = (24, nr - 2)                 # query 0's genome twice, in different 64-blocks
        assert self.twins[0] // 64 != self.twins[1] // 64
        for t in self.twins:
            rs[t] = qs[0]
        self.Q = _build(torch, ctx, qs, w, self.mask, kind, param)
        self.R = _build(torch, ctx, rs, w, self.mask, kind, r_param or param)
        self.qsizes = self.Q.sizes().astype(np.int64)
        self.rsizes = self.R.sizes().astype(np.int64)
        self.shared = _shared(_keys(self.Q), _keys(self.R))
        assert self.qsizes[7] == 0 and self.rsizes[nr - 30] == 0

    def expected(self, k, rank, **kw):
        return _expected(self.shared, self.qsizes, self.rsizes, self.k, k, rank, **kw)


@pytest.fixture(scope="module")
def frac(gpu):
    torch, ctx = gpu
    return Case(torch, ctx, 70, 130, 31, 21, sksffi.SKS_FRAC_MOD, 50)


@pytest.fixture(scope="module")
def wide(gpu):
    torch, ctx = gpu
    return Case(torch, ctx, 70, 70, 45, 30, sksffi.SKS_FRAC_MOD, 50)


def _tie_by_index(hits, counts):
    """Some list holds two neighbours equal in (score, shared): their order is the index's."""
    for q in range(len(counts)):
        row = hits[q, :counts[q]]
        same = (row["score"][1:] == row["score"][:-1]) & (row["shared"][1:] == row["shared"][:-1])
        if same.any():
            assert (row["ref"][1:][same] > row["ref"][:-1][same]).all()
            return True
    return False


@pytest.mark.parametrize("rank", [Q_, R_, M_])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_k_and_rank_kinds(gpu, frac, k, rank):
    _, ctx = gpu
    want = frac.expected(k, rank)
    eligible = want[2].sum(axis=1)
    live = frac.qsizes > 0
    assert (eligible[~live] == 0).all() and not want[2][:, frac.R.n - 30].any()
    if k == 5:   # more eligible references than slots for every non-empty query: entries are evicted
        assert (eligible[live] > 5).all()
        assert _tie_by_index(want[0], want[1])  # query 0's twins, 24 before 128
    if k == 64:  # no query fills its list: partially filled lists
        assert (eligible < 64).all() and (want[1][live] > 0).all()
        assert _tie_by_index(want[0], want[1])
    got = ctx.search_topk(frac.Q, frac.R, k, rank=rank)
    _check(got, want)
    assert got[0]["ref"][got[0]["ref"] != NOREF].max() < frac.R.n


def test_rank_kinds_do_not_alias(frac):
    """The expected order of some query differs between SKS_RANK_QUERY and
    SKS_RANK_REF, so test_k_and_rank_kinds cannot pass with one kind for both."""
    a, b = frac.expected(5, Q_)[0], frac.expected(5, R_)[0]
    assert any(not np.array_equal(a["ref"][q], b["ref"][q]) for q in range(frac.Q.n))
    assert not np.array_equal(a["score"], b["score"])


def test_forced_batches(gpu, frac):
    """One and two reference blocks per batch (three and two batches of the 130
    references) give the default's arrays to the byte, for every rank kind."""
    _, ctx = gpu
    for rank in (Q_, R_, M_):
        base = ctx.search_topk(frac.Q, frac.R, 5, rank=rank)
        assert base[1].any()
        try:
            for blocks in (1, 2):
                ctx.set_search_batch(blocks)
                got = ctx.search_topk(frac.Q, frac.R, 5, rank=rank)
                assert got[0].tobytes() == base[0].tobytes(), (rank, blocks)
                assert got[1].tobytes() == base[1].tobytes(), (rank, blocks)
        finally:
            ctx.set_search_batch(0)


def test_wide_kmers(gpu, wide):
    """w=45 / k=30: 128-bit k-mers (elem_words 2), 70 x 70, default and one-block batches."""
    _, ctx = gpu
    assert wide.Q.elem_words == 2
    _check(ctx.search_topk(wide.Q, wide.R, 5, rank=M_), wide.expected(5, M_))
    try:
        ctx.set_search_batch(1)
        _check(ctx.search_topk(wide.Q, wide.R, 5, rank=M_), wide.expected(5, M_))
        _check(ctx.search_topk(wide.Q, wide.R, 64), wide.expected(64, Q_))
    finally:
        ctx.set_search_batch(0)


def test_agrees_with_search(gpu, frac):
    """SKS_RANK_QUERY, k = 64, min_score = thr: the filled records are the pairs
    sks_search_sets reports at min_containment = thr, with the same bits in
    shared, query_size, score / containment and ani."""
    _, ctx = gpu
    thr = _threshold(frac.shared, frac.qsizes)
    _, score = _scores(frac.shared, frac.qsizes, frac.rsizes, Q_)
    assert ((score >= thr) & (frac.shared > 0)).sum(axis=1).max() <= 64  # no list overflows
    want = ctx.search(frac.Q, frac.R, min_containment=thr)
    assert len(want)
    hits, counts = ctx.search_topk(frac.Q, frac.R, 64, rank=Q_, min_score=thr)
    assert int(counts.sum()) == len(want)
    rows = []
    for q in range(frac.Q.n):  # query by query, each list put in ref order
        row = hits[q, :counts[q]]
        assert (row["query"] == q).all() and (row["rank"] == np.arange(counts[q])).all()
        rows.append(row[np.argsort(row["ref"])])
    got = np.concatenate(rows)
    for f, g in (("query", "query"), ("ref", "ref"), ("shared", "shared"), ("query_size", "query_size"),
                 ("containment", "score"), ("ani", "ani")):
        assert np.ascontiguousarray(want[f]).tobytes() == np.ascontiguousarray(got[g]).tobytes(), f


def test_few_queries_many_large_references(gpu):
    """The large case of tests/test_search.py (6 queries x 330 references of
    about 23 000 elements: one query block of region log 1 against reference
    batches of region log 3 and 2): the 5 best per query by containment in the
    query, in one batch and in batches of four and two blocks."""
    torch, ctx = gpu
    case = LargeCase(torch, ctx, 330, 31, 21)
    want = _expected(case.shared, case.qsizes, case.rsizes, case.k, 5, Q_)
    assert want[1].tolist() == [5, 5, 0, 5, 5, min(5, int((case.shared[5] > 0).sum()))]
    # query 0's genome is a prefix of every unmutated copy of its ancestor: full ties, decided by
    # the index across blocks (its own genome is reference 24)
    assert want[0]["ref"][0].tolist() == [0, 24, 48, 72, 96] and (want[0]["score"][0] == 1.0).all()
    try:
        for blocks in (0, 4):
            ctx.set_search_batch(blocks)
            _check(ctx.search_topk(case.Q, case.R, 5, rank=Q_), want)
    finally:
        ctx.set_search_batch(0)


def _midpoint(values):
    """Midpoint of the widest gap between adjacent distinct values; none within 1e-9 of it."""
    u = np.unique(values)
    assert len(u) >= 2
    g = int(np.argmax(np.diff(u)))
    thr = (u[g] + u[g + 1]) / 2
    assert np.abs(values - thr).min() > 1e-9
    return thr


def test_min_shared_and_min_score(gpu, frac):
    _, ctx = gpu
    u = np.unique(frac.shared[frac.shared > 0])
    ms = int(u[len(u) // 2])
    assert u[len(u) // 2 - 1] < ms  # between two observed counts
    want = frac.expected(5, Q_, min_shared=ms)
    assert 0 < want[2].sum() < (frac.shared > 0).sum()
    _check(ctx.search_topk(frac.Q, frac.R, 5, min_shared=ms), want)
    for rank in (R_, M_):
        _, score = _scores(frac.shared, frac.qsizes, frac.rsizes, rank)
        thr = _midpoint(score[frac.shared > 0])
        want = frac.expected(5, rank, min_score=thr)
        assert 0 < want[2].sum() < (frac.shared > 0).sum()
        _check(ctx.search_topk(frac.Q, frac.R, 5, rank=rank, min_score=thr), want)
    # both at once, and a min_shared below 1 never lets pairs that share nothing in
    _, score = _scores(frac.shared, frac.qsizes, frac.rsizes, Q_)
    thr = _midpoint(score[frac.shared > 0])
    _check(ctx.search_topk(frac.Q, frac.R, 64, min_score=thr, min_shared=ms),
           frac.expected(64, Q_, min_score=thr, min_shared=ms))
    _check(ctx.search_topk(frac.Q, frac.R, 64, min_score=-1.0, min_shared=-5), frac.expected(64, Q_))


def test_knn_of_one_set(gpu, frac):
    """The reference set against itself: with skip_same_index no sketch lists
    itself; without it every non-empty sketch lists itself with score 1.0."""
    _, ctx = gpu
    S = frac.R
    sizes = frac.rsizes
    own = _shared(_keys(S), _keys(S))
    hits, counts = ctx.search_topk(S, S, 5, skip_same_index=True)
    _check((hits, counts), _expected(own, sizes, sizes, frac.k, 5, Q_, skip=True))
    assert not (hits["ref"] == hits["query"]).any()
    a, b = frac.twins  # each twin lists the other with score 1.0, not itself
    assert hits[a][hits[a]["ref"] == b]["score"].tolist() == [1.0]
    assert hits[b][hits[b]["ref"] == a]["score"].tolist() == [1.0]
    hits, counts = ctx.search_topk(S, S, 5)
    _check((hits, counts), _expected(own, sizes, sizes, frac.k, 5, Q_))
    for i in range(S.n):
        me = hits[i][hits[i]["ref"] == i]
        if sizes[i]:
            assert len(me) == 1 and me[0]["score"] == 1.0 and me[0]["shared"] == sizes[i]
        else:
            assert counts[i] == 0 and len(me) == 0


def test_bottom_s_of_different_s(gpu):
    """Bottom-128 queries against bottom-256 references: accepted and exact."""
    torch, ctx = gpu
    case = Case(torch, ctx, 70, 70, 31, 21, sksffi.SKS_BOTTOM_S, 128, r_param=256)
    assert case.Q.info()["param"] == 128 and case.R.info()["param"] == 256
    for rank in (Q_, R_):
        _check(ctx.search_topk(case.Q, case.R, 5, rank=rank), case.expected(5, rank))


def _arrays(ss):
    sz = ss.sizes().astype(np.int64)
    return ss.device_ptrs() + (ss.n, int(sz.max()), int(sz.sum()))


def test_array_form_and_edges(gpu, frac):
    torch, ctx = gpu
    some, none = _arrays(frac.R), (0, 0, 0, 0, 0, 0)
    # the device-array form (bounds sampled from the references), default and one-block batches
    want = frac.expected(5, M_)
    try:
        for blocks in (0, 1):
            ctx.set_search_batch(blocks)
            _check(ctx.search_topk_arrays(_arrays(frac.Q), some, 1, frac.k, 5, rank=M_), want)
    finally:
        ctx.set_search_batch(0)
    # no references: every slot of every query is written, empty
    hits, counts = ctx.search_topk_arrays(_arrays(frac.Q), none, 1, frac.k, 3)
    assert hits.shape == (frac.Q.n, 3) and not counts.any()
    assert (hits["ref"] == NOREF).all() and np.array_equal(hits["query"], np.arange(70)[:, None].repeat(3, 1))
    assert np.array_equal(hits["rank"], np.arange(3)[None, :].repeat(70, 0))
    for f in ("shared", "query_size", "ref_size", "score", "ani"):
        assert not hits[f].any()
    # no queries: SKS_OK, nothing written (no buffers needed)
    assert ctx.search_topk_arrays_raw(none, some, 1, frac.k, Q_, 5, 0.0, 1, False, 0, 0) == sksffi.SKS_OK
    # counts may be NULL
    buf = torch.zeros(70 * 5 * 40, dtype=torch.uint8, device="cuda:0")
    assert ctx.search_topk_sets_raw(frac.Q, frac.R, M_, 5, 0.0, 1, False, buf.data_ptr(), 0) == sksffi.SKS_OK
    ctx.synchronize()
    assert buf.cpu().numpy().view(sksffi.TOP_HIT_DTYPE).tobytes() == \
        ctx.search_topk(frac.Q, frac.R, 5, rank=M_)[0].tobytes()


def test_argument_checks(gpu, frac):
    torch, ctx = gpu
    L = sksffi.lib()
    buf = torch.zeros(70 * 64 * 40, dtype=torch.uint8, device="cuda:0")
    d = buf.data_ptr()
    q, r = _arrays(frac.Q), _arrays(frac.R)

    def sets(rank=Q_, k=5, min_score=0.0, hits=d):
        return ctx.search_topk_sets_raw(frac.Q, frac.R, rank, k, min_score, 1, False, hits, 0)

    def arrays(ew=1, ones=21, rank=Q_, k=5, min_score=0.0, hits=d):
        return ctx.search_topk_arrays_raw(q, r, ew, ones, rank, k, min_score, 1, False, hits, 0)

    def err():
        return L.sks_last_error().decode()

    E_ARG, E_UNS = sksffi.SKS_E_ARG, sksffi.SKS_E_UNSUPPORTED
    assert L.sks_search_topk_sets(None, frac.Q.h, frac.R.h, Q_, 5, 0.0, 1, 0, C.c_void_p(d), None) == E_ARG
    assert "ctx" in err()
    v = C.c_void_p
    assert L.sks_search_topk(None, v(q[0]), v(q[1]), v(q[2]), q[3], q[4], q[5], v(r[0]), v(r[1]), v(r[2]), r[3],
                             r[4], r[5], 1, 21, Q_, 5, 0.0, 1, 0, v(d), None) == E_ARG
    assert "ctx" in err()
    for call in (sets, arrays):
        assert call(hits=0) == E_ARG and "d_hits" in err()
        assert call(k=0) == E_ARG and "k must" in err()
        assert call(min_score=float("nan")) == E_ARG and "min_score" in err()
        for bad in (3, -1):
            assert call(rank=bad) == E_ARG and "rank_kind" in err()
        assert call(k=65) == E_UNS and "k = 65" in err()
        assert call(k=64) == sksffi.SKS_OK
    assert arrays(ew=3) == E_ARG and "elem_words" in err()
    assert arrays(ones=0) == E_ARG and "kmer_num_ones" in err()
    assert ctx.search_topk_sets_raw(frac.Q, None, Q_, 5, 0.0, 1, False, d, 0) == E_ARG
    ctx.synchronize()


def test_incompatible_sets(gpu):
    """The rules and messages of sks_search_sets."""
    torch, ctx = gpu
    specs = [_spec(i, 0) for i in range(2)]
    m = sksffi.mask_generate(31, 21, 0)
    F = sksffi.SKS_FRAC_MOD
    base = _build(torch, ctx, specs, 31, m, F, 50)
    others = {
        "window": _build(torch, ctx, specs, 32, m, F, 50),
        "mask": _build(torch, ctx, specs, 31, sksffi.mask_generate(31, 21, 1), F, 50),
        "hash flavour": _build(torch, ctx, specs, 31, m, F, 50, flavour=1),
        "policy param": _build(torch, ctx, specs, 31, m, F, 40),
    }
    for field, other in others.items():
        with pytest.raises(sksffi.SksError, match="the query and reference sets differ in " + field) as e:
            ctx.search_topk(base, other, 2)
        assert e.value.code == 1, field


def test_invalid_layout(gpu, monkeypatch):
    """The recipe of tests/test_search.py::test_invalid_layout_reports_no_hits
    through the array form: SKS_E_UNSUPPORTED naming the invalid layout."""
    torch, ctx = gpu
    monkeypatch.setenv("SKS_LAYOUT_GROUP_CAP", "64")
    rng = np.random.default_rng(31)
    n = 70
    hi = np.arange(1000, 1300, dtype=np.uint64)
    with np.errstate(over="ignore"):
        lo = np.uint64(0x1234567) ^ (hi * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(0x165667B19E3779F9))
    coll = np.stack([lo, hi], axis=1)
    sk = []
    for _ in range(n):
        ex = rng.integers(2**40, 2**63, size=(300, 2), dtype=np.uint64)
        a = np.unique(np.concatenate([coll[rng.random(len(coll)) < 0.8], ex]), axis=0)
        sk.append(a[np.lexsort((a[:, 0], a[:, 1]))])
    sizes = np.array([len(x) for x in sk], dtype=np.uint32)
    starts = np.zeros(n, dtype=np.uint64)
    starts[1:] = np.cumsum(sizes[:-1], dtype=np.uint64)
    d = torch.from_numpy(np.concatenate([x.reshape(-1) for x in sk]).view(np.int64)).to("cuda:0")
    st = torch.from_numpy(starts.view(np.int64)).to("cuda:0")
    sz = torch.from_numpy(sizes.view(np.int32)).to("cuda:0")
    side = (d.data_ptr(), st.data_ptr(), sz.data_ptr(), n, int(sizes.max()), int(sizes.sum()))
    buf = torch.zeros(n * 5 * 40, dtype=torch.uint8, device="cuda:0")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    rc = ctx.search_topk_arrays_raw(side, side, 2, 30, Q_, 5, 0.0, 1, False, buf.data_ptr(), cnt.data_ptr())
    assert rc == sksffi.SKS_E_UNSUPPORTED
    assert b"invalid layout" in sksffi.lib().sks_last_error()
    ctx.synchronize()
