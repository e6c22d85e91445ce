"""Query-vs-reference search (sks_search / sks_search_sets): thresholded hit
lists instead of a dense matrix.

Genomes are synthetic (sks_synth_bases): a few ancestors, each with descendants
at substitution rates 0 .. 0.05 and lengths 20-40 kb, so a query shares
everything, something or nothing with a reference.  The expected hits are
computed on the host from the sketches copied out of the device sets
(np.intersect1d per pair, float64 shared / size, sksffi.ani_from_counts):
shared, query_size and containment must be equal exactly, ani within 1e-9 (the
tolerance tests/test_scale.py uses for the fused ANI, whose device pow is
within an ulp of the host's).  Every threshold sits midway between two adjacent
distinct containment values of the expected result, so no pair is decided by
rounding."""
import ctypes as C

import numpy as np
import pytest

import sksffi

pytestmark = pytest.mark.gpu

RATES = [0.0, 0.005, 0.01, 0.02, 0.03, 0.05]
N_ANC = 8
EMPTY = 5  # bases of a segment too short for any window: an empty sketch


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.close()


def _spec(i, salt):
    """Genome i of a set: (length, ancestor seed, mutation seed, rate)."""
    return (20000 + (i * 997 + salt * 131) % 20001, 100 + (i + salt) % N_ANC, 1000 * (salt + 1) + i,
            RATES[(i // N_ANC + salt) % len(RATES)])


def _build(torch, ctx, specs, w, mask, kind, param, flavour=0):
    offs = [0]
    for L, _, _, _ in specs:
        offs.append(offs[-1] + L + 1)
    dev = torch.full((offs[-1],), ord("\n"), dtype=torch.uint8, device="cuda:0")
    for g, (L, seed, mseed, rate) in enumerate(specs):
        ctx.synth_bases(dev.data_ptr() + offs[g], L, seed, mseed, rate)
    torch.cuda.synchronize()
    return ctx.sketch_build(dev.data_ptr(), offs[-1], offs, w, mask, kind, param, flavour=flavour)


def _keys(ss):
    """Each sketch of the set as a 1-D array intersect1d can compare."""
    out = []
    for i in range(ss.n):
        a = np.ascontiguousarray(ss.sketch(i))
        out.append(a[:, 0].copy() if ss.elem_words == 1
                   else a.view([("lo", "<u8"), ("hi", "<u8")]).ravel())
    return out


def _shared(qk, rk):
    m = np.zeros((len(qk), len(rk)), dtype=np.int32)
    for i, a in enumerate(qk):
        if len(a):
            for j, b in enumerate(rk):
                if len(b):
                    m[i, j] = len(np.intersect1d(a, b, assume_unique=True))
    return m


def _expected(shared, qsizes, k, min_containment=0.0, min_shared=1):
    q, r = np.nonzero(shared >= max(min_shared, 1))  # row-major: ascending (query, ref)
    sh = shared[q, r].astype(np.int32)
    sz = qsizes[q].astype(np.int32)
    cont = sh.astype(np.float64) / sz.astype(np.float64)
    keep = cont >= min_containment
    q, r, sh, sz, cont = q[keep], r[keep], sh[keep], sz[keep], cont[keep]
    cont2, ani = sksffi.ani_from_counts(sh, sz, k)
    assert np.array_equal(cont2, cont)
    out = np.zeros(len(q), dtype=sksffi.HIT_DTYPE)
    out["query"], out["ref"], out["shared"], out["query_size"] = q, r, sh, sz
    out["containment"], out["ani"] = cont, ani
    return out


def _threshold(shared, qsizes):
    """Midpoint of the widest gap between adjacent distinct containment values of
    the sharing pairs; at least one sharing pair on each side, none within 1e-9."""
    q, r = np.nonzero(shared)
    cont = shared[q, r].astype(np.float64) / qsizes[q].astype(np.float64)
    u = np.unique(cont)
    assert len(u) >= 2
    g = int(np.argmax(np.diff(u)))
    thr = (u[g] + u[g + 1]) / 2
    assert np.abs(cont - thr).min() > 1e-9
    assert (cont >= thr).any() and (cont < thr).any()
    return thr


def _check(got, want):
    assert got.dtype == sksffi.HIT_DTYPE
    for f in ("query", "ref", "shared", "query_size", "containment"):
        assert np.array_equal(got[f], want[f]), f
    assert np.abs(got["ani"] - want["ani"]).max(initial=0.0) <= 1e-9


class Case:
    def __init__(self, torch, ctx, nq, nr, w, k, kind, param, r_param=None):
        self.w, self.k = w, k
        self.mask = sksffi.mask_generate(w, k, 0)
        qs = [_spec(i, 0) for i in range(nq)]
        rs = [_spec(i, 3) for i in range(nr)]
        qs[7] = (EMPTY,) + qs[7][1:]    # an empty query sketch
        rs[nr - 30] = (EMPTY,) + rs[nr - 30][1:]  # and an empty reference
        rs[24] = qs[0]                  # a reference that is a query's genome: full containment
        self.Q = _build(torch, ctx, qs, w, self.mask, kind, param)
        self.R = _build(torch, ctx, rs, w, self.mask, kind, r_param or param)
        self.qsizes = self.Q.sizes().astype(np.int64)
        self.shared = _shared(_keys(self.Q), _keys(self.R))
        assert self.qsizes[7] == 0 and self.R.sizes()[nr - 30] == 0
        nz = self.shared[self.shared > 0]
        # counts from nothing to everything
        assert (self.shared == 0).any() and (self.shared == self.qsizes[:, None])[self.qsizes > 0].any()
        assert len(np.unique(nz)) > 10

    def expected(self, **kw):
        return _expected(self.shared, self.qsizes, self.k, **kw)


@pytest.fixture(scope="module")
def frac(gpu):
    torch, ctx = gpu
    return Case(torch, ctx, 70, 130, 31, 21, sksffi.SKS_FRAC_MOD, 50)


@pytest.fixture(scope="module")
def bottom(gpu):
    torch, ctx = gpu
    return Case(torch, ctx, 70, 130, 31, 21, sksffi.SKS_BOTTOM_S, 256)


@pytest.fixture(scope="module")
def wide(gpu):
    torch, ctx = gpu
    return Case(torch, ctx, 70, 70, 45, 30, sksffi.SKS_FRAC_MOD, 50)


@pytest.mark.parametrize("which", ["frac", "bottom"])
def test_ragged_blocks(gpu, request, which):
    """70 x 130: both sets end in a partial 64-sketch block; no padding row or
    column appears, the hits are the expected list in (query, ref) order."""
    _, ctx = gpu
    case = request.getfixturevalue(which)
    thr = _threshold(case.shared, case.qsizes)
    got = ctx.search(case.Q, case.R, min_containment=thr)
    want = case.expected(min_containment=thr)
    assert 0 < len(want) < int((case.shared > 0).sum())
    _check(got, want)
    assert got["query"].max() < 70 and got["ref"].max() < 130
    key = got["query"].astype(np.uint64) << np.uint64(32) | got["ref"].astype(np.uint64)
    assert (np.diff(key.astype(np.int64)) > 0).all()
    # every sharing pair with both thresholds at their lowest
    _check(ctx.search(case.Q, case.R), case.expected())


def test_forced_batches(gpu, frac):
    """One and two reference blocks per batch (three and two batches of the 130
    references) give the default's array to the byte."""
    _, ctx = gpu
    thr = _threshold(frac.shared, frac.qsizes)
    base = ctx.search(frac.Q, frac.R, min_containment=thr)
    assert len(base)
    try:
        for blocks in (1, 2):
            ctx.set_search_batch(blocks)
            got = ctx.search(frac.Q, frac.R, min_containment=thr)
            assert got.tobytes() == base.tobytes(), blocks
    finally:
        ctx.set_search_batch(0)


def test_wide_kmers(gpu, wide):
    """w=45 / k=30: 128-bit k-mers (elem_words 2), 70 x 70."""
    _, ctx = gpu
    assert wide.Q.elem_words == 2
    thr = _threshold(wide.shared, wide.qsizes)
    _check(ctx.search(wide.Q, wide.R, min_containment=thr), wide.expected(min_containment=thr))
    try:
        ctx.set_search_batch(1)
        _check(ctx.search(wide.Q, wide.R), wide.expected())
    finally:
        ctx.set_search_batch(0)


def _dense_rows(torch, ctx, ss, rows):
    out = torch.zeros((rows, ss.n), dtype=torch.int32, device="cuda:0")
    data, starts, sizes = ss.device_ptrs()
    ctx.intersect_all(data, starts, sizes, ss.elem_words, ss.n, 0, rows, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_matches_dense_engine(gpu, frac):
    """The hits at the lowest thresholds are the non-zero cells of what the
    all-vs-all engine counts for concat(Q, R); a set against itself gives the
    non-zero cells of its own matrix; the device-array form agrees."""
    torch, ctx = gpu
    nq, nr = frac.Q.n, frac.R.n
    cat = ctx.concat([frac.Q, frac.R])
    dense = _dense_rows(torch, ctx, cat, nq)[:, nq:nq + nr]
    assert np.array_equal(dense, frac.shared)
    got = ctx.search(frac.Q, frac.R, min_containment=0.0, min_shared=1)
    q, r = np.nonzero(dense)
    assert np.array_equal(got["query"], q) and np.array_equal(got["ref"], r)
    assert np.array_equal(got["shared"], dense[q, r])
    own = _dense_rows(torch, ctx, frac.R, nr)
    got = ctx.search(frac.R, frac.R)
    q, r = np.nonzero(own)
    assert np.array_equal(got["query"], q) and np.array_equal(got["ref"], r)
    assert np.array_equal(got["shared"], own[q, r])
    assert np.array_equal(got["query_size"], frac.R.sizes().astype(np.int32)[q])

    def arrays(ss):
        sz = ss.sizes().astype(np.int64)
        return ss.device_ptrs() + (ss.n, int(sz.max()), int(sz.sum()))
    thr = _threshold(frac.shared, frac.qsizes)
    want = ctx.search(frac.Q, frac.R, min_containment=thr)
    try:
        for blocks in (0, 1):  # group bounds sampled from the references, reused by every batch
            ctx.set_search_batch(blocks)
            got = ctx.search_arrays(arrays(frac.Q), arrays(frac.R), 1, frac.k, min_containment=thr)
            assert got.tobytes() == want.tobytes()
    finally:
        ctx.set_search_batch(0)


def test_edge_sets(gpu, frac):
    torch, ctx = gpu
    got = ctx.search(frac.Q, frac.R)
    assert 7 not in got["query"] and (frac.R.n - 30) not in got["ref"]
    # no queries / no references: SKS_OK and no hits
    sz = frac.R.sizes().astype(np.int64)
    some = frac.R.device_ptrs() + (frac.R.n, int(sz.max()), int(sz.sum()))
    none = (0, 0, 0, 0, 0, 0)
    assert len(ctx.search_arrays(none, some, 1, frac.k)) == 0
    assert len(ctx.search_arrays(some, none, 1, frac.k)) == 0
    # min_shared alone, between two observed counts
    u = np.unique(frac.shared[frac.shared > 0])
    ms = int(u[len(u) // 2])
    assert u[len(u) // 2 - 1] < ms
    got = ctx.search(frac.Q, frac.R, min_containment=0.0, min_shared=ms)
    want = frac.expected(min_shared=ms)
    assert 0 < len(want) < int((frac.shared > 0).sum())
    _check(got, want)
    # min_shared below 1 never lets pairs that share nothing in
    _check(ctx.search(frac.Q, frac.R, min_containment=-1.0, min_shared=-5), frac.expected())


def test_capacity(gpu, frac):
    torch, ctx = gpu
    thr = _threshold(frac.shared, frac.qsizes)
    want = frac.expected(min_containment=thr)
    rc, n = ctx.search_sets_raw(frac.Q, frac.R, thr, 1, 0, 0)
    assert (rc, n) == (sksffi.SKS_OK, len(want))
    buf = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    rc, n2 = ctx.search_sets_raw(frac.Q, frac.R, thr, 1, buf.data_ptr(), n - 1)
    assert (rc, n2) == (sksffi.SKS_E_LENGTH, n)
    with pytest.raises(sksffi.SksError) as e:
        sksffi.check(rc)
    assert e.value.code == 6
    rc, n3 = ctx.search_sets_raw(frac.Q, frac.R, thr, 1, buf.data_ptr(), n)
    assert (rc, n3) == (sksffi.SKS_OK, n)
    ctx.synchronize()
    _check(buf.cpu().numpy().view(sksffi.HIT_DTYPE), want)


def test_incompatible_sets(gpu):
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
        with pytest.raises(sksffi.SksError, match=field) as e:
            ctx.search(base, other)
        assert e.value.code == 1, field
    n = C.c_uint64(7)
    assert sksffi.lib().sks_search_sets(ctx.h, base.h, None, 0.0, 1, None, 0, C.byref(n)) == 1


def test_invalid_layout_reports_no_hits(gpu, monkeypatch):
    """128-bit values whose 64-bit layout mixes all collide (the recipe of
    tests/test_join_dedup.py::test_layout_invalid_flag_reaches_all_vs_all) make
    the layout build raise its status word 1 at group cap 64: the search returns
    SKS_E_UNSUPPORTED and a hit count of 0 instead of hits from such a layout."""
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
    nh = C.c_uint64(99)
    v = C.c_void_p
    rc = sksffi.lib().sks_search(ctx.h, v(side[0]), v(side[1]), v(side[2]), n, side[4], side[5],
                                 v(side[0]), v(side[1]), v(side[2]), n, side[4], side[5], 2, 30, 0.0, 1, None, 0,
                                 C.byref(nh))
    assert rc == sksffi.SKS_E_UNSUPPORTED and nh.value == 0
    assert b"invalid layout" in sksffi.lib().sks_last_error()
    ctx.synchronize()


def test_bottom_s_of_different_s(gpu):
    """Bottom-128 queries against bottom-256 references: accepted and exact."""
    torch, ctx = gpu
    case = Case(torch, ctx, 70, 70, 31, 21, sksffi.SKS_BOTTOM_S, 128, r_param=256)
    assert case.Q.info()["param"] == 128 and case.R.info()["param"] == 256
    thr = _threshold(case.shared, case.qsizes)
    _check(ctx.search(case.Q, case.R, min_containment=thr), case.expected(min_containment=thr))


# ---- few queries against many large references ---------------------------------------------------
# The shape sks-search exists for.  The query layout and each reference batch's
# layout take their region size from their own block count
# (join_layout_region_log), so one block of queries against batches of 2 or of 4
# and more blocks joins layouts of different region sizes in one k_join launch:
# a window of 64 buckets is four regions of the rows and two or one of the
# columns.  Sketches of more than 21 760 elements put the layouts at 2^14
# buckets, where those region logs are 1, 2 and 3.

LARGE_RATES = [0.0, 0.002, 0.01, 0.03]
_LARGE_HOST = {}  # (nr, w, k) -> (qsizes, rsizes, shared): the host side, computed once per process


def _shared_indexed(Q, R):
    """shared[q, r] with the references indexed once: the lo words of all their
    elements with the owning reference, one sort.  A query element's candidates
    are the run of equal lo words; it is shared with those whose hi word is
    equal too (hi is 0 for 64-bit elements)."""
    parts = [R.sketch(j) for j in range(R.n)]
    owner = np.repeat(np.arange(R.n), [len(p) for p in parts])
    allr = np.concatenate(parts)
    order = np.argsort(allr[:, 0], kind="stable")
    slo, shi, sown = allr[order, 0], allr[order, 1], owner[order]
    shared = np.zeros((Q.n, R.n), dtype=np.int32)
    for i in range(Q.n):
        a = Q.sketch(i)
        if not len(a):
            continue
        b = np.searchsorted(slo, a[:, 0], "left")
        cnt = np.searchsorted(slo, a[:, 0], "right") - b
        idx = np.repeat(b - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
        ok = shi[idx] == np.repeat(a[:, 1], cnt)
        shared[i] = np.bincount(sown[idx[ok]], minlength=R.n)
    return shared


class LargeCase:
    """6 queries (one empty, one a reference's genome, one related to nothing)
    against nr references of 23-26 kb in families of 6 ancestors at rates
    0 .. 0.03, FracMinHash c = 1: every sketch holds about 23 000 elements."""

    def __init__(self, torch, ctx, nr, w, k):
        self.w, self.k = w, k
        self.mask = sksffi.mask_generate(w, k, 0)
        length = lambda i: 23000 + (i * 997) % 3001  # noqa: E731
        qs = [(length(0), 200, 0, 0.0), (length(1), 201, 7001, 0.01), (EMPTY, 202, 0, 0.0),
              (length(3), 202, 7003, 0.03), (length(4), 203, 0, 0.0), (length(5), 299, 0, 0.0)]
        rs = [(length(i + 7), 200 + i % 6, 8000 + i, LARGE_RATES[(i // 6) % len(LARGE_RATES)]) for i in range(nr)]
        rs[24] = qs[0]                            # a reference that is a query's genome
        rs[nr - 30] = (EMPTY,) + rs[nr - 30][1:]  # and an empty reference
        self.Q = _build(torch, ctx, qs, w, self.mask, sksffi.SKS_FRAC_MOD, 1)
        self.R = _build(torch, ctx, rs, w, self.mask, sksffi.SKS_FRAC_MOD, 1)
        qsizes, rsizes = self.Q.sizes().astype(np.int64), self.R.sizes().astype(np.int64)
        key = (nr, w, k)
        if key not in _LARGE_HOST:
            shared = _shared_indexed(self.Q, self.R)
            # the index against the pairwise reference of this file, on a corner
            assert np.array_equal(shared[:2, 23:26], _shared(_keys(self.Q)[:2], _keys(self.R)[23:26]))
            _LARGE_HOST[key] = (qsizes, rsizes, shared)
        self.qsizes, self.rsizes, self.shared = _LARGE_HOST[key]
        assert np.array_equal(qsizes, self.qsizes) and np.array_equal(rsizes, self.rsizes)  # the same sets again
        # the premise: 2^14 buckets, and a region log per block count
        assert qsizes[2] == 0 and rsizes[nr - 30] == 0 and rsizes[rsizes > 0].min() > 21760
        assert sksffi.join_layout_log_b(int(max(qsizes.max(), rsizes.max()))) == 14
        assert [sksffi.join_layout_region_log(b, 14) for b in (1, 2, 4, 6)] == [1, 2, 3, 3]
        # from nothing to everything
        # (unrelated genomes of this size can share a chance k-mer or two)
        assert self.shared[0, 24] == qsizes[0] and self.shared[5].sum() <= 3 and not self.shared[2].any()
        assert self.shared[:, 4::6].sum() <= 3 and len(np.unique(self.shared[self.shared > 0])) > 10

    def expected(self, **kw):
        return _expected(self.shared, self.qsizes, self.k, **kw)


@pytest.fixture(scope="module")
def large(gpu):
    torch, ctx = gpu
    return LargeCase(torch, ctx, 330, 31, 21)


def test_few_queries_many_large_references(gpu, large):
    """6 x 330 at 2^14 buckets: one query block (region log 1) against the six
    reference blocks in one batch (3), one block a batch (1), two (2), and four
    then two (3 and 2 in one call).  Every run is the host's list."""
    _, ctx = gpu
    assert large.Q.n == 6 and (large.R.n + 63) // 64 == 6 and large.R.n % 64
    want = large.expected()
    assert len(want) > 200
    try:
        for blocks in (0, 1, 2, 4):
            ctx.set_search_batch(blocks)
            _check(ctx.search(large.Q, large.R), want)
    finally:
        ctx.set_search_batch(0)


def test_few_queries_many_large_references_wide(gpu):
    """The same at w = 45 / k = 30 (128-bit elements): four reference blocks in
    one batch, region log 3 against the queries' 1."""
    torch, ctx = gpu
    case = LargeCase(torch, ctx, 230, 45, 30)
    assert case.Q.elem_words == 2 and (case.R.n + 63) // 64 == 4
    _check(ctx.search(case.Q, case.R), case.expected())
