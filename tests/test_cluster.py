"""Single-linkage clusters on the device (sks_cluster / sks_cluster_set).

Genomes are synthetic (sks_synth_bases), 29-31 kb: genome i belongs to family
i % 8, whose first member is the ancestor (rate 0) and whose later members are
descendants at substitution rates 0.01 and 0.02, each with a mutation seed of
its own.  With k = 21 an ancestor keeps about 0.81 / 0.65 of its k-mers in such
a descendant, two 0.01 siblings share about 0.66, a 0.01 and a 0.02 sibling
0.53 and two 0.02 siblings 0.43, so a threshold between those values links
some siblings only through a third genome.  One segment is too short for any
window (an empty sketch).  The mutation seeds were chosen, with the CPU oracle,
so that both sketch kinds meet the preconditions test_matches_host asserts.

The expected labels come from the host (tests/cluster_ref.py): the sketches
copied out of the device set, np.intersect1d per pair, the link rule in float64 (shared / size for both
sketches of the pair), a plain union-find, clusters numbered by ascending
smallest member, representatives by (size, -index).  The threshold is the
midpoint of the widest gap between adjacent distinct values of
shared / min(size_i, size_j) over the sharing pairs, so no pair is decided by
rounding.  Labels, representatives and the cluster count must be exactly
equal."""
import ctypes as C

import numpy as np
import pytest

import sksffi
from cluster_ref import components, keys_of, links, shared_matrix, threshold

pytestmark = pytest.mark.gpu

N_FAM = 8
EMPTY = 5            # bases of a segment too short for any window: an empty sketch
EMPTY_AT = 77
LATE = (1, 9)        # the generations (i // 8) at rate 0.02; the others descend at 0.01
# Every bottom-256 sketch of a 20-40 kb genome holds exactly 256 elements, so a
# representative could never differ from its cluster's first member.  The
# bottom-s case therefore replaces three genomes by a family of their own, short
# enough (fewer than 256 windows) that their sketches hold all their k-mers and
# differ in size: genome -> (length, rate).  (Under FracMinHash 1/50 they would
# hold four or five elements, whose coarse ratios would decide the threshold.)
TRIO = {3: (200, 0.0), 11: (235, 0.01), 19: (270, 0.02)}
TRIO_SEED = 399


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.close()


def spec(i, trio=False):
    """Genome i: (length, ancestor seed, mutation seed, rate)."""
    if trio and i in TRIO:
        return (TRIO[i][0], TRIO_SEED, 7400 + i, TRIO[i][1])
    gen = i // N_FAM
    rate = 0.0 if gen == 0 else (0.02 if gen in LATE else 0.01)
    length = EMPTY if i == EMPTY_AT else 29000 + (i * 997) % 2001
    return (length, 300 + i % N_FAM, 7400 + i, rate)


def _build(torch, ctx, specs, w, mask, kind, param):
    offs = [0]
    for L, _, _, _ in specs:
        offs.append(offs[-1] + L + 1)
    dev = torch.full((offs[-1],), ord("\n"), dtype=torch.uint8, device="cuda:0")
    for g, (L, seed, mseed, rate) in enumerate(specs):
        ctx.synth_bases(dev.data_ptr() + offs[g], L, seed, mseed, rate)
    torch.cuda.synchronize()
    return ctx.sketch_build(dev.data_ptr(), offs[-1], offs, w, mask, kind, param)


def check_preconditions(labels, reps, link, sizes, n):
    """What test_matches_host needs of its input to mean anything."""
    C_ = len(reps)
    assert 1 < C_ < n
    same = labels[:, None] == labels[None, :]
    off = ~np.eye(n, dtype=bool)
    assert (same & ~link & off).any(), "no cluster has two members that are not directly linked"
    blocks = [set(labels[b:min(n, b + 64)].tolist()) for b in range(0, n, 64)]
    assert len(blocks) == 3 and set.intersection(*blocks), "no cluster has members in all three blocks"
    first = np.array([int(np.nonzero(labels == c)[0][0]) for c in range(C_)])
    assert (reps != first).any(), "every representative is its cluster's smallest index"
    assert sizes[EMPTY_AT] == 0 and (labels == labels[EMPTY_AT]).sum() == 1


class Case:
    def __init__(self, torch, ctx, n, w, k, kind, param, trio=False):
        self.n, self.w, self.k = n, w, k
        self.mask = sksffi.mask_generate(w, k, 0)
        self.S = _build(torch, ctx, [spec(i, trio) for i in range(n)], w, self.mask, kind, param)
        self.sizes = self.S.sizes().astype(np.int64)
        self.shared = shared_matrix(keys_of(self.S))
        self.thr = threshold(self.shared, self.sizes)

    def expected(self, min_containment=None, min_shared=1):
        thr = self.thr if min_containment is None else min_containment
        link = links(self.shared, self.sizes, thr, min_shared)
        return components(link, self.sizes) + (link,)


@pytest.fixture(scope="module")
def frac(gpu):
    torch, ctx = gpu
    return Case(torch, ctx, 130, 31, 21, sksffi.SKS_FRAC_MOD, 50)


@pytest.fixture(scope="module")
def bottom(gpu):
    torch, ctx = gpu
    return Case(torch, ctx, 130, 31, 21, sksffi.SKS_BOTTOM_S, 256, trio=True)


@pytest.fixture(scope="module")
def wide(gpu):
    torch, ctx = gpu
    return Case(torch, ctx, 70, 45, 30, sksffi.SKS_FRAC_MOD, 50)


def _same(got, want):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], want[0]), "labels"
    assert np.array_equal(got[1], want[1]), "representatives"


@pytest.mark.parametrize("which", ["frac", "bottom"])
def test_matches_host(gpu, request, which):
    """n = 130: three blocks with 2 sketches in the last.  Labels,
    representatives and the cluster count equal the host's."""
    _, ctx = gpu
    case = request.getfixturevalue(which)
    labels, reps, link = case.expected()
    check_preconditions(labels, reps, link, case.sizes, case.n)
    got = ctx.cluster(case.S, min_containment=case.thr)
    print(which, "threshold", case.thr, "clusters", len(reps), "got", len(got[1]))
    _same(got, (labels, reps))
    assert got[0][0] == 0 and len(got[1]) == len(reps)


def test_matches_search_hits(gpu, frac):
    """The components of the (query, ref) list that search(S, S) reports at the
    same thresholds are the clusters."""
    _, ctx = gpu
    hits = ctx.search(frac.S, frac.S, min_containment=frac.thr)
    link = np.zeros((frac.n, frac.n), dtype=bool)
    link[hits["query"], hits["ref"]] = True
    link |= link.T
    np.fill_diagonal(link, False)
    assert link.any()
    _same(ctx.cluster(frac.S, min_containment=frac.thr), components(link, frac.sizes))


def test_forced_batches(gpu, frac):
    """One and two column blocks per batch (three and two batches of the three
    blocks) give the default's arrays to the byte."""
    _, ctx = gpu
    base = ctx.cluster(frac.S, min_containment=frac.thr)
    assert 1 < len(base[1]) < frac.n
    try:
        for blocks in (1, 2):
            ctx.set_search_batch(blocks)
            got = ctx.cluster(frac.S, min_containment=frac.thr)
            assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), blocks
    finally:
        ctx.set_search_batch(0)


def test_wide_kmers(gpu, wide):
    """w=45 / k=30: 128-bit k-mers (elem_words 2), n = 70, default and batch 1."""
    _, ctx = gpu
    assert wide.S.elem_words == 2
    want = wide.expected()[:2]
    assert 1 < len(want[1]) < wide.n
    _same(ctx.cluster(wide.S, min_containment=wide.thr), want)
    try:
        ctx.set_search_batch(1)
        _same(ctx.cluster(wide.S, min_containment=wide.thr), want)
    finally:
        ctx.set_search_batch(0)


def test_extremes(gpu, frac):
    torch, ctx = gpu
    n = frac.n
    # 130 copies of one genome: every cell of every tile links, one cluster, representative 0
    one = _build(torch, ctx, [(30000, 41, 0, 0.0)] * n, 31, frac.mask, sksffi.SKS_FRAC_MOD, 50)
    labels, reps = ctx.cluster(one, min_containment=1.0)
    assert one.sizes().min() > 0
    assert np.array_equal(labels, np.zeros(n, dtype=np.uint32)) and np.array_equal(reps, [0])
    # a threshold no pair can meet: labels and representatives are the identity
    labels, reps = ctx.cluster(frac.S, min_containment=2.0)
    assert np.array_equal(labels, np.arange(n)) and np.array_equal(reps, np.arange(n))
    # min_shared alone, between two observed counts
    u = np.unique(frac.shared[frac.shared > 0])
    ms = int(u[len(u) // 2])
    assert u[len(u) // 2 - 1] < ms
    want = frac.expected(min_containment=0.0, min_shared=ms)[:2]
    every = frac.expected(min_containment=0.0)[:2]
    assert len(every[1]) < len(want[1]) < n
    _same(ctx.cluster(frac.S, min_containment=0.0, min_shared=ms), want)
    # thresholds below their lowest: every sharing pair links, no other
    _same(ctx.cluster(frac.S, min_containment=-1.0, min_shared=-5), every)
    # either output may be NULL: the count still comes back
    lab = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    rep = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    want = frac.expected()[:2]
    assert ctx.cluster_set_raw(frac.S, frac.thr, 1, 0, 0) == (sksffi.SKS_OK, len(want[1]))
    assert ctx.cluster_set_raw(frac.S, frac.thr, 1, lab.data_ptr(), 0) == (sksffi.SKS_OK, len(want[1]))
    assert ctx.cluster_set_raw(frac.S, frac.thr, 1, 0, rep.data_ptr()) == (sksffi.SKS_OK, len(want[1]))
    ctx.synchronize()
    assert np.array_equal(lab.cpu().numpy().view(np.uint32), want[0])
    assert np.array_equal(rep.cpu().numpy().view(np.uint32)[:len(want[1])], want[1])
    # one sketch
    single = _build(torch, ctx, [spec(0)], 31, frac.mask, sksffi.SKS_FRAC_MOD, 50)
    labels, reps = ctx.cluster(single, min_containment=0.5)
    assert np.array_equal(labels, [0]) and np.array_equal(reps, [0])


def test_order_independent(gpu, frac):
    """The same genomes in a permuted order: the same partition under the
    permutation, canonically renumbered, with the same representatives."""
    torch, ctx = gpu
    n = frac.n
    perm = np.random.default_rng(5).permutation(n)  # new position p holds genome perm[p]
    P = _build(torch, ctx, [spec(int(g)) for g in perm], 31, frac.mask, sksffi.SKS_FRAC_MOD, 50)
    assert np.array_equal(P.sizes().astype(np.int64), frac.sizes[perm])
    base_labels, base_reps = ctx.cluster(frac.S, min_containment=frac.thr)
    labels, reps = ctx.cluster(P, min_containment=frac.thr)
    # position p and q together iff genomes perm[p] and perm[q] are
    assert np.array_equal(labels[:, None] == labels[None, :],
                          base_labels[perm][:, None] == base_labels[perm][None, :])
    first = [int(np.nonzero(labels == c)[0][0]) for c in range(len(reps))]
    assert first == sorted(first) and labels[0] == 0 and len(reps) == len(base_reps)
    # the largest sketch of each cluster, ties to the smallest new position
    want_link = links(frac.shared[np.ix_(perm, perm)], frac.sizes[perm], frac.thr)
    _same((labels, reps), components(want_link, frac.sizes[perm]))


def test_many_small_sketches(gpu):
    """The array form on 4100 tiny sketches (65 blocks, 17 numbering chunks) with
    a closed-form answer: sketch i holds one value shared by the three sketches
    of group i // 3 and i % 3 values of its own; every 50th sketch is empty."""
    torch, ctx = gpu
    n = 4100
    sk = []
    for i in range(n):
        own = [10_000_000 + 4 * i + t for t in range(i % 3)]
        sk.append(np.array([] if i % 50 == 0 else sorted([1000 + i // 3] + own), dtype=np.uint64))
    sizes = np.array([len(x) for x in sk], dtype=np.uint32)
    starts = np.zeros(n, dtype=np.uint64)
    starts[1:] = np.cumsum(sizes[:-1], dtype=np.uint64)
    d = torch.from_numpy(np.concatenate(sk).view(np.int64)).to("cuda:0")
    st = torch.from_numpy(starts.view(np.int64)).to("cuda:0")
    sz = torch.from_numpy(sizes.view(np.int32)).to("cuda:0")
    side = (d.data_ptr(), st.data_ptr(), sz.data_ptr(), n, int(sizes.max()), int(sizes.sum()))
    # by arithmetic: an empty sketch is alone, the others of a group are one cluster
    want_labels, want_reps = np.zeros(n, dtype=np.uint32), []
    for g in range((n + 2) // 3):
        members = [i for i in range(3 * g, min(n, 3 * g + 3))]
        full = [i for i in members if i % 50 != 0]
        for i in members:  # ascending: an emptied first member comes before its group's cluster
            if i % 50 == 0:
                want_labels[i] = len(want_reps)
                want_reps.append(i)
            elif i == full[0]:
                want_labels[full] = len(want_reps)
                want_reps.append(full[-1])  # the member with the most values of its own
    # 1367 groups, and the 82 emptied sketches (each group keeps another member)
    assert len(want_reps) == 1367 + 82 and want_labels[n - 1] == len(want_reps) - 1
    got = ctx.cluster_arrays(side, 1, 21, min_containment=0.0, min_shared=1)
    _same(got, (want_labels, np.array(want_reps, dtype=np.uint32)))


def test_invalid_layout_links_nothing(gpu, monkeypatch):
    """128-bit values whose 64-bit layout mixes all collide (the recipe of
    tests/test_search.py::test_invalid_layout_reports_no_hits) make the layout
    build raise its status word 1 at group cap 64: sks_cluster returns
    SKS_E_UNSUPPORTED and 0 clusters instead of clusters from such a layout."""
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
    lab = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    rc, c = ctx.cluster_arrays_raw(side, 2, 30, 0.0, 1, lab.data_ptr(), 0)
    assert rc == sksffi.SKS_E_UNSUPPORTED and c == 0
    assert b"invalid layout" in sksffi.lib().sks_last_error()
    ctx.synchronize()


def test_argument_errors(gpu, frac):
    _, ctx = gpu
    L = sksffi.lib()
    sz = frac.sizes
    side = frac.S.device_ptrs() + (frac.n, int(sz.max()), int(sz.sum()))
    assert ctx.cluster_set_raw(frac.S, float("nan"), 1, 0, 0) == (sksffi.SKS_E_ARG, 0)
    assert ctx.cluster_arrays_raw(side, 1, 21, float("nan"), 1, 0, 0) == (sksffi.SKS_E_ARG, 0)
    assert ctx.cluster_set_raw(None, 0.5, 1, 0, 0) == (sksffi.SKS_E_ARG, 0)
    assert ctx.cluster_arrays_raw(side, 3, 21, 0.5, 1, 0, 0) == (sksffi.SKS_E_ARG, 0)
    assert ctx.cluster_arrays_raw(side, 1, 0, 0.5, 1, 0, 0) == (sksffi.SKS_E_ARG, 0)
    assert L.sks_cluster_set(ctx.h, frac.S.h, 0.5, 1, None, None, None) == sksffi.SKS_E_ARG
    v = C.c_void_p
    assert L.sks_cluster(ctx.h, v(side[0]), v(side[1]), v(side[2]), side[3], side[4], side[5], 1, 21, 0.5, 1,
                         None, None, None) == sksffi.SKS_E_ARG
    # >= 2^32 elements: refused before anything is launched
    big = side[:5] + (1 << 32,)
    assert ctx.cluster_arrays_raw(big, 1, 21, 0.5, 1, 0, 0) == (sksffi.SKS_E_UNSUPPORTED, 0)
    # no sketches: SKS_OK and no clusters
    assert ctx.cluster_arrays_raw((0, 0, 0, 0, 0, 0), 1, 21, 0.5, 1, 0, 0) == (sksffi.SKS_OK, 0)
