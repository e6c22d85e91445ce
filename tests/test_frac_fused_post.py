"""The fused post-processing of one narrow FracMinHash genome (build.cpp
build_frac_single, post.hip k_frac_partition / k_frac_sort_unique /
k_frac_gather) against the oracle, bit-exactly: sketch, size and windows.

The path splits the scan's survivors by their top key bits into buckets of at
most 4096 keys (one partition workgroup of 1024 threads per 16384 records of
capacity), sorts and uniques each bucket in one workgroup with a register tile
of 4, 8 or 16 keys per thread, and gathers the buckets.  A bucket over
its capacity, or keys crowding one sub-bucket of a bucket's sort, is a status:
the general post-processing then runs on the same scan records.  A scan that
overflows its record region is rescanned by the general build.  The cases sit
at these capacities (lowered through sks_ctx_set_frac_post where the default
would need a large genome) and assert the path taken where the case is about
it.  c = 1 keeps every window."""
import threading

import numpy as np
import pytest

import pyoracle as O
import sksffi
import synth

pytestmark = pytest.mark.gpu

ROW = 1024         # threads of a partition workgroup
PART = 16384       # record capacity per partition workgroup
BUCKET = 4096      # keys per bucket
GENERAL, FUSED, FUSED_THEN_GENERAL = (sksffi.BUILD_PATH_GENERAL, sksffi.BUILD_PATH_FUSED,
                                      sksffi.BUILD_PATH_FUSED_THEN_GENERAL_POST)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.close()


@pytest.fixture(autouse=True)
def _default_controls(gpu):
    yield
    gpu[1].set_frac_post(sksffi.FRAC_POST_AUTO, 0, 0)


_oracle_cache = {}


def _oracle(g, w, m, c, flavour=0):
    key = (g, w, m, c, flavour)
    if key not in _oracle_cache:
        _oracle_cache[key] = O.sketch(O.cut_runs(g), w, m, "frac", c, 1, flavour)
    return _oracle_cache[key]


def _build(torch, ctx, g, w, m, c, flavour=0):
    stream = g + b"\n"
    dev = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
    return ctx.sketch_build(dev.data_ptr(), len(stream), [0, len(stream)], w, m, sksffi.SKS_FRAC_MOD, c, 1,
                            flavour)


def _check(gpu, g, w, m, c, flavour=0, path=None):
    torch, ctx = gpu
    ss = _build(torch, ctx, g, w, m, c, flavour)
    want, nw = _oracle(g, w, m, c, flavour)
    tag = (len(g), w, c, flavour)
    assert int(ss.windows()[0]) == nw, tag
    assert int(ss.sizes()[0]) == len(want), tag
    assert np.array_equal(ss.sketch(0), want), tag
    if path is not None:
        assert ctx.last_build_path() == path, (tag, ctx.last_build_path())
    return ss


# ---- 1. window and mask shapes ---------------------------------------------------------------
@pytest.fixture(scope="module")
def genome70k():
    return synth.bases(70000, seed=611).tobytes()


@pytest.mark.parametrize("w,k", [(31, 21), (32, 32), (32, 20), (16, 11), (2, 2), (1, 1)])
def test_window_and_mask_shapes(gpu, genome70k, w, k):
    """Key widths from 64 bits down to 2 (fewer key bits than bucket bits: the
    bucket is the key itself, and c = 1 then overfills it: status path), both
    hash flavours; c = 1 keeps every window so many buckets fill, an even c runs
    the pre-filter scan and an odd c the plain one.  The 4 or 16 k-mers of the
    two shortest windows survive whole or not at all at c > 1, so those builds
    may also overflow the scan's region (general path)."""
    m = O.mask(w, k, 3)
    for flavour in (0, 1):
        for c in (1, 8, 1000, 7):
            _check(gpu, genome70k, w, m, c, flavour, path=(FUSED if c == 1 and k > 11 else None))


# ---- 2. survivor counts at the capacities ----------------------------------------------------
W, K = 31, 21


def _clean(n_survivors, seed):
    """A clean genome with n_survivors windows (c = 1 keeps them all)."""
    return synth.bases(n_survivors + W - 1 if n_survivors else W - 1, seed=seed).tobytes()


def test_tiny_counts(gpu):
    m = O.mask(W, K, 0)
    _check(gpu, b"", W, m, 1, path=FUSED)  # only the separator
    torch, ctx = gpu
    dev = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    ss = ctx.sketch_build(dev.data_ptr(), 16, [0, 0], W, m, sksffi.SKS_FRAC_MOD, 1)  # an empty segment
    assert int(ss.sizes()[0]) == 0 and int(ss.windows()[0]) == 0 and len(ss.sketch(0)) == 0
    assert ctx.last_build_path() == FUSED
    for n in (0, 1, 2):
        ss = _check(gpu, _clean(n, 700 + n), W, m, 1, path=FUSED)
        assert int(ss.windows()[0]) == n
    _check(gpu, _clean(0, 710), W, m, 1000, path=FUSED)


@pytest.mark.parametrize("buckets", [0, 1])
def test_partition_workgroup_edges(gpu, buckets):
    """One below, at and above one row of a partition workgroup (its 1024 threads
    take a record each) and three rows, with the default bucket count and with
    one bucket; and, with the default buckets, around the record capacity at
    which a second and a third workgroup share the rows (the region's capacity at
    c = 1 is the genome's length + 1 = survivors + W)."""
    m = O.mask(W, K, 0)
    gpu[1].set_frac_post(sksffi.FRAC_POST_AUTO, 0, buckets)
    # one bucket: 1024 and 2048 keys are also the edges of the sort's register tiles
    sizes = [ROW - 1, ROW, ROW + 1, 2 * ROW, 2 * ROW + 1, 3 * ROW - 1, 3 * ROW + 1]
    if buckets == 0:
        sizes += [PART - W - 1, PART - W, PART - W + 1, PART + ROW + 1, 2 * PART - W + 1]
    for n in sizes:
        _check(gpu, _clean(n, 720 + n % 7), W, m, 1, path=FUSED)


@pytest.mark.parametrize("cap", [64, BUCKET])
def test_bucket_capacity_edges(gpu, cap):
    """One bucket of capacity `cap`: cap - 1 and cap keys are sorted by its
    workgroup, cap + 1 is a status (never a store) and the general
    post-processing finishes the build from the same scan."""
    m = O.mask(W, K, 0)
    torch, ctx = gpu
    ctx.set_frac_post(sksffi.FRAC_POST_AUTO, cap, 1)
    for n, path in ((cap - 1, FUSED), (cap, FUSED), (cap + 1, FUSED_THEN_GENERAL)):
        _check(gpu, _clean(n, 730 + n % 5), W, m, 1, path=path)
        assert ctx.timings()["scan_launches"] == 1
        assert ctx.timings()["survivors"] == n


def test_runs_cut_by_n(gpu):
    g = synth.bases(70000, seed=741)
    g[::5000] = ord("N")
    g = g.tobytes()
    m = O.mask(W, K, 0)
    for c in (1, 8):
        _check(gpu, g, W, m, c, path=FUSED)


# ---- 3. duplicates ---------------------------------------------------------------------------
def test_duplicates(gpu):
    """Two copies of a 30 kb sequence: every key twice in its bucket, uniqued by
    the bucket's workgroup.  A 37-base unit 4000 times: at most 37 distinct keys
    4000 times each, which crowd their sub-buckets (status path)."""
    m = O.mask(W, K, 0)
    one = synth.bases(30000, seed=751).tobytes()
    for c in (1, 8):
        ss = _check(gpu, one + b"N" + one, W, m, c, path=FUSED)
        assert int(ss.sizes()[0]) < gpu[1].timings()["survivors"]
    unit = synth.bases(37, seed=752).tobytes()
    ss = _check(gpu, unit * 4000, W, m, 1, path=FUSED_THEN_GENERAL)
    assert int(ss.sizes()[0]) <= 37


# ---- 4. fallbacks ----------------------------------------------------------------------------
def test_homopolymer_status_path(gpu):
    """300 000 windows, one key: its bucket overflows; status, then the general
    post-processing on the same records."""
    m = O.mask(31, 31, 0)
    ss = _check(gpu, b"A" * 300000, 31, m, 1, path=FUSED_THEN_GENERAL)
    assert int(ss.sizes()[0]) == 1
    assert gpu[1].timings()["scan_launches"] == 1


def test_homopolymer_scan_region_overflow(gpu):
    """At a c that divides the one k-mer's fmh every window survives where 1 / c
    of them were expected: the record region overflows and the general build
    rescans with the counted capacity.  (The smallest divisor of this mask's fmh
    is 35201 for the boost-mix flavour and 2 for the legacy one; either leaves a
    region of a few thousand records for 299 970 survivors.)"""
    w = k = 31
    m = O.mask(w, k, 0)
    for flavour in (0, 1):
        f = O.frac_min_hash(0, m, w, 1, flavour)  # the canonical k-mer of A...A / T...T is 0
        c = next(d for d in range(2, 100000) if f % d == 0)
        ss = _check(gpu, b"A" * 300000, w, m, c, flavour, path=GENERAL)
        assert int(ss.sizes()[0]) == 1
        assert gpu[1].timings()["scan_launches"] > 1


def test_forced_small_capacity_status_path(gpu):
    g = synth.bases(200000, seed=761).tobytes()
    gpu[1].set_frac_post(sksffi.FRAC_POST_AUTO, 64, 0)
    _check(gpu, g, W, O.mask(W, K, 0), 8, path=FUSED_THEN_GENERAL)


# ---- 5. old and new path ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def genomes300k():
    return [synth.bases(300000, seed=770 + i).tobytes() for i in range(3)]


def test_forced_paths_agree(gpu, genomes300k):
    torch, ctx = gpu
    m = O.mask(W, K, 0)
    ctx.set_frac_post(sksffi.FRAC_POST_GENERAL, 0, 0)
    old = _check(gpu, genomes300k[0], W, m, 8, path=GENERAL)
    ctx.set_frac_post(sksffi.FRAC_POST_FUSED, 0, 0)
    new = _check(gpu, genomes300k[0], W, m, 8, path=FUSED)
    assert np.array_equal(old.sketch(0), new.sketch(0))
    assert np.array_equal(old.sizes(), new.sizes()) and np.array_equal(old.windows(), new.windows())
    assert np.array_equal(old.starts(), new.starts())


# ---- 6. contexts in flight -------------------------------------------------------------------
def test_three_contexts_in_flight(gpu, genomes300k):
    """Three contexts, each on its own stream and host thread, each building its
    own genome four times: the scratch (regions, cursors, status) is per context."""
    torch, _ = gpu
    m = O.mask(W, K, 0)
    devs = [torch.frombuffer(bytearray(g + b"\n"), dtype=torch.uint8).to("cuda:0") for g in genomes300k]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in genomes300k]
    ctxs = [sksffi.Context(0, s.cuda_stream) for s in streams]
    got = [[] for _ in genomes300k]
    errors = []

    def work(i):
        try:
            for _ in range(4):
                ss = ctxs[i].sketch_build(devs[i].data_ptr(), devs[i].numel(), [0, devs[i].numel()], W, m,
                                          sksffi.SKS_FRAC_MOD, 8)
                got[i].append((ss.sketch(0), int(ss.windows()[0]), ctxs[i].last_build_path()))
                ss.free(streams[i].cuda_stream)
        except Exception as e:  # surfaced below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(ctxs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    for c in ctxs:
        c.close()
    assert not errors, errors
    for i, g in enumerate(genomes300k):
        want, nw = _oracle(g, W, m, 8)
        assert len(got[i]) == 4
        for sk, wins, path in got[i]:
            assert path == FUSED
            assert wins == nw
            assert np.array_equal(sk, want)


# ---- 7. the set's device arrays --------------------------------------------------------------
def test_export_and_union(gpu, genomes300k):
    """sks_sketch_set_export reads the set's device sizes and starts, which the
    gather kernel wrote; the union of two such sets' exported rows equals the
    union of the oracle's sketches."""
    torch, ctx = gpu
    m = O.mask(W, K, 0)
    rows, sizes = [], []
    for g in genomes300k[:2]:
        ss = _check(gpu, g, W, m, 8, path=FUSED)
        n = int(ss.sizes()[0])
        stride = n + 5
        d = torch.zeros(stride, dtype=torch.int64, device="cuda:0")
        dn = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        ss.export(d.data_ptr(), stride, dn.data_ptr())
        want, _ = _oracle(g, W, m, 8)
        assert int(dn.cpu()[0]) == n == len(want)
        host = d.cpu().numpy().view(np.uint64)
        assert np.array_equal(host[:n], want[:, 0])
        assert (host[n:] == np.uint64(2**64 - 1)).all()
        rows.append(d[:n])
        sizes.append(n)
    both = torch.cat(rows).contiguous()
    out = torch.zeros_like(both)
    torch.cuda.synchronize()
    k = ctx.sketch_union(both.data_ptr(), both.numel(), out.data_ptr())
    torch.cuda.synchronize()
    want = np.union1d(_oracle(genomes300k[0], W, m, 8)[0][:, 0], _oracle(genomes300k[1], W, m, 8)[0][:, 0])
    assert k == len(want)
    assert np.array_equal(out[:k].cpu().numpy().view(np.uint64), want)
