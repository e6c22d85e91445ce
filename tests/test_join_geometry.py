"""The join (join.hip k_join over layout.hip's layout) at forced work splits,
region sizes and launch slices, against numpy, count for count.

How a join call is cut up is decided on the host (csrc/join_plan.hpp): buckets
per workgroup, column entries per chunk, buckets per layout region, the
contiguous or the piecewise kernel, tiles per launch.  The knobs that force
these (SKS_JOIN_WGS, SKS_JOIN_CAP, SKS_LAYOUT_RG, SKS_JOIN_TILE_ORDER) are read
once per process, so each setting runs in a child process (this file as a
script, one at a time) that first asserts, through sks_join_launch_plan,
sks_join_layout_region_log and sks_join_layout_capacity, that it reached the
geometry it is there for, then runs one fixed battery:

* u64: 150 caller arrays in three families, one empty, 0 and 2^64 - 1 present,
  three sketches (two in one block, one in another) sharing 5000 values so a
  pair's count carries out of the 12 count planes where one workgroup holds
  enough buckets, four sketches of exactly 700 elements (the fused ANI's table
  rows).  sks_intersect_all whole and on rows 64..150 and 3..97;
  sks_intersect_sym in tile ranges (0, 2), (2, T); sks_join_layout_build +
  sks_intersect_sym_layout at the natural log_b and at log_b 0 and 3 (buckets
  far above the chunk capacity); sks_intersect_layout_tiles packed, over a
  layout of blocks 1.. with a tile list; sks_intersect_layout_ani, whose ANI
  equals sks_ani_rows on the same counts bit for bit (table rows and pow rows);
  one call of the check build with no violation.
* 128-bit: 130 arrays with a pair equal in lo and different in hi: the three
  layout calls and sks_intersect_all.

The battery also runs in this process at the defaults.  One more child forces
one bucket per workgroup on a layout of 2^14 buckets and 23 blocks, so that the
276 tiles need two launches (256 + 20 tiles): the second launch's offsets into
the packed output and the fused ANI's tile counters.  The pair kernels' second
launch (more than 2^24 pairs) is at the end, in-process.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":  # the child process: the paths tests/conftest.py sets up
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "spaced-kmer-sketching_amd"), os.path.join(_root, "oracle"),
               os.path.join(_root, "tests")):
        sys.path.insert(0, _p)

import sksffi
from test_gpu_parity import _device_sketch_arrays, _family_arrays, torch_cuda, ctx  # noqa: F401
from test_join_dedup import _wide_arrays

pytestmark = pytest.mark.gpu

K_ONES = 21
ROOT_SIZE = 700  # the fused ANI's table rows
U64_MAX = 2**64 - 1


# ---- data and the numpy reference --------------------------------------------------------------

def expected_counts(sk):
    """|S_i ∩ S_j| of every pair: M @ M.T of the sketch x distinct-value
    membership matrix (0 / 1 in float32: every partial sum is an integer below
    2^24, so the product is exact).  u64 arrays, or (lo, hi) rows."""
    n = len(sk)
    sizes = np.array([len(s) for s in sk])
    assert sizes.max() < 2**24
    if sk[0].ndim == 2:
        flat = np.ascontiguousarray(np.concatenate(sk)).view([("lo", np.uint64), ("hi", np.uint64)]).reshape(-1)
    else:
        flat = np.concatenate(sk)
    _, inv = np.unique(flat, return_inverse=True)
    m = np.zeros((n, int(inv.max()) + 1), dtype=np.float32)
    m[np.repeat(np.arange(n), sizes), inv.reshape(-1)] = 1.0
    want = (m @ m.T).astype(np.int64)
    assert np.array_equal(np.diag(want), sizes)  # every sketch's values are distinct
    return want


def u64_case():
    rng = np.random.default_rng(61)
    n = 150
    sk = _family_arrays(rng, n, 2500, 3, 0.2, 0.9, 300)
    sk[5] = np.zeros(0, np.uint64)
    sk[3] = np.union1d(sk[3], np.array([0], np.uint64))
    sk[40] = np.union1d(sk[40], np.array([0, U64_MAX], np.uint64))
    sk[100] = np.union1d(sk[100], np.array([U64_MAX], np.uint64))
    for i in (30, 31, 95, 140):  # rows the fused ANI reads from the context's table
        assert len(sk[i]) >= ROOT_SIZE
        sk[i] = np.sort(rng.choice(sk[i], ROOT_SIZE, replace=False))
    common = np.unique(rng.integers(0, U64_MAX, size=5000, dtype=np.uint64))
    for i in (20, 21, 90):  # a diagonal and an off-diagonal pair sharing >= 4096 values
        sk[i] = np.union1d(sk[i], common)
    want = expected_counts(sk)
    assert want[20, 21] >= 4096 and want[20, 90] >= 4096 and want[5].sum() == 0
    assert want[3, 40] >= 1 and want[40, 100] >= 1
    return sk, want


def wide_case():
    rng = np.random.default_rng(62)
    n = 130
    sk = _wide_arrays(rng, n, 1500, 3, 200)
    sk[7] = np.zeros((0, 2), np.uint64)
    # equal in lo but not in hi, and the reverse, across sketches and blocks
    sk[10] = np.concatenate([sk[10], np.array([[5, 2**63 + 1], [9, 2**63 + 7]], np.uint64)])
    sk[11] = np.concatenate([sk[11], np.array([[5, 2**63 + 2], [8, 2**63 + 7]], np.uint64)])
    sk[80] = np.concatenate([sk[80], np.array([[5, 2**63 + 1], [8, 2**63 + 7]], np.uint64)])
    for i in (10, 11, 80):
        sk[i] = sk[i][np.lexsort((sk[i][:, 0], sk[i][:, 1]))]
    want = expected_counts(sk)
    base = expected_counts([s[(s[:, 1] < 2**63)] for s in sk])  # without the added rows
    assert want[10, 11] == base[10, 11] and want[10, 80] == base[10, 80] + 1 and want[11, 80] == base[11, 80] + 1
    return sk, want


def _device_wide_arrays(torch, sk):
    sizes = np.array([len(x) for x in sk], dtype=np.uint32)
    starts = np.zeros(len(sk), dtype=np.uint64)
    starts[1:] = np.cumsum(sizes[:-1], dtype=np.uint64)
    flat = np.concatenate([x.reshape(-1) for x in sk] + [np.zeros(2, np.uint64)])
    return (torch.from_numpy(flat.view(np.int64)).to("cuda:0"), torch.from_numpy(starts.view(np.int64)).to("cuda:0"),
            torch.from_numpy(sizes.view(np.int32)).to("cuda:0"))


def sym_tiles(nb):
    return [(i, j) for i in range(nb) for j in range(i, nb)]


# ---- the calls ---------------------------------------------------------------------------------

def build_layout(torch, ctx, dev, sizes, first, count, log_b, ew):
    """The layout of sketches [first, first + count) (block 0 = sketch `first`)."""
    d, st, sz = dev
    tot = int(sizes[first:first + count].sum())
    nb = (count + 63) // 64
    lay = (torch.empty(max(tot, 1) * ew, dtype=torch.int64, device="cuda:0"),
           torch.empty(max(tot, 1), dtype=torch.int64, device="cuda:0"),
           torch.zeros(nb * sksffi.join_layout_boff_words(log_b), dtype=torch.int32, device="cuda:0"),
           torch.zeros(nb + 1, dtype=torch.int64, device="cuda:0"))
    mx = ctx.join_layout_build(d.data_ptr(), st.data_ptr() + 8 * first, sz.data_ptr() + 4 * first, count, log_b,
                               *(t.data_ptr() for t in lay), elem_words=ew)
    assert mx != 2**32 - 1, "layout invalid"
    torch.cuda.synchronize()
    assert int(lay[3][nb].item()) == tot
    return lay, mx


def check_sym_layout(torch, ctx, lay, n, log_b, ew, want):
    T = sksffi.intersect_sym_tiles(n)
    out = torch.full((n * n,), 7, dtype=torch.int32, device="cuda:0")
    ctx.intersect_sym_layout(n, log_b, *(t.data_ptr() for t in lay), 0, T, out.data_ptr(), elem_words=ew)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(n, n), want), ("sym_layout", log_b, ew)


def check_packed_tile_list(torch, ctx, dev, sizes, n, log_b, ew, want):
    """A layout of global blocks 1.. (blk0 = 1), a tile list, packed output."""
    own, _ = build_layout(torch, ctx, dev, sizes, 64, n - 64, log_b, ew)
    tiles = [(1, 1), (1, 2), (2, 2)]
    tl = torch.tensor(tiles, dtype=torch.int32, device="cuda:0")
    packed = torch.zeros((len(tiles), 64, 64), dtype=torch.int32, device="cuda:0")
    ctx.intersect_layout_tiles(n, log_b, *(t.data_ptr() for t in own), 1, tl.data_ptr(), 0, len(tiles), True,
                               packed.data_ptr(), elem_words=ew)
    torch.cuda.synchronize()
    pk = packed.cpu().numpy()
    for t, (I, J) in enumerate(tiles):
        blk = want[I * 64:I * 64 + 64, J * 64:J * 64 + 64]
        assert np.array_equal(pk[t, :blk.shape[0], :blk.shape[1]], blk), ("packed", I, J, ew)
        assert int(pk[t].sum()) == int(blk.sum()), ("packed: cells beyond n", I, J, ew)


def check_fused_ani(torch, ctx, lay, dev, n, log_b, ew, want, sizes):
    """sks_intersect_layout_ani over every tile of one layout: counts, and the ANI
    bit for bit that of sks_ani_rows (pow) on the same counts."""
    ctx.ani_table(ROOT_SIZE, K_ONES)
    ptrs = [t.data_ptr() for t in lay]
    out = torch.zeros((n, n), dtype=torch.int32, device="cuda:0")
    ani = torch.full((n, n), -1.0, dtype=torch.float64, device="cuda:0")
    ctx.intersect_layout_ani(n, log_b, ptrs, 0, ptrs, 0, 0, 0, sksffi.intersect_sym_tiles(n), False, out.data_ptr(),
                             dev[2].data_ptr(), K_ONES, ani.data_ptr(), elem_words=ew)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want), ("fused counts", ew)
    dense = torch.from_numpy(want.astype(np.int32)).to("cuda:0")
    rows = torch.full((n, n), -2.0, dtype=torch.float64, device="cuda:0")
    ctx.ani_rows(dense.data_ptr(), n, 0, n, K_ONES, rows.data_ptr())
    torch.cuda.synchronize()
    got, ref = ani.cpu().numpy(), rows.cpu().numpy()
    assert np.array_equal(got.view(np.int64), ref.view(np.int64)), ("fused ANI", ew)
    table = np.flatnonzero(sizes == ROOT_SIZE)
    if ew == 1:  # both kinds of row were there, with something to convert
        assert table.size >= 4 and (ref[table] > 0).sum() > table.size and (sizes != ROOT_SIZE).sum() > 100


def run_battery(torch, ctx, cases):
    (sk, want), (wsk, wwant) = cases
    # ---- u64 ----
    n = len(sk)
    sizes = np.array([len(s) for s in sk], dtype=np.int64)
    dev = _device_sketch_arrays(torch, sk)
    d, st, sz = (t.data_ptr() for t in dev)
    out = torch.full((n * n,), -3, dtype=torch.int32, device="cuda:0")
    ctx.intersect_all(d, st, sz, 1, n, 0, n, out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(n, n), want), "intersect_all"
    for r0, r1 in ((64, 150), (3, 97)):  # row blocks aligned / not aligned with the column blocks
        rows = torch.full(((r1 - r0) * n,), -5, dtype=torch.int32, device="cuda:0")
        ctx.intersect_all(d, st, sz, 1, n, r0, r1, rows.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(rows.cpu().numpy().reshape(r1 - r0, n), want[r0:r1]), ("rows", r0, r1)
    T = sksffi.intersect_sym_tiles(n)
    acc = np.zeros((n, n), dtype=np.int64)
    for a, b in ((0, 2), (2, T)):
        part = torch.full((n * n,), 5, dtype=torch.int32, device="cuda:0")
        ctx.intersect_sym(d, st, sz, 1, n, a, b, part.data_ptr())
        torch.cuda.synchronize()
        acc += part.cpu().numpy().reshape(n, n)
    assert np.array_equal(acc, want), "intersect_sym ranges"
    log_b = sksffi.join_layout_log_b(int(sizes.max()))
    cap = sksffi.join_layout_capacity()
    nat = None
    for lb in (log_b, 0, 3):
        lay, mx = build_layout(torch, ctx, dev, sizes, 0, n, lb, 1)
        if lb != log_b:
            assert mx > 2 * cap  # sub-chunks
        else:
            nat = lay
        check_sym_layout(torch, ctx, lay, n, lb, 1, want)
    check_packed_tile_list(torch, ctx, dev, sizes, n, log_b, 1, want)
    check_fused_ani(torch, ctx, nat, dev, n, log_b, 1, want, sizes)
    ctx.join_check_violations()  # reset
    ctx.set_join_check(True)
    try:
        out.fill_(-1)
        ctx.intersect_sym(d, st, sz, 1, n, 0, T, out.data_ptr())
        assert ctx.join_check_violations() == 0
    finally:
        ctx.set_join_check(False)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(n, n), want), "check build"
    # ---- 128-bit ----
    n = len(wsk)
    sizes = np.array([len(s) for s in wsk], dtype=np.int64)
    dev = _device_wide_arrays(torch, wsk)
    d, st, sz = (t.data_ptr() for t in dev)
    out = torch.full((n * n,), -3, dtype=torch.int32, device="cuda:0")
    ctx.intersect_all(d, st, sz, 2, n, 0, n, out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(n, n), wwant), "wide intersect_all"
    log_b = sksffi.join_layout_log_b(int(sizes.max()))
    lay, _ = build_layout(torch, ctx, dev, sizes, 0, n, log_b, 2)
    check_sym_layout(torch, ctx, lay, n, log_b, 2, wwant)
    check_packed_tile_list(torch, ctx, dev, sizes, n, log_b, 2, wwant)
    check_fused_ani(torch, ctx, lay, dev, n, log_b, 2, wwant, sizes)
    return log_b


@pytest.fixture(scope="module")
def cases():
    return u64_case(), wide_case()


def test_battery_at_defaults(torch_cuda, ctx, cases):
    """The battery in this process, with whatever geometry the default rules
    pick: the children below differ from it only in their one setting."""
    run_battery(torch_cuda, ctx, cases)


# ---- the children ------------------------------------------------------------------------------

U64_SYM_TILES = 6  # 150 sketches: 3 blocks
CHILDREN = {
    # name: (variable, value)
    "one_group": ("SKS_JOIN_WGS", "1"),
    "three_groups": ("SKS_JOIN_WGS", str(3 * U64_SYM_TILES)),
    "cap64": ("SKS_JOIN_CAP", "64"),
    "cap200": ("SKS_JOIN_CAP", "200"),
    "rg0": ("SKS_LAYOUT_RG", "0"),
    "rg1": ("SKS_LAYOUT_RG", "1"),
    "rg2": ("SKS_LAYOUT_RG", "2"),
    "rg3": ("SKS_LAYOUT_RG", "3"),
    "plain_tile_order": ("SKS_JOIN_TILE_ORDER", "1"),
    "two_slices": ("SKS_JOIN_WGS", str(1 << 40)),
}


def assert_premise(name, log_b):
    """The geometry the child is there for, as this process reports it."""
    var, value = CHILDREN[name]
    assert os.environ.get(var) == value
    if name == "one_group":
        for tiles in (1, 2, 3, 6):
            for lb in (0, 3, log_b, 14):
                assert sksffi.join_launch_plan(tiles, lb)[0] == 1
    elif name == "three_groups":
        assert sksffi.intersect_sym_tiles(150) == U64_SYM_TILES and log_b >= 3
        assert sksffi.join_launch_plan(U64_SYM_TILES, log_b)[0] == 3
        assert (1 << log_b) % 3 != 0  # so the last group is short
    elif name in ("cap64", "cap200"):
        assert sksffi.join_layout_capacity() == int(value)
        # the bucket count moves with it: a mean raw block-bucket of cap / 6
        assert sksffi.join_layout_log_b(600) == {"cap64": 12, "cap200": 11}[name]
    elif name.startswith("rg"):
        for nb in (1, 2, 3, 23, 1000):
            for lb in (0, 3, 6, log_b, 14):
                assert sksffi.join_layout_region_log(nb, lb) == int(value)
    else:
        assert name == "plain_tile_order"


def slices_case():
    """1430 sketches (23 blocks, the last of 22) of about 48 elements in 11
    families of 96 values, a few private values each."""
    rng = np.random.default_rng(63)
    n, fams = 1430, 11
    base = [np.unique(rng.integers(1, U64_MAX, size=96, dtype=np.uint64)) for _ in range(fams)]
    sk = []
    for i in range(n):
        b = base[i % fams]
        keep = b[rng.random(b.size) < 0.25 + 0.05 * (i % 10)]
        sk.append(np.unique(np.concatenate([keep, rng.integers(1, U64_MAX, size=i % 4, dtype=np.uint64)])))
    sk[700] = np.zeros(0, np.uint64)
    sk[0] = np.union1d(sk[0], np.array([0, U64_MAX], np.uint64))
    sk[1429] = np.union1d(sk[1429], np.array([0, U64_MAX], np.uint64))
    return sk, expected_counts(sk)


def run_two_slices(torch, ctx):
    log_b, n = 14, 1430
    nb = (n + 63) // 64
    tiles = sym_tiles(nb)
    T = len(tiles)
    assert nb == 23 and T == 276 == sksffi.intersect_sym_tiles(n)
    # the premise: one bucket per workgroup, so two launches of 256 and 20 tiles
    assert sksffi.join_launch_plan(T, log_b) == (16384, 256)
    sk, want = slices_case()
    sizes = np.array([len(s) for s in sk], dtype=np.int64)
    assert want[0, 1429] >= 2 and 40 <= np.median(sizes) <= 56
    dev = _device_sketch_arrays(torch, sk)
    lay, _ = build_layout(torch, ctx, dev, sizes, 0, n, log_b, 1)
    ptrs = [t.data_ptr() for t in lay]
    times = {}

    def timed(name, call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times[name] = time.perf_counter() - t0

    # dense
    out = torch.full((n * n,), 7, dtype=torch.int32, device="cuda:0")
    timed("dense", lambda: ctx.intersect_sym_layout(n, log_b, *ptrs, 0, T, out.data_ptr()))
    assert np.array_equal(out.cpu().numpy().reshape(n, n), want), "dense"

    # packed, every tile; the cells of the ragged block beyond n keep a mark
    def marked():
        p = np.zeros((T, 64, 64), dtype=np.int32)
        for t, (I, J) in enumerate(tiles):
            p[t, n - I * 64:, :] = -7
            p[t, :, n - J * 64:] = -7
        return p

    def check_packed(pk, what):
        for t, (I, J) in enumerate(tiles):
            blk = want[I * 64:I * 64 + 64, J * 64:J * 64 + 64]
            h, w = blk.shape
            assert np.array_equal(pk[t, :h, :w], blk), (what, t, I, J)
            assert (pk[t, h:, :] == -7).all() and (pk[t, :, w:] == -7).all(), (what, "beyond n", t, I, J)
    assert (marked()[T - 1] == -7).sum() == 4096 - 22 * 22
    packed = torch.from_numpy(marked()).to("cuda:0")
    timed("packed", lambda: ctx.intersect_layout_tiles(n, log_b, *ptrs, 0, 0, 0, T, True, packed.data_ptr()))
    check_packed(packed.cpu().numpy(), "packed")

    # fused ANI, packed counts
    root = int(np.bincount(sizes).argmax())
    ctx.ani_table(root, K_ONES)
    packed2 = torch.from_numpy(marked()).to("cuda:0")
    ani = torch.full((n, n), -1.0, dtype=torch.float64, device="cuda:0")
    timed("fused", lambda: ctx.intersect_layout_ani(n, log_b, ptrs, 0, ptrs, 0, 0, 0, T, True, packed2.data_ptr(),
                                                    dev[2].data_ptr(), K_ONES, ani.data_ptr()))
    check_packed(packed2.cpu().numpy(), "fused counts")
    dense = torch.from_numpy(want.astype(np.int32)).to("cuda:0")
    rows = torch.full((n, n), -2.0, dtype=torch.float64, device="cuda:0")
    ctx.ani_rows(dense.data_ptr(), n, 0, n, K_ONES, rows.data_ptr())
    torch.cuda.synchronize()
    got, ref = ani.cpu().numpy().view(np.int64), rows.cpu().numpy().view(np.int64)
    second = np.zeros((n, n), dtype=bool)  # the cells of the second launch's tiles, both orientations
    for I, J in tiles[256:]:
        second[I * 64:I * 64 + 64, J * 64:J * 64 + 64] = True
        second[J * 64:J * 64 + 64, I * 64:I * 64 + 64] = True
    assert second.sum() > 20 * 22 * 22 and (ref[second] != 0).sum() > 1000
    assert np.array_equal(got[second], ref[second]), "fused ANI, second launch"
    assert np.array_equal(got, ref), "fused ANI"
    print("two-slice calls: " + ", ".join(f"{k} {v * 1e3:.1f} ms" for k, v in times.items()))


def _run_child(name, timeout):
    var, value = CHILDREN[name]
    env = dict(os.environ)
    for v, _ in CHILDREN.values():
        env.pop(v, None)
    env[var] = value
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, capture_output=True, text=True,
                       timeout=timeout)
    print(f"child {name}: {time.perf_counter() - t0:.1f} s wall\n" + r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith(f"join geometry child {name} ok")


@pytest.mark.parametrize("name", [c for c in CHILDREN if c != "two_slices"])
def test_forced_geometry(name):
    """The battery in a fresh process with one knob set; the child asserts its
    premise through the accessors before it runs."""
    _run_child(name, 240)


def test_two_launch_slices():
    """276 tiles at 16384 workgroups per tile: launches of 256 and 20 tiles.  The
    dense, packed and fused-ANI calls equal numpy and sks_ani_rows; the cells of
    the ragged last block beyond n are untouched."""
    _run_child("two_slices", 240)


# ---- the pair kernels' second launch -------------------------------------------------------------

def test_pair_kernels_second_launch(torch_cuda, ctx):
    """sks_intersect_all under the global kernel and sks_intersect_pairs cut
    their pairs into launches of 2^24 (intersect.hip: 2^22 workgroups of four
    pairs).  4097 sketches, each 0..3 of 40 values (0 and 2^64 - 1 among them):
    4097^2 = 2^24 + 8193 pairs, so the last 8193 cells of the matrix belong to
    the second launch; then 2^24 + 1000 random pairs over 128-bit versions of
    the same sketches (hi word: a constant of the value, five distinct ones, so
    the 128-bit order differs from the lo words').  Expected: M @ M.T of the
    4097 x 40 membership matrix."""
    torch = torch_cuda
    rng = np.random.default_rng(64)
    n, u = 4097, 40
    lo = np.unique(np.concatenate([np.array([0, U64_MAX], np.uint64),
                                   rng.integers(1, U64_MAX, size=u - 2, dtype=np.uint64)]))
    assert lo.size == u
    hi = (np.arange(u, dtype=np.uint64) * np.uint64(7)) % np.uint64(5)
    member = np.zeros((n, u), dtype=np.int32)
    for i in range(n):
        member[i, rng.choice(u, size=i % 4, replace=False)] = 1
    member[n - 1, [0, u - 1]] = 1  # the last sketch holds both extremes: the last cell is 2 or 3
    want = member @ member.T
    assert n * n == (1 << 24) + 8193 and want.reshape(-1)[-8193:].any()
    d, st, sz = _device_sketch_arrays(torch, [lo[np.flatnonzero(m)] for m in member])
    want_d = torch.from_numpy(want).to("cuda:0")
    out = torch.full((n, n), -9, dtype=torch.int32, device="cuda:0")
    ctx.set_intersect_kernel(sksffi.INTERSECT_GLOBAL)
    try:
        ctx.intersect_all(d.data_ptr(), st.data_ptr(), sz.data_ptr(), 1, n, 0, n, out.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.set_intersect_kernel(sksffi.INTERSECT_AUTO)
    assert not bool((out.reshape(-1)[-8193:] == -9).any()), "the second launch wrote nothing"
    assert torch.equal(out, want_d)
    # 128-bit elements in (hi, lo) order
    order = np.lexsort((lo, hi))
    wide = np.stack([lo[order], hi[order]], axis=1)
    assert (np.diff(wide[:, 0].astype(np.float64)) < 0).any()  # not the lo words' order
    wd, wst, wsz = _device_wide_arrays(torch, [wide[np.flatnonzero(m[order])] for m in member])
    n_pairs = (1 << 24) + 1000
    a = rng.integers(0, n, size=n_pairs, dtype=np.int32)
    b = rng.integers(0, n, size=n_pairs, dtype=np.int32)
    a[-1], b[-1] = n - 1, n - 1
    a_d, b_d = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
    got = torch.full((n_pairs,), -9, dtype=torch.int32, device="cuda:0")
    ctx.intersect_pairs(wd.data_ptr(), wst.data_ptr(), wsz.data_ptr(), 2, a_d.data_ptr(), b_d.data_ptr(), n_pairs,
                        got.data_ptr())
    torch.cuda.synchronize()
    want_p = want_d[a_d.long(), b_d.long()]
    assert int(want_p[-1]) == int(member[n - 1].sum()) >= 2 and bool(want_p[-1000:].any())
    assert not bool((got[-1000:] == -9).any()), "the second launch wrote nothing"
    assert torch.equal(got, want_p)


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available()
    which = sys.argv[1]
    cx = sksffi.Context(0)
    if which == "two_slices":
        run_two_slices(torch, cx)
    else:
        both = (u64_case(), wide_case())
        natural = sksffi.join_layout_log_b(max(len(s) for s in both[0][0]))
        assert_premise(which, natural)
        run_battery(torch, cx, both)
    cx.close()
    print(f"join geometry child {which} ok")
