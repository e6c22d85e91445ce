"""Every rank of the multi-GPU all-vs-all (sks_dist.all_vs_all_join, world > 1)
replayed on one GPU against numpy, count for count and ANI bit for bit.

On N GPUs every rank runs the join kernels in a geometry no one-rank call has:
its own layout starts at a global block blk0 = g0 / 64 > 0 and |S_g| is read
through a sizes pointer moved back by g0 words; one layout is built over the
exchange buffer (row g = genome g at a fixed stride, whole 64-sketch blocks of
it empty, the region log picked from the blocks that hold sketches); the plan's
cross tiles pair a lower rank's block with a higher rank's, for wrap-around
peers from opposite ends of that layout; and the native call clears its own
counts, finisher counters and status words.  Here each rank's step runs in this
process with no process group, as tools/rank_sim.py runs it: the exchange is
replaced by a buffer in which the peers' padded rows (their own ops.pad output)
already lie and into which the call writes only the rank's own slot; size_bound,
bounds_mask and dst=None keep every collective out of the way.

* u64: 330 caller arrays (6 blocks, the last of 10 sketches) in four families,
  sizes 0 .. 700, five sketches of exactly 700 elements (the fused ANI's table
  rows, the rest pow rows), an empty sketch in a full block and one in the last
  block, every sketch of global block 2 empty, 0 and 2^64 - 1 present.  Worlds
  2, 3, 4 (rank 3 without genomes, rank 2 needs rank 0) and 8 (ranks 6 and 7
  without genomes, rank 5 owns the 10-sketch block and needs rank 0).
* 128-bit: 200 arrays whose high words differ within a sketch, pairs equal in
  lo and different in hi across ranks.  Worlds 2 and 4 (rank 3 holds 8).

Per (world, rank): every packed tile equals numpy's counts (cells past n are
0), the layouts' status words are clean, the ANI of the rank's tiles (both
orientations) is sks_ani_rows' bit for bit and within 1e-9 of the host's
sks_ani_from_counts, and no other cell of the matrix changed.  Per world: the
ranks' tiles cover the upper triangle exactly once, place_tiles of them is the
numpy matrix and the shared ANI matrix is that of one sks_all_pairs_ani call.
Each parametrisation first establishes, from what the run itself reports, the
geometry it is there for (assert_premise); one that cannot fails.

Routes: native (sks_layout_tiles_ani), non-native (sks_join_layout_build with a
blocks hint + sks_intersect_layout_pair_tiles / sks_intersect_layout_ani with a
tile list), counts only, ANI into pinned host memory, rank 0's sampled bounds
instead of the mask's, the step repeated on the same context over a dirtied
count buffer, and, in child processes (this file as a script, one at a time),
forced region logs and work splits.  At the end, the entry points this path and
its callers use that no other test calls: sks_sketches_export,
sks_sketch_set_export_csr, the k-mer list's device arrays and
sks_join_layout_stat_copy.
"""
import ctypes
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

import sks_dist
import sksffi
from test_gpu_parity import _device_sketch_arrays, torch_cuda, ctx  # noqa: F401
from test_join_geometry import _device_wide_arrays, build_layout, expected_counts

pytestmark = pytest.mark.gpu

TILE = sks_dist.TILE
U64_MAX = 2**64 - 1
JUNK = 0x5A5A5A5A5A5A5A5A  # rows of the exchange buffer nothing may read
DIRTY = 0x2B2B2B2B         # count tiles before a native call


# ---- data and the numpy reference --------------------------------------------------------------

class Case:
    """name; ew; sk: the sorted unique arrays; want: numpy's counts; bound: the
    size bound every rank passes (the largest sketch: table rows); k, mask: the
    ANI's k and the k-mer mask the group bounds come from."""

    def __init__(self, name, ew, sk, bound, k, mask):
        self.name, self.ew, self.sk, self.bound, self.k, self.mask = name, ew, sk, bound, k, mask
        self.n = len(sk)
        self.sizes = np.array([len(s) for s in sk], dtype=np.int64)
        self.want = expected_counts(sk)
        nb = (self.n + TILE - 1) // TILE
        self.want_pad = np.zeros((nb * TILE, nb * TILE), dtype=np.int64)  # cells past n: 0
        self.want_pad[:self.n, :self.n] = self.want
        assert self.sizes.max() == bound

    def tile(self, I, J):
        return self.want_pad[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE]


def u64_case():
    rng = np.random.default_rng(71)
    n, fams, bound, k = 330, 4, 700, 21
    mask = sksffi.mask_generate(31, k, 0)
    assert bin(mask).count("1") == 2 * k and mask >> 64 == 0
    m = np.uint64(mask)

    def draw(size):  # values a sketch built with the mask could hold
        return rng.integers(0, U64_MAX, size=size, dtype=np.uint64) & m

    base = [np.unique(draw(640)) for _ in range(fams)]
    sk = []
    for i in range(n):  # every block holds every family: blocks of different ranks share elements
        b = base[i % fams]
        keep = b[rng.random(b.size) < 0.1 + 0.8 * ((i * 7) % 10) / 10]
        sk.append(np.union1d(keep, draw(i % 50)))
    for i, size in ((1, 1), (65, 2), (321, 3)):
        sk[i] = sk[i][:size].copy()
    table = (7, 66, 200, 260, 322)  # rows the fused ANI reads from the context's table: blocks 0, 1, 3, 4, 5
    for i in table:
        pool = np.union1d(base[i % fams], draw(200))
        sk[i] = np.sort(rng.choice(pool, bound, replace=False))
    sk[3] = np.union1d(sk[3], np.array([0], np.uint64))
    sk[40] = np.union1d(sk[40], np.array([0, U64_MAX], np.uint64))
    sk[300] = np.union1d(sk[300], np.array([U64_MAX], np.uint64))
    sk[329] = np.union1d(sk[329], np.array([0, U64_MAX], np.uint64))
    sk[70] = np.zeros(0, np.uint64)   # an empty sketch inside a full block
    sk[325] = np.zeros(0, np.uint64)  # and one in the last block
    for i in range(128, 192):         # every sketch of global block 2
        sk[i] = np.zeros(0, np.uint64)
    case = Case("u64", 1, sk, bound, k, mask)
    sizes, want = case.sizes, case.want
    assert np.flatnonzero(sizes == bound).tolist() == list(table) and sizes.min() == 0
    assert (sizes[sizes != bound] < bound - 8).all() and (sizes[sizes != bound] > 0).sum() > 250
    assert want[128:192].sum() == 0 and want[70].sum() == 0 and want[325].sum() == 0
    assert want[40, 329] >= 2 and want[3, 329] >= 1 and want[300, 329] >= 1
    assert (want[:64, 320:] > 0).sum() > 60 and (want[64:128, 256:320] > 0).sum() > 500  # shared across ranks
    return case


def wide_case():
    rng = np.random.default_rng(72)
    n, fams, bound, k = 200, 3, 560, 30
    mask = sksffi.mask_generate(45, k, 0)
    assert bin(mask).count("1") == 2 * k and mask >> 64 != 0
    m = np.array([mask & U64_MAX, mask >> 64], dtype=np.uint64)

    def draw(size):  # (lo, hi) rows within the mask
        return rng.integers(0, U64_MAX, size=(size, 2), dtype=np.uint64) & m

    def ordered(a):  # distinct rows in (hi, lo) order
        a = np.unique(a, axis=0)
        return a[np.lexsort((a[:, 0], a[:, 1]))]

    base = [draw(500) for _ in range(fams)]
    sk = []
    for i in range(n):
        b = base[i % fams]
        keep = b[rng.random(len(b)) < 0.2 + 0.7 * ((i * 7) % 10) / 10]
        sk.append(ordered(np.concatenate([keep, draw(i % 40)])))
    for i in (20, 197):  # table rows, one of them among the last rank's eight
        pool = ordered(np.concatenate([base[i % fams], draw(100)]))
        sk[i] = ordered(pool[rng.choice(len(pool), bound, replace=False)])
    sk[9] = np.zeros((0, 2), np.uint64)
    # equal in lo but not in hi, and the reverse, across blocks (at world 4: across ranks)
    top = 2**63
    sk[10] = ordered(np.concatenate([sk[10], np.array([[5, top + 1], [9, top + 7]], np.uint64)]))
    sk[11] = ordered(np.concatenate([sk[11], np.array([[5, top + 2], [8, top + 7]], np.uint64)]))
    sk[130] = ordered(np.concatenate([sk[130], np.array([[5, top + 1], [8, top + 7]], np.uint64)]))
    sk[195] = ordered(np.concatenate([sk[195], np.array([[5, top + 2], [9, top + 7]], np.uint64)]))
    case = Case("wide", 2, sk, bound, k, mask)
    base_counts = expected_counts([s[s[:, 1] < top] for s in sk])  # without the added rows
    extra = case.want - base_counts
    assert extra[10, 11] == 0 and extra[10, 130] == 1 and extra[11, 130] == 1
    assert extra[10, 195] == 1 and extra[11, 195] == 1 and extra[130, 195] == 0
    assert all(len(np.unique(s[:, 1])) > 50 for s in sk if len(s) > 60)  # high words differ within a sketch
    assert np.flatnonzero(case.sizes == bound).tolist() == [20, 197] and case.sizes.min() == 0
    return case


CASES = {"u64": u64_case, "wide": wide_case}
WORLDS = [("u64", 2), ("u64", 3), ("u64", 4), ("u64", 8), ("wide", 2), ("wide", 4)]


def upload(torch, sk, ew):
    """The arrays as a rank holds them: its own CSR device arrays."""
    if not sk:
        return sks_dist.sketches_of(None, ew)
    d, st, sz = (_device_sketch_arrays if ew == 1 else _device_wide_arrays)(torch, sk)
    return sks_dist.Sketches(d, sz, ew, starts=st)


def packed_want(case, tiles):
    """numpy's counts of the tiles, packed [tile][64][64] (cells past n: 0)."""
    if not len(tiles):
        return np.zeros((0, TILE, TILE), np.int64)
    return np.stack([case.tile(I, J) for I, J in tiles])


class Reference:
    """Computed once per case and process and left unchanged: the ANI of numpy's
    counts by sks_ani_rows (bit reference) and by the host (within 1e-9), and
    the one-process call's ANI matrix (sks_all_pairs_ani over all n sketches)."""

    def __init__(self, torch, ctx, case):
        n = case.n
        self.all = upload(torch, case.sk, case.ew)
        dense = torch.from_numpy(case.want.astype(np.int32)).to("cuda:0")
        rows = torch.full((n, n), -2.0, dtype=torch.float64, device="cuda:0")
        ctx.ani_rows(dense.data_ptr(), n, 0, n, case.k, rows.data_ptr())
        torch.cuda.synchronize()
        self.ani = rows.cpu().numpy()
        _, host = sksffi.ani_from_counts(case.want.reshape(-1), np.repeat(case.sizes, n), case.k)
        self.host_ani = host.reshape(n, n)
        assert np.abs(self.ani - self.host_ani).max() <= 1e-9
        one = torch.full((n, n), -1.0, dtype=torch.float64, device="cuda:0")
        res = sks_dist.all_vs_all_join(n, 1, 0, self.all, DirtyPartsOps(ctx, case.ew), sksffi.join_layout_log_b,
                                       device="cuda", dst=None, ani_ones=case.k, ani_out=one,
                                       max_size=int(case.sizes.max()), size_bound=case.bound)
        torch.cuda.synchronize()
        res.check_layouts()
        assert np.array_equal(res.counts.cpu().numpy(), packed_want(case, res.tiles)), "one process: counts"
        self.one_ani = one.cpu().numpy()
        assert np.array_equal(self.one_ani.view(np.int64), self.ani.view(np.int64)), "one process: ANI"
        table = case.sizes == case.bound  # both kinds of row, with something to convert
        assert (self.ani[table] > 0).sum() > table.sum() and (self.ani[~table] > 0).sum() > 1000


# ---- the kernels' callers ----------------------------------------------------------------------

class DirtyPartsOps(sks_dist.GpuJoinOps):
    """GpuJoinOps whose count tiles hold a non-zero pattern wherever the kernels
    are to clear them (the native calls): a call that does not clear its output
    shows as wrong counts, in cells past n as well."""

    fills = 0

    def parts(self, T, device, zeroed=True):
        p = super().parts(T, device, zeroed)
        if not zeroed:
            p.fill_(DIRTY)
            self.fills += 1
        return p


class NoNativeOps:
    """Forwards everything except layout_tiles_ani, so all_vs_all_join takes the
    build + count route (hasattr is false)."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        if name == "layout_tiles_ani":
            raise AttributeError(name)
        return getattr(self._inner, name)


def make_ops(ctx, ew, native=True):
    ops = DirtyPartsOps(ctx, ew)
    if native:
        assert hasattr(ops, "layout_tiles_ani")
        return ops
    ops = NoNativeOps(ops)
    assert not hasattr(ops, "layout_tiles_ani") and hasattr(ops, "count_ani") and hasattr(ops, "build")
    return ops


# ---- the replay --------------------------------------------------------------------------------

def read_ani(torch, ani_out, n):
    torch.cuda.synchronize()
    if hasattr(ani_out, "data_ptr"):
        return ani_out.cpu().numpy().reshape(n, n).copy()
    return np.array(ani_out.array).reshape(n, n)


def write_ani(torch, ani_out, value):
    if hasattr(ani_out, "data_ptr"):
        ani_out.copy_(torch.from_numpy(value).reshape(ani_out.shape))
    else:
        ani_out.array[:] = value.reshape(-1)


def replay_world(torch, case, ref, world, ops, patch, fused=True, ani_out=None, sampled=False, repeat=1):
    """Every rank's step of `world`, one after another in this process; returns
    the facts of each rank's geometry for assert_premise."""
    n, ew, S, k = case.n, case.ew, case.bound, case.k
    per = sks_dist.block_shard(n, world, 0)[0] * TILE
    row = per * S * ew
    # what the exchange delivers: every rank's padded rows, each its own ops.pad
    # output; rows past a rank's genomes belong to nobody and keep JUNK with size 0
    xbuf = torch.full((world * row,), JUNK, dtype=torch.int64, device="cuda:0")
    full_sz = torch.zeros(world * per, dtype=torch.int32, device="cuda:0")
    shards = [sks_dist.block_shard(n, world, q)[1:] for q in range(world)]
    mine_of = [upload(torch, case.sk[a:b], ew) for a, b in shards]
    for q, (a, b) in enumerate(shards):
        if b > a:
            ops.pad(mine_of[q], S, xbuf[q * row:(q + 1) * row], full_sz[q * per:(q + 1) * per])
    torch.cuda.synchronize()
    want_buf = np.full((world * per, S * ew), JUNK, dtype=np.uint64)
    want_sz = np.zeros(world * per, dtype=np.int64)
    for q, (a, b) in enumerate(shards):
        for g in range(a, b):
            r = q * per + g - a
            want_buf[r] = U64_MAX
            want_buf[r, :len(case.sk[g]) * ew] = case.sk[g].reshape(-1)
            want_sz[r] = len(case.sk[g])
    assert np.array_equal(xbuf.cpu().numpy().view(np.uint64).reshape(world * per, S * ew), want_buf), "ops.pad: rows"
    assert np.array_equal(full_sz.cpu().numpy(), want_sz), "ops.pad: sizes"
    assert all(a == q * per for q, (a, b) in enumerate(shards) if b > a)  # row g = genome g
    rank_sz = []
    for r in range(world):
        keep = torch.zeros(world * per, dtype=torch.bool, device="cuda:0")
        for q in [r] + sks_dist.peer_needs(n, world, r):
            keep[q * per:(q + 1) * per] = True
        rank_sz.append(torch.where(keep, full_sz, torch.zeros_like(full_sz)))
    state = {"rank": None, "exchanges": 0, "broadcasts": 0, "gb": None}

    def fake_exchange(own, n_genomes, world_, rank, stride, ops_, mode):
        # the rank's own slot: its export, as the real exchange writes it before
        # sending; the peers' rows are already in place
        assert (n_genomes, world_, rank, stride, own.ew) == (n, world, state["rank"], S, ew)
        state["exchanges"] += 1
        sz = rank_sz[rank]
        if own.n:
            ops_.pad(own, stride, xbuf[rank * row:(rank + 1) * row], sz[rank * per:(rank + 1) * per])

        def wait():
            return sks_dist._strided(xbuf, sz, ew, stride)
        return wait

    def fake_broadcast(t, src, world_):
        assert src == 0 and world_ == world
        state["broadcasts"] += 1
        if state["rank"] == 0:
            state["gb"] = t.clone()
        else:
            t.copy_(state["gb"])
        return t

    patch.setattr(sks_dist, "_exchange_start", fake_exchange)
    patch.setattr(sks_dist, "_broadcast", fake_broadcast)
    if fused and ani_out is None:
        ani_out = torch.full((n, n), -1.0, dtype=torch.float64, device="cuda:0")
    if fused:
        write_ani(torch, ani_out, np.full((n, n), -1.0))
    facts, all_tiles, all_counts = [], [], []
    for rank in range(world):
        g0, g1 = shards[rank]
        mine = mine_of[rank]
        mx = int(case.sizes[g0:g1].max()) if g1 > g0 else 0
        plan = sks_dist._plan_in_count_order(n, world, rank)
        local, _ = sks_dist.tile_plan_by_peer(n, world, rank)
        tq, held = sks_dist._cross_plan(n, world, rank)
        need = sks_dist.peer_needs(n, world, rank)
        cells = np.zeros((n, n), dtype=bool)  # the rank's tiles, both orientations
        for I, J in plan:
            cells[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE] = True
            cells[J * TILE:(J + 1) * TILE, I * TILE:(I + 1) * TILE] = True
        before = read_ani(torch, ani_out, n) if fused else None
        first = None
        for it in range(repeat):
            state["rank"] = rank
            # the rank's own slot as before its export: the call has to write it
            xbuf[rank * row:(rank + 1) * row] = JUNK
            rank_sz[rank][rank * per:(rank + 1) * per] = 0
            if it:
                write_ani(torch, ani_out, before)
            res = sks_dist.all_vs_all_join(n, world, rank, mine, ops, sksffi.join_layout_log_b, device="cuda",
                                           dst=None, ani_ones=k if fused else None,
                                           ani_out=ani_out if fused else None, max_size=mx, size_bound=S,
                                           bounds_mask=None if sampled else case.mask)
            torch.cuda.synchronize()
            res.check_layouts()
            where = (case.name, world, rank, it)
            assert np.array_equal(np.asarray(res.tiles).reshape(-1, 2), plan), where
            got_counts = res.counts.cpu().numpy()
            assert got_counts.shape == (len(plan), TILE, TILE), where
            bad = np.flatnonzero((got_counts != packed_want(case, plan)).any(axis=(1, 2)))
            assert bad.size == 0, (where, "tiles with wrong counts", [tuple(plan[t]) for t in bad])
            if fused:
                assert res.ani is ani_out
                got = read_ani(torch, ani_out, n)
                assert (before[cells] == -1.0).all(), where  # nobody wrote them earlier
                assert np.array_equal(got.view(np.int64)[cells], ref.ani.view(np.int64)[cells]), (where, "ANI")
                if cells.any():
                    assert np.abs(got[cells] - ref.host_ani[cells]).max() <= 1e-9, (where, "ANI against the host")
                assert np.array_equal(got.view(np.int64)[~cells], before.view(np.int64)[~cells]), \
                    (where, "a cell outside the rank's tiles changed")
            else:
                assert res.ani is None
                got = None
            if first is None:
                first = (got_counts, got)
            else:
                assert np.array_equal(first[0], got_counts) and (got is None or np.array_equal(first[1], got)), \
                    (where, "the repeated step differs")
        all_tiles.append(plan)
        all_counts.append(res.counts)
        sz_blocks = rank_sz[rank].cpu().numpy().reshape(-1, TILE).any(axis=1)
        facts.append({"rank": rank, "blk0": g0 // TILE, "own": g1 - g0, "local": len(local), "cross": len(tq),
                      "need": need, "held": held, "layout_blocks": world * per // TILE,
                      "buffer": "".join("X" if b else "." for b in sz_blocks)})
        print(f"replay {case.name} world {world} rank {rank}: blk0 {g0 // TILE}, {g1 - g0} own sketches, "
              f"{len(local)} local + {len(tq)} cross tiles, needs {need}, holds {held} of "
              f"{world * per // TILE} layout blocks, buffer {facts[-1]['buffer']}")
    assert state["exchanges"] == world * repeat
    assert state["broadcasts"] == (world * repeat if sampled else 0)
    # the rank's exports left the buffer as the peers' exports had
    assert np.array_equal(xbuf.cpu().numpy().view(np.uint64).reshape(world * per, S * ew), want_buf)
    # after all ranks: the upper triangle exactly once, the assembled counts, the shared ANI
    tiles = np.concatenate(all_tiles).reshape(-1, 2)
    nb = (n + TILE - 1) // TILE
    assert sorted(map(tuple, tiles.tolist())) == [(i, j) for i in range(nb) for j in range(i, nb)]
    mat = torch.zeros((n, n), dtype=torch.int32, device="cuda:0")
    sks_dist.place_tiles(mat, tiles, torch.cat(all_counts), n)
    assert np.array_equal(mat.cpu().numpy(), case.want), (case.name, world, "place_tiles")
    if fused:
        got = read_ani(torch, ani_out, n)
        assert np.array_equal(got.view(np.int64), ref.one_ani.view(np.int64)), (case.name, world, "shared ANI")
    return facts


def assert_premise(name, world, facts):
    """The geometry the parametrisation is there for, from what the run reported."""
    by = {f["rank"]: f for f in facts}
    # a rank whose own layout starts at a global block > 0 and that joins cross tiles
    assert any(f["blk0"] > 0 and f["local"] and f["cross"] for f in facts), (name, world, "blk0 > 0")
    between = [f for f in facts if f["cross"] and ".X" in f["buffer"].strip(".")]
    fewer = [f for f in facts if f["cross"] and f["held"] < f["layout_blocks"]]
    if name == "u64":
        # global block 2 holds only empty sketches: an all-empty block between two held ones everywhere
        assert between, (name, world, "no empty block between held blocks")
        if world == 2:
            assert all(f["held"] == 6 == f["layout_blocks"] and f["own"] for f in facts)
        elif world == 3:
            assert all(f["local"] == 3 and f["cross"] == 4 for f in facts) and fewer
        elif world == 4:
            assert by[3]["own"] == 0 and by[3]["local"] + by[3]["cross"] == 0
            assert 0 in by[2]["need"] and fewer
        else:
            assert world == 8 and by[6]["own"] == 0 and by[7]["own"] == 0
            assert by[5]["own"] == 10 and by[5]["need"] == [0] and by[5]["held"] == 2 and by[5] in fewer
            assert by[5]["buffer"].rstrip(".") == "X....X"  # the two held runs at opposite ends
    else:
        assert name == "wide"
        if world == 2:
            assert all(f["held"] == 4 == f["layout_blocks"] for f in facts)
        else:
            assert world == 4 and all(f["own"] for f in facts) and by[3]["own"] == 8
            assert by[3]["need"] == [0] and by[3] in fewer and by[3] in between


# ---- in this process ---------------------------------------------------------------------------

_CACHE = {}


def case_of(name):
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]


@pytest.fixture(scope="module")
def refs(torch_cuda, ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Reference(torch_cuda, ctx, case_of(name))
        return case_of(name), made[name]
    return get


@pytest.mark.parametrize("name,world", WORLDS)
@pytest.mark.parametrize("route", ["native", "build_count"])
def test_replay_fused(torch_cuda, ctx, refs, monkeypatch, name, world, route):
    """Counts and the fused ANI (device matrix prefilled with -1) of every rank,
    by sks_layout_tiles_ani and by the build + count route (there the exchange
    buffer's layout is built under sks_ctx_set_layout_blocks_hint(held) and
    joined with a tile list)."""
    case, ref = refs(name)
    ops = make_ops(ctx, case.ew, native=route == "native")
    hints, set_hint = [], ctx.set_layout_blocks_hint
    monkeypatch.setattr(ctx, "set_layout_blocks_hint", lambda b: (hints.append(int(b)), set_hint(b))[1])
    facts = replay_world(torch_cuda, case, ref, world, ops, monkeypatch)
    assert_premise(name, world, facts)
    if route == "native":
        assert ops.fills >= sum(1 for f in facts if f["local"] + f["cross"]) and not hints
    else:
        assert [h for h in hints if h] == [f["held"] for f in facts if f["cross"]] and hints[-1] == 0


@pytest.mark.parametrize("name,world", WORLDS)
@pytest.mark.parametrize("route", ["native", "build_count"])
def test_replay_counts_only(torch_cuda, ctx, refs, monkeypatch, name, world, route):
    """ani_ones=None: the same tiles without the finisher."""
    case, ref = refs(name)
    ops = make_ops(ctx, case.ew, native=route == "native")
    facts = replay_world(torch_cuda, case, ref, world, ops, monkeypatch, fused=False)
    assert_premise(name, world, facts)


def test_replay_ani_into_pinned_host_memory(torch_cuda, ctx, refs, monkeypatch):
    """ani_out a sksffi.HostBuffer: the join writes the ANI through the device
    view of pinned host memory (u64, world 8)."""
    case, ref = refs("u64")
    hb = sksffi.HostBuffer(case.n * case.n * 8)
    try:
        facts = replay_world(torch_cuda, case, ref, 8, make_ops(ctx, 1), monkeypatch, ani_out=hb)
        assert_premise("u64", 8, facts)
    finally:
        hb.free()


@pytest.mark.parametrize("name,world", [("u64", 8), ("wide", 4)])
def test_replay_step_twice_on_one_context(torch_cuda, ctx, refs, monkeypatch, name, world):
    """Every rank's step twice in a row on the same ops and context, the count
    tiles filled with a non-zero pattern before each: the call clears its counts,
    its tiles' finisher counters and its status words, and both runs agree."""
    case, ref = refs(name)
    ops = make_ops(ctx, case.ew)
    facts = replay_world(torch_cuda, case, ref, world, ops, monkeypatch, repeat=2)
    assert_premise(name, world, facts)
    assert ops.fills >= 2 * sum(1 for f in facts if f["local"] + f["cross"])


@pytest.mark.parametrize("route", ["native", "build_count"])
def test_replay_sampled_bounds(torch_cuda, ctx, refs, monkeypatch, route):
    """bounds_mask=None: rank 0 samples the group bounds of its own sketches and
    the (patched) broadcast hands them to the other ranks (u64, world 4)."""
    case, ref = refs("u64")
    facts = replay_world(torch_cuda, case, ref, 4, make_ops(ctx, 1, native=route == "native"), monkeypatch,
                         sampled=True)
    assert_premise("u64", 4, facts)


# ---- forced join geometry: one child process per setting ----------------------------------------

CHILD_WORLDS = [("u64", 4), ("wide", 2)]
CHILDREN = {
    # name: (variable, value)
    "rg0": ("SKS_LAYOUT_RG", "0"),
    "rg1": ("SKS_LAYOUT_RG", "1"),
    "rg2": ("SKS_LAYOUT_RG", "2"),
    "rg3": ("SKS_LAYOUT_RG", "3"),
    "one_group": ("SKS_JOIN_WGS", "1"),
    "three_groups": ("SKS_JOIN_WGS", "9"),  # 3 groups a tile in the calls of 3 and of 4 tiles
}


def assert_child_premise(which, case, facts):
    """The forced geometry, as this process reports it, for the calls of the replay."""
    var, value = CHILDREN[which]
    assert os.environ.get(var) == value
    log_b = sksffi.join_layout_log_b(case.bound)
    calls = sorted({f[key] for f in facts for key in ("local", "cross") if f[key]})
    blocks = sorted({(f["own"] + TILE - 1) // TILE for f in facts if f["own"]} |
                    {x for f in facts if f["cross"] for x in (f["held"], f["layout_blocks"])})
    assert calls and blocks and log_b >= 6
    if which.startswith("rg"):
        assert all(sksffi.join_layout_region_log(nb, log_b) == int(value) for nb in blocks), (which, blocks)
    elif which == "one_group":
        assert all(sksffi.join_launch_plan(t, log_b)[0] == 1 for t in calls), (which, calls)
    else:
        assert which == "three_groups"
        groups = {t: sksffi.join_launch_plan(t, log_b)[0] for t in calls}
        assert 3 in groups.values() and min(groups.values()) > 1, groups
        assert (1 << log_b) % 3 != 0  # so the last group is short


def _run_child(which, timeout):
    var, value = CHILDREN[which]
    env = dict(os.environ)
    for v in ("SKS_JOIN_WGS", "SKS_JOIN_CAP", "SKS_LAYOUT_RG", "SKS_JOIN_TILE_ORDER"):
        env.pop(v, None)
    env[var] = value
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], env=env, capture_output=True, text=True,
                       timeout=timeout)
    print(f"child {which}: {time.perf_counter() - t0:.1f} s wall\n" + r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith(f"rank replay child {which} ok")


@pytest.mark.parametrize("which", list(CHILDREN))
def test_replay_forced_geometry(which):
    """World 4 of the u64 case and world 2 of the 128-bit case, both routes,
    fused, in a fresh process with one knob set; the child asserts through
    sks_join_layout_region_log / sks_join_launch_plan that its calls had the
    geometry before it trusts their results."""
    _run_child(which, 240)


# ---- entry points of this path and its callers that nothing else calls --------------------------

def test_join_layout_stat_copy_nonzero_status(torch_cuda, ctx):
    """sks_join_layout_stat_copy after a build that leaves a non-zero status:
    the copied words are (largest block bucket, 0), the first as the build's
    read-back reports it; a later build's words replace them."""
    torch = torch_cuda
    case = case_of("u64")
    log_b = sksffi.join_layout_log_b(case.bound)
    dev = _device_sketch_arrays(torch, case.sk)
    got = []
    for first, count in ((0, 128), (128, 64), (192, case.n - 192)):  # block 2: nothing to place
        _, mx = build_layout(torch, ctx, dev, case.sizes, first, count, log_b, 1)
        slot = torch.full((4,), -9, dtype=torch.int32, device="cuda:0")
        ctx.join_layout_stat_copy(slot.data_ptr() + 4)
        torch.cuda.synchronize()
        assert slot.tolist() == [-9, mx, 0, -9]
        got.append(mx)
    assert got[0] > 0 and got[1] == 0 and got[2] > 0


def _export_case(torch, ew, stride):
    rng = np.random.default_rng(73 + ew)
    sizes = [stride, 0, 1, stride - 1, 5] + [int(x) for x in rng.integers(0, stride + 1, size=65)] + [0, stride]
    if ew == 1:
        sk = [np.unique(rng.integers(0, U64_MAX, size=4 * stride, dtype=np.uint64))[:s] for s in sizes]
    else:
        sk = []
        for s in sizes:
            a = np.unique(rng.integers(0, U64_MAX, size=(s, 2), dtype=np.uint64), axis=0)
            sk.append(a[np.lexsort((a[:, 0], a[:, 1]))])
    assert [len(s) for s in sk] == sizes
    return sk


@pytest.mark.parametrize("ew", [1, 2])
def test_sketches_export_device_arrays(torch_cuda, ctx, ew):
    """sks_sketches_export of caller-owned device arrays (72 sketches, stride 37):
    each row holds its sketch, then ~0 words; a sketch of exactly `stride`
    elements is exported whole, a size-0 sketch as size 0; d_dst_sizes are the
    sizes; the guard words past the last row and size stay untouched."""
    torch = torch_cuda
    stride = 37
    sk = _export_case(torch, ew, stride)
    n = len(sk)
    d, st, sz = (_device_sketch_arrays if ew == 1 else _device_wide_arrays)(torch, sk)
    guard = 0x0123456789ABCDEF
    dst = torch.full((n * stride * ew + 3,), guard, dtype=torch.int64, device="cuda:0")
    dst_sz = torch.full((n + 2,), -5, dtype=torch.int32, device="cuda:0")
    ctx.sketches_export(d.data_ptr(), st.data_ptr(), sz.data_ptr(), n, dst.data_ptr(), stride, dst_sz.data_ptr(),
                        elem_words=ew)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().view(np.uint64)
    want = np.full((n, stride * ew), U64_MAX, dtype=np.uint64)
    for i, s in enumerate(sk):
        want[i, :len(s) * ew] = s.reshape(-1)
    assert np.array_equal(got[:n * stride * ew].reshape(n, stride * ew), want)
    assert (got[n * stride * ew:] == guard).all()
    assert dst_sz.tolist() == [len(s) for s in sk] + [-5, -5]


@pytest.fixture(scope="module")
def list_stream():
    from test_kmer_list import _genome
    genomes = [_genome(9000, 10 + i, n_runs=i) for i in range(3)] + [_genome(20, 99, 0)]
    stream = b"".join(g.tobytes() + b"\n" for g in genomes)
    offs = [0]
    for g in genomes:
        offs.append(offs[-1] + len(g) + 1)
    return stream, offs


@pytest.mark.parametrize("w,k,c", [(31, 21, 13), (40, 30, 11)])
def test_sketch_set_export_csr(torch_cuda, ctx, list_stream, w, k, c):
    """sks_sketch_set_export_csr: the set's sketches back to back and its sizes,
    equal to sks_sketch_set_copy of every sketch and sks_sketch_set_sizes; the
    words past them stay untouched.  The last genome (20 bases) has no k-mer."""
    import pyoracle as O
    torch = torch_cuda
    stream, offs = list_stream
    d = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
    ss = ctx.sketch_build(d.data_ptr(), len(stream), offs, w, O.mask(w, k, 1), sksffi.SKS_FRAC_MOD, c)
    ew, n = ss.elem_words, ss.n
    assert ew == (1 if w <= 32 else 2)
    sizes = ss.sizes()
    total = int(sizes.astype(np.int64).sum())
    assert sizes[-1] == 0 and total > 500
    data = torch.full((total * ew + 2,), 0x77, dtype=torch.int64, device="cuda:0")
    out_sz = torch.full((n + 1,), -3, dtype=torch.int32, device="cuda:0")
    sksffi.check(sksffi.lib().sks_sketch_set_export_csr(ss.h, ctypes.c_void_p(data.data_ptr()),
                                                        ctypes.c_void_p(out_sz.data_ptr())))
    torch.cuda.synchronize()
    assert out_sz.tolist() == [int(x) for x in sizes] + [-3]
    got = data.cpu().numpy().view(np.uint64)
    assert (got[total * ew:] == 0x77).all()
    rows = got[:total * ew].reshape(total, ew)
    o = 0
    for i in range(n):
        want = ss.sketch(i)
        assert np.array_equal(rows[o:o + len(want)], want[:, :ew]), i
        o += len(want)
    assert o == total
    ss.free()


@pytest.mark.parametrize("w,k,c", [(31, 21, 13), (40, 30, 11)])
def test_kmer_list_device_arrays(torch_cuda, ctx, list_stream, w, k, c):
    """sks_kmer_list_device_positions / _bits: the list's device arrays hold what
    sks_kmer_list_copy returns (which test_kmer_list.py compares with the oracle
    for these inputs), one narrow and one wide list."""
    import pyoracle as O
    torch = torch_cuda
    L = sksffi.lib()
    stream, offs = list_stream
    m = O.mask(w, k, 1)
    d = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
    seg = np.ascontiguousarray(offs, dtype=np.uint64)
    pol = sksffi.Policy(sksffi.SKS_FRAC_MOD, 0, c, 1)
    h = ctypes.c_void_p()
    sksffi.check(L.sks_kmer_list_build(ctx.h, ctypes.c_void_p(d.data_ptr()), len(stream), seg.ctypes.data,
                                       len(seg) - 1, w, sksffi._mask_arr(m), ctypes.byref(pol), ctypes.byref(h)))
    try:
        total = int(L.sks_kmer_list_total(h))
        assert total > 500
        pos = np.zeros(total, np.uint64)
        bits = np.zeros(4 * total, np.uint64)
        sksffi.check(L.sks_kmer_list_copy(h, pos.ctypes.data, bits.ctypes.data))
        p_pos, p_bits = L.sks_kmer_list_device_positions(h), L.sks_kmer_list_device_bits(h)
        assert p_pos and p_bits
        d_pos = torch.as_tensor(sksffi._DeviceArray(p_pos, total, "<i8"), device="cuda:0").cpu().numpy()
        d_bits = torch.as_tensor(sksffi._DeviceArray(p_bits, 4 * total, "<i8"), device="cuda:0").cpu().numpy()
    finally:
        L.sks_kmer_list_free(h)
    assert np.array_equal(d_pos.view(np.uint64), pos) and np.array_equal(d_bits.view(np.uint64), bits)
    wpos, wbits, counts = ctx.kmer_list(d.data_ptr(), len(stream), offs, w, m, c)
    assert np.array_equal(pos, wpos) and np.array_equal(bits.reshape(-1, 4), wbits) and int(counts.sum()) == total
    assert (np.diff(pos.astype(np.int64)) >= 0).all() and (bits.reshape(-1, 4)[:, 3] != 0).any() == (w > 32)


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available()
    which = sys.argv[1]
    cx = sksffi.Context(0)
    for case_name, wld in CHILD_WORLDS:
        cs = case_of(case_name)
        rf = Reference(torch, cx, cs)
        for native_route in (True, False):
            with pytest.MonkeyPatch.context() as mp:
                fx = replay_world(torch, cs, rf, wld, make_ops(cx, cs.ew, native=native_route), mp)
            assert_premise(case_name, wld, fx)
            assert_child_premise(which, cs, fx)
    cx.close()
    print(f"rank replay child {which} ok")
