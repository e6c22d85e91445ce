"""The count -> containment / ANI kernels (ani.hip) through their C entry
points, against the host's double arithmetic (sks_ani_from_counts: the
reference's containment and binomial_estimator) and numpy's division.

sks_ani_matrix, with and without the containment output, at n = 1, 63, 64 and
130 (one thread per ordered pair, 256 a workgroup: fewer cells than a
workgroup, a row length that is no multiple of it, more than one workgroup),
on counts with zeros, with counts[i][j] == counts[i][i] (containment exactly 1)
and with a zero diagonal entry (an empty set: its row and column are 0).
sks_ani_tiles on packed tiles of 130 sets, the last block ragged: plane 0 is
[r][c] with |S_i| as denominator, plane 1 the transposed [c][r] with |S_j|,
cells past n are 0.0 whatever the packed counts hold there.
"""
import numpy as np
import pytest

import sksffi
from test_gpu_parity import torch_cuda, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

K_ONES = 21
TILE = 64


def counts_case(n, seed=81):
    """A symmetric count matrix with diag = |S_i| in 1 .. 700 (one of them 0)."""
    rng = np.random.default_rng(seed + n)
    d = rng.integers(1, 701, size=n).astype(np.int64)
    u = rng.random((n, n))
    c = np.floor(np.minimum(u, u.T) * np.minimum.outer(d, d)).astype(np.int64)
    z = rng.random((n, n))
    c[np.minimum(z, z.T) < 0.15] = 0
    full = []
    for i in range(0, n - 1, 7):  # S_i within S_j: counts[i][j] == counts[i][i]
        j = i + 1 + int(rng.integers(0, n - 1 - i))
        if d[i] <= d[j]:
            c[i, j] = c[j, i] = d[i]
            full.append((i, j))
    if n >= 3:
        e = n // 2  # an empty set
        d[e] = 0
        c[e, :] = 0
        c[:, e] = 0
        full = [(i, j) for i, j in full if e not in (i, j)]
    np.fill_diagonal(c, d)
    assert np.array_equal(c, c.T) and (c <= np.minimum.outer(d, d)).all()
    if n >= 63:
        assert len(full) >= 3 and (c == 0).sum() > n and (c > 0).sum() > n * n // 2
    return c, d, full


def host_reference(c, d, k):
    n = len(d)
    cont, ani = sksffi.ani_from_counts(c.reshape(-1), np.repeat(d, n), k)
    cont, ani = cont.reshape(n, n), ani.reshape(n, n)
    quot = np.divide(c.astype(np.float64), d.astype(np.float64)[:, None], out=np.zeros((n, n)), where=c != 0)
    assert np.array_equal(cont, quot)  # the host's containment is counts / diag, 0 where the count is 0
    return quot, ani


def device_rows(torch, ctx, c, k):
    n = len(c)
    dense = torch.from_numpy(c.astype(np.int32)).to("cuda:0")
    rows = torch.full((n, n), -2.0, dtype=torch.float64, device="cuda:0")
    ctx.ani_rows(dense.data_ptr(), n, 0, n, k, rows.data_ptr())
    torch.cuda.synchronize()
    return rows.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 130])
def test_ani_matrix(torch_cuda, ctx, n):
    torch = torch_cuda
    c, d, full = counts_case(n)
    want_cont, host_ani = host_reference(c, d, K_ONES)
    rows = device_rows(torch, ctx, c, K_ONES)
    dense = torch.from_numpy(c.astype(np.int32)).to("cuda:0")
    for with_cont in (True, False):
        ani = torch.full((n * n + 2,), -3.0, dtype=torch.float64, device="cuda:0")
        cont = torch.full((n * n + 2,), -4.0, dtype=torch.float64, device="cuda:0")
        ctx.ani_matrix(dense.data_ptr(), n, K_ONES, ani.data_ptr(), cont.data_ptr() if with_cont else None)
        torch.cuda.synchronize()
        got, got_cont = ani.cpu().numpy(), cont.cpu().numpy()
        assert (got[n * n:] == -3.0).all() and (got_cont[n * n:] == -4.0).all()  # nothing past the matrix
        got = got[:n * n].reshape(n, n)
        assert np.array_equal(got.view(np.int64), rows.view(np.int64)), "sks_ani_rows(0, n)"
        assert np.abs(got - host_ani).max() <= 1e-9
        assert np.array_equal(got == 0.0, c == 0) and (got[c > 0] > 0).all() and got.max() <= 1.0
        if with_cont:
            assert np.array_equal(got_cont[:n * n].reshape(n, n).view(np.int64), want_cont.view(np.int64))
        else:
            assert (got_cont == -4.0).all()
        for i, j in full:
            assert got[i, j] == 1.0 and c[i, j] == d[i]
        assert np.array_equal(np.diag(got), (d > 0).astype(np.float64))
    if n >= 3:
        assert d[n // 2] == 0 and not rows[n // 2].any() and not rows[:, n // 2].any()


def test_ani_tiles(torch_cuda, ctx):
    torch = torch_cuda
    n = 130
    tiles = [(0, 0), (0, 2), (1, 2), (2, 2)]
    c, d, _ = counts_case(n)
    _, host_ani = host_reference(c, d, K_ONES)
    rows = device_rows(torch, ctx, c, K_ONES)
    assert np.abs(rows - host_ani).max() <= 1e-9
    nb = (n + TILE - 1) // TILE
    c_pad = np.full((nb * TILE, nb * TILE), 12345, dtype=np.int64)  # cells past n: not to be converted
    c_pad[:n, :n] = c
    rows_pad = np.zeros((nb * TILE, nb * TILE))
    rows_pad[:n, :n] = rows
    packed = np.stack([c_pad[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE] for I, J in tiles]).astype(np.int32)
    d_packed = torch.from_numpy(packed).to("cuda:0")
    d_tiles = torch.tensor(tiles, dtype=torch.int32, device="cuda:0")
    d_sizes = torch.from_numpy(d.astype(np.int32)).to("cuda:0")
    out = torch.full((len(tiles) * 2 * TILE * TILE + 2,), -7.0, dtype=torch.float64, device="cuda:0")
    ctx.ani_tiles(d_packed.data_ptr(), d_tiles.data_ptr(), len(tiles), n, d_sizes.data_ptr(), K_ONES, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[-2:] == -7.0).all()
    got = got[:-2].reshape(len(tiles), 2, TILE, TILE)
    for t, (I, J) in enumerate(tiles):
        rs, cs = slice(I * TILE, (I + 1) * TILE), slice(J * TILE, (J + 1) * TILE)
        # plane 0: [r][c] = ANI(i, j), |S_i| below; plane 1: [c][r] = ANI(j, i), |S_j| below
        assert np.array_equal(got[t, 0].view(np.int64), rows_pad[rs, cs].view(np.int64)), (I, J, "plane 0")
        assert np.array_equal(got[t, 1].view(np.int64), rows_pad[cs, rs].view(np.int64)), (I, J, "plane 1")
        assert np.abs(got[t, 0][:n - I * TILE, :n - J * TILE] - host_ani[rs, cs]).max() <= 1e-9
        assert np.abs(got[t, 1][:n - J * TILE, :n - I * TILE] - host_ani[cs, rs]).max() <= 1e-9
    ragged = got[1]  # tile (0, 2): columns 2 .. 63 of plane 0 and rows 2 .. 63 of plane 1 lie past n
    assert not ragged[0][:, n - 2 * TILE:].any() and not ragged[1][n - 2 * TILE:, :].any()
    assert ragged[0][:, :n - 2 * TILE].any() and (got[1, 0] != got[1, 1].T).any()  # the two denominators differ
