"""The identity behind the narrow scan's one-op canonical minimum, on the CPU:
for unsigned 64-bit values below 2^62 the IEEE-754 double with the same bit
pattern is finite and non-negative (bit 63 clear; bit 62 clear, so the exponent
field is never all ones: no NaN, no infinity), and such doubles order exactly
as their bit patterns do, zero and the denormals (below 2^52) included.  So the
floating-point minimum of the views is the unsigned minimum, bit for bit.
numpy's minimum on float64 does not flush denormals, like the kernels' float
mode.  Also checks that the inputs of tests/test_scan_canonical_min.py hold the
edge values its docstring names."""
import numpy as np

import pyoracle as O
import test_scan_canonical_min as T

LIM = 1 << 62


def _pairs():
    rng = np.random.default_rng(20)
    a = rng.integers(0, LIM, 1_000_000, dtype=np.uint64)
    b = rng.integers(0, LIM, 1_000_000, dtype=np.uint64)
    # small values too: uniform draws below 2^62 are almost never denormal patterns
    sh = rng.integers(0, 62, 1_000_000).astype(np.uint64)
    a[::2] >>= sh[::2]
    b[::3] >>= sh[::3]
    edges = np.array([0, 1, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, LIM - 1], dtype=np.uint64)
    ea, eb = np.meshgrid(edges, edges)  # every edge against every edge: the equal pairs too
    a = np.concatenate([a, ea.ravel(), a[:1000]])
    b = np.concatenate([b, eb.ravel(), a[:1000]])
    return a, b


def test_f64_minimum_of_bit_patterns_is_the_unsigned_minimum():
    a, b = _pairs()
    assert int(a.max()) < LIM and int(b.max()) < LIM
    fa, fb = a.view(np.float64), b.view(np.float64)
    assert not np.isnan(fa).any() and not np.isnan(fb).any()
    assert np.isfinite(fa).all() and np.isfinite(fb).all()
    assert not np.signbit(fa).any() and not np.signbit(fb).any()
    got = np.minimum(fa, fb).view(np.uint64)
    assert np.array_equal(got, np.minimum(a, b))
    assert ((a < (1 << 52)) & (a > 0)).sum() > 1000  # denormal patterns were among the operands
    # and the boundary the kernels respect: with bit 62 set the view can be a NaN
    assert np.isnan(np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)).all()


def test_canonical_min_inputs_hold_the_edge_values():
    """The oracle's windows of the w = 31 input include canonical 0, ties under
    the mask without the middle position, and values below 2^52; all below 2^62."""
    w = 31
    m = dict(T.masks(w))["nomiddle"]
    rows = O.windows(O.cut_runs(T.genome(w)), w, m)
    # rows: F lo, hi, R lo, hi, C lo, hi, ...; narrow windows have zero high words
    assert not rows[:, 1].any() and not rows[:, 3].any() and not rows[:, 5].any()
    F, R, Cn = rows[:, 0] & np.uint64(m), rows[:, 2] & np.uint64(m), rows[:, 4]
    assert np.array_equal(Cn, np.minimum(F, R))
    assert (Cn == 0).sum() >= 2 * (300 - w)
    assert ((F == R) & (Cn != 0)).sum() >= 40
    assert ((Cn > 0) & (Cn < np.uint64(1 << 52))).sum() >= 100
    assert int(Cn.max()) < LIM
    for w2 in (5, 16, 32):  # even w: the (ACGT)^n run and the X + revcomp(X) blocks tie under any mask
        m2 = T.masks(w2)[0][1]
        r2 = O.windows(O.cut_runs(T.genome(w2)), w2, m2)
        assert ((r2[:, 0] & np.uint64(m2)) == (r2[:, 2] & np.uint64(m2))).sum() >= (40 if w2 % 2 == 0 else 0)
