"""The narrow scan's canonical minimum, min(F & M, R & M), against the oracle,
bit-exactly, at both of its instantiations.

For w <= 31 the masked words are below 2^62 and the narrow FracMinHash and
bottom-s kernels take their minimum with one v_min_f64 on the bit patterns
(finite, non-negative doubles order as their bit patterns do); w = 32 uses bit
63 and keeps the 64-bit compare and select.  The inputs, about three tiles per
case, hold what a floating-point minimum could get wrong if an assumption
failed: poly-A and poly-T runs (canonical value 0: a zero double), windows
whose masked forward and reverse words tie (reverse-palindromic (ACGT)^n runs
for even w; X + G + revcomp(X) blocks under a mask without the middle position
for odd w), and k-mers whose high bases are all A (values below 2^52:
denormal patterns, which must come through unflushed), among random bases
(tests/test_unsigned_min_as_f64.py checks on the CPU that the inputs hold them).
Policies: FracMinHash at c = 1 (the plain kernel, every window kept) and c = 8
(the pre-filter kernel), and bottom-s.
"""
import numpy as np
import pytest

import pyoracle as O
import sksffi
import synth

pytestmark = pytest.mark.gpu

TILE = 4096
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(b):
    return b.translate(COMP)[::-1]


def genome(w):
    rng = np.random.default_rng(100 + w)
    rnd = lambda n: synth.ACGT[rng.integers(0, 4, n)].tobytes()
    parts = [rnd(1500), b"A" * 300, b"T" * 300, rnd(100), b"ACGT" * 64, rnd(100)]
    half = w // 2
    for _ in range(40):  # masked ties for odd w (and plain ones when w is even: X + revcomp(X))
        x = rnd(half)
        parts += [x, b"G" if w % 2 else b"", revcomp(x), rnd(int(rng.integers(1, 9)))]
    for _ in range(100):  # high bases all A: F below 2^(2w - 14)
        parts += [b"A" * 7, rnd(w + 5)]
    for _ in range(20):  # and the same on the reverse strand
        parts += [rnd(w + 5), b"T" * 7]
    body = b"".join(parts)
    return body + rnd(3 * TILE - 40 - len(body))


def masks(w):
    """(id, mask): the generator's k < w mask, and for odd w one without the
    middle position, under which the X + G + revcomp(X) blocks tie."""
    k = {5: 3, 16: 11, 31: 21, 32: 22}[w]
    out = [(f"k{k}", O.mask(w, k, 0))]
    if w % 2:
        out.append(("nomiddle", synth.positions_mask(p for p in range(w) if p != w // 2)))
    return out


CASES = [(w, mid, m) for w in (5, 16, 31, 32) for mid, m in masks(w)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.close()


_genomes = {}


def _genome(w):
    if w not in _genomes:
        g = genome(w)
        assert 2 * TILE < len(g) <= 3 * TILE
        _genomes[w] = g
    return _genomes[w]


@pytest.mark.parametrize("kind,param", [("frac", 1), ("frac", 8), ("bottom", 500)],
                         ids=["frac_c1", "frac_c8", "bottom_s500"])
@pytest.mark.parametrize("w,mid,m", CASES, ids=[f"w{w}_{mid}" for w, mid, _ in CASES])
def test_canonical_min(gpu, w, mid, m, kind, param):
    torch, ctx = gpu
    g = _genome(w)
    stream = g + b"\n"
    dev = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
    k = sksffi.SKS_FRAC_MOD if kind == "frac" else sksffi.SKS_BOTTOM_S
    ss = ctx.sketch_build(dev.data_ptr(), len(stream), [0, len(stream)], w, m, k, param)
    want, nw = O.sketch(O.cut_runs(g), w, m, kind, param)
    assert int(ss.windows()[0]) == nw
    assert int(ss.sizes()[0]) == len(want)
    assert np.array_equal(ss.sketch(0), want)
    if kind == "frac" and param == 1 and w == 31:
        lo = want[:, 0]
        assert lo[0] == 0 and (lo < np.uint64(1 << 52)).sum() > 100  # zero and denormal patterns are in the sketch
