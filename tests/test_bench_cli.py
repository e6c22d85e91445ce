"""bench.py's --dump-outputs files: the u64 sketch survives the float64 .npy
files bit for bit (high and low 32-bit halves), and config 3's dump stays
under the 64 MB limit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class _FakeSet:
    """What dump_c3_outputs reads of a sksffi.SketchSet."""

    def __init__(self, values, windows):
        self.v = np.asarray(values, dtype=np.uint64)
        self.w = windows

    def sketch(self, i):
        assert i == 0
        return np.stack([self.v, np.zeros_like(self.v)], axis=1)

    def sizes(self):
        return np.array([self.v.size], dtype=np.uint32)

    def windows(self):
        return np.array([self.w], dtype=np.uint64)


def test_dump_outputs_roundtrip_is_exact(tmp_path):
    import bench
    # values that a float64 cannot hold whole: all 64 bits set, 2^53 + 1, 2^63 + 1
    vals = [0, 1, 0xFFFFFFFF, 1 << 32, (1 << 53) + 1, (1 << 63) + 1, 0xFFFFFFFFFFFFFFFF]
    d = tmp_path / "out" / "nested"
    bench.dump_c3_outputs(str(d), _FakeSet(vals, 2_999_036_400))
    files = sorted(os.listdir(d))
    assert files == ["sizes.npy", "sketch_hi32.npy", "sketch_lo32.npy", "windows.npy"]
    arrs = {f: np.load(d / f) for f in files}
    assert all(a.dtype == np.float64 for a in arrs.values())
    hi = arrs["sketch_hi32.npy"].astype(np.uint64)
    lo = arrs["sketch_lo32.npy"].astype(np.uint64)
    back = (hi << np.uint64(32)) | lo
    assert back.tolist() == vals
    assert arrs["sizes.npy"].tolist() == [len(vals)]
    assert arrs["windows.npy"].tolist() == [2_999_036_400]


def test_config3_dump_fits_the_size_limit():
    import bench
    # FracMinHash 1/1000 of the config-3 windows, 16 B per element in the two files
    expected = bench.c3_windows() / bench.C3_FRAC
    assert expected * 16 * 1.05 < 64e6
