"""CPU: the scratch carver (csrc/scratch_carve.hpp) through
tests/cpp/carve_test.cpp, a plain C++ program without HIP or libsks: regions
256-byte aligned, in order, not overlapping, at least their requested size,
and at the offsets the join-layout scratch has always had."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_carver_offsets():
    subprocess.run(["make", "-s", "-C", CPP, "build/carve_test"], check=True)
    r = subprocess.run([os.path.join(CPP, "build", "carve_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "carve ok: 5 shapes" in r.stdout
