"""CPU: the sketch build's planning arithmetic (csrc/build_plan.hpp) through
tests/cpp/plan_test.cpp, a plain C++ program without HIP or libsks: thresholds
and capacities, the retry escalation, the fused FracMinHash bucket count and
the choice of post-processing path, against values worked out by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_build_plan():
    subprocess.run(["make", "-s", "-C", CPP, "build/plan_test"], check=True)
    r = subprocess.run([os.path.join(CPP, "build", "plan_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan ok" in r.stdout
