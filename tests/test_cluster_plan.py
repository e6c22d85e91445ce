"""CPU: the arithmetic of sks_cluster (csrc/cluster_plan.hpp) through
tests/cpp/cluster_plan_test.cpp, a plain C++ program without HIP or libsks built
here with the address and undefined-behaviour sanitizers: the lock-free union by
index against a breadth-first search (every graph on up to 6 vertices, and
random graphs whose edges four threads share), the link rule at its corners,
and the triangle tiles with their batch ranges."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cluster_plan_test.cpp")
INC = os.path.join(ROOT, "spaced-kmer-sketching_amd", "csrc")


def test_cluster_plan(tmp_path):
    exe = tmp_path / "cluster_plan_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cluster plan ok" in r.stdout
