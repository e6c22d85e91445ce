"""CPU: the arithmetic of sks_sketch_set_merge (csrc/merge_plan.hpp) through
tests/cpp/merge_plan_test.cpp, a plain C++ program without HIP or libsks built
here with the address and undefined-behaviour sanitizers: the merge-path
partition the kernel cuts its tiles with, exhaustively over small sorted arrays
against std::merge, and the round planner against values worked out by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "merge_plan_test.cpp")
INC = os.path.join(ROOT, "spaced-kmer-sketching_amd", "csrc")


def test_merge_plan(tmp_path):
    exe = tmp_path / "merge_plan_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "merge plan ok" in r.stdout
