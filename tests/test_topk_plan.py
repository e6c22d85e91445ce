"""CPU: the arithmetic of sks_search_topk (csrc/topk_plan.hpp) through
tests/cpp/topk_plan_test.cpp, a plain C++ program without HIP or libsks built
here with the address and undefined-behaviour sanitizers: the order is strict
and total, the denominator per rank kind, eligibility, and the sorted-list
update against std::sort of all candidates on inputs dense with ties, for every
k from 1 to 64, fed in several orders and cut into several batches."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "topk_plan_test.cpp")
INC = os.path.join(ROOT, "spaced-kmer-sketching_amd", "csrc")


def test_topk_plan(tmp_path):
    exe = tmp_path / "topk_plan_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "topk plan ok" in r.stdout
