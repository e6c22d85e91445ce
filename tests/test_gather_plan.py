"""CPU: the arithmetic of sks_gather (csrc/gather_plan.hpp) through
tests/cpp/gather_plan_test.cpp, a plain C++ program without HIP or libsks built
here with the address and undefined-behaviour sanitizers: the round's key
against a sort by (-count, index), the bitmap's tail mask for every size from 1
to 130, the bounded search against std::lower_bound on 64- and 128-bit arrays,
the map of list chunks to scoring workgroups and the round-group plan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "gather_plan_test.cpp")
INC = os.path.join(ROOT, "spaced-kmer-sketching_amd", "csrc")


def test_gather_plan(tmp_path):
    exe = tmp_path / "gather_plan_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gather plan ok" in r.stdout
