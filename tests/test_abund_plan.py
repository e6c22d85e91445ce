"""CPU: the arithmetic of the k-mer abundances (csrc/abund_plan.hpp) through
tests/cpp/abund_plan_test.cpp, a plain C++ program without HIP or libsks built
here with the address and undefined-behaviour sanitizers: run lengths from the
runs' first indices and the segments' ends, exhaustively over small sorted
multisets cut into segments (empty ones included) against a naive count, the
clamp at UINT32_MAX, the keep rule at its corners and the padded size of the
sketch file's abundance section."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "abund_plan_test.cpp")
INC = os.path.join(ROOT, "spaced-kmer-sketching_amd", "csrc")


def test_abund_plan(tmp_path):
    exe = tmp_path / "abund_plan_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "abund plan ok" in r.stdout
