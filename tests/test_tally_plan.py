"""CPU: the arithmetic of sks_sketch_set_tally (csrc/tally_plan.hpp) through
tests/cpp/tally_plan_test.cpp, a plain C++ program without HIP or libsks built
here with the address and undefined-behaviour sanitizers: the keep rule and the
run-end search the kernel runs, exhaustively over small sorted multisets against
a naive run-length count and with a reader that refuses positions beyond the
group, and the command line's fraction-to-count rule against hand-worked values."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tally_plan_test.cpp")
INC = os.path.join(ROOT, "spaced-kmer-sketching_amd", "csrc")


def test_tally_plan(tmp_path):
    exe = tmp_path / "tally_plan_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tally plan ok" in r.stdout
