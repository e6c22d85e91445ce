"""CPU: the host arithmetic of the join (csrc/join_plan.hpp) through
tests/cpp/join_plan_test.cpp, a plain C++ program without HIP or libsks built
here with the address and undefined-behaviour sanitizers.  For every bucket
count 2^0 .. 2^14, tile counts from 1 to 5 * 10^6 and the default rule or a
forced workgroup total (one, three per tile, 2^40): every group holds a bucket
and no bucket is lost, a launch stays below 2^22 workgroups, and the default
rule gives the groups per tile the tuned cases have always had.  The launches
of a sliced call tile its range in order with the packed-output offset of each,
the diagonal-last condition, the contiguous / piecewise kernel choice and the
bucket count of a layout (14 above 21 760 elements at capacity 1024)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "join_plan_test.cpp")
INC = os.path.join(ROOT, "spaced-kmer-sketching_amd", "csrc")


def test_join_plan(tmp_path):
    exe = tmp_path / "join_plan_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "join plan ok" in r.stdout
