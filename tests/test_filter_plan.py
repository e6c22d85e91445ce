"""CPU: the arithmetic of sks_sketch_set_filter (csrc/filter_plan.hpp) through
tests/cpp/filter_plan_test.cpp, a plain C++ program without HIP or libsks built
here with the address and undefined-behaviour sanitizers: the bracket of a chunk
in an ascending filter sketch, by one lane's search and by the 64-ary narrowing
a wavefront runs, against std::lower_bound / std::upper_bound on 64- and 128-bit
arrays (sizes 0, 1, 2, 63, 64, 65 and larger, elements that share one word and
differ in the other, chunk ends equal to filter elements), and a replay of the
mark and scatter passes against std::set_difference / std::set_intersection
for chunk-crossing sizes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "filter_plan_test.cpp")
INC = os.path.join(ROOT, "spaced-kmer-sketching_amd", "csrc")


def test_filter_plan(tmp_path):
    exe = tmp_path / "filter_plan_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "filter plan ok" in r.stdout
