"""CPU: the rules the set-level calls share (csrc/set_rules.hpp) through
tests/cpp/set_rules_test.cpp, a plain C++ program without HIP or libsks built
here with the address and undefined-behaviour sanitizers: the first field two
sets differ in under both param rules, the positions a mask selects, and the
one retry with sampled group bounds after an invalid layout."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "set_rules_test.cpp")
INC = [os.path.join(ROOT, "spaced-kmer-sketching_amd", "csrc"), os.path.join(ROOT, "include")]


def test_set_rules(tmp_path):
    exe = tmp_path / "set_rules_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC[0], "-I", INC[1], SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "set rules ok" in r.stdout
