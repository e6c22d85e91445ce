"""Source hash of libsks.so: sha256 over the library's source files (every
csrc/*.hip, csrc/*.cpp, csrc/*.hpp, cpp/*.cpp, cpp/*.hpp and include/sks.h),
each as its package-relative path, a NUL, its bytes and a NUL, in sorted path
order; first 16 hex digits.  The Makefile compiles it into the library
(sks_build_info) and tests/conftest.py recomputes it, so a test run proves the
loaded binary was built from the sources it sits next to."""
import glob
import hashlib
import os
import re
import sys

PKG = os.path.dirname(os.path.abspath(__file__))


def files():
    pats = ["csrc/*.hip", "csrc/*.cpp", "csrc/*.hpp", "cpp/*.cpp", "cpp/*.hpp", "../include/sks.h"]
    out = []
    for p in pats:
        out += [os.path.relpath(f, PKG) for f in glob.glob(os.path.join(PKG, p))]
    return sorted(out)


def include_closure(roots):
    """The roots and every file they reach through quoted #include "..." lines
    that name a file in csrc/ (package-relative paths, sorted)."""
    seen, todo = set(), list(roots)
    while todo:
        rel = todo.pop()
        if rel in seen:
            continue
        seen.add(rel)
        with open(os.path.join(PKG, rel), encoding="utf-8") as f:
            for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                if os.path.isfile(os.path.join(PKG, "csrc", name)):
                    todo.append("csrc/" + name)
    return sorted(seen)


# the sources the fused scan kernel is compiled from (profiles/rNN/traffic.json
# records this hash; bench.py uses a traffic figure only when it still matches)
SCAN_FILES = include_closure(["csrc/scan.hip"])


def source_hash(rels=None):
    h = hashlib.sha256()
    for rel in (files() if rels is None else sorted(rels)):
        h.update(rel.encode() + b"\0")
        with open(os.path.join(PKG, rel), "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    return h.hexdigest()[:16]


# the sources of the all-pairs join (k_join and its layout build):
# profiles/rNN/pair_lds.json records this hash
JOIN_FILES = include_closure(["csrc/join.hip", "csrc/layout.hip"])


def scan_hash():
    return source_hash(SCAN_FILES)


def join_hash():
    return source_hash(JOIN_FILES)


if __name__ == "__main__":
    sys.stdout.write(source_hash())
