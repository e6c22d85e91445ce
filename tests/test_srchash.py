"""CPU: the per-kernel source hashes (srchash.scan_hash / join_hash) follow the
kernels' own include closure, so a change to another unit's header leaves them
alone while the library's source_hash() still sees it.  Runs on a copy of
srchash.py and csrc/ in a temporary directory."""
import importlib.util
import os
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spaced-kmer-sketching_amd")


def _load(pkg):
    spec = importlib.util.spec_from_file_location("srchash_copy", os.path.join(pkg, "srchash.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _hashes(pkg):
    m = _load(pkg)
    return m.source_hash(), m.scan_hash(), m.join_hash()


def test_kernel_hashes_follow_their_includes(tmp_path):
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    shutil.copy(os.path.join(PKG, "srchash.py"), pkg / "srchash.py")
    shutil.copytree(os.path.join(PKG, "csrc"), pkg / "csrc")

    def touch(name):
        with open(pkg / "csrc" / name, "a") as f:
            f.write("// a comment\n")

    m = _load(str(pkg))
    assert "csrc/sks_hash.hpp" in m.SCAN_FILES and "csrc/scan.hip" in m.SCAN_FILES
    assert {"csrc/join.hip", "csrc/layout.hip", "csrc/join_common.hpp"} <= set(m.JOIN_FILES)

    src0, scan0, join0 = _hashes(str(pkg))
    touch("downsample.hpp")  # another unit's header: the library changed, the two kernels did not
    src1, scan1, join1 = _hashes(str(pkg))
    assert src1 != src0 and scan1 == scan0 and join1 == join0
    touch("wave_prims.hpp")  # the join's and the layout build's primitives
    src2, scan2, join2 = _hashes(str(pkg))
    assert src2 != src1 and join2 != join1 and scan2 == scan1
    touch("scan.hpp")
    src3, scan3, join3 = _hashes(str(pkg))
    assert src3 != src2 and scan3 != scan2 and join3 == join2
