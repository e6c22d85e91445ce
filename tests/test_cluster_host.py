"""CPU: the cluster entry points of the C ABI are exported and declared, and a
null context is refused on the host, before any device is touched, with a
message and a zeroed cluster count."""
import ctypes as C
import os
import re

import sksffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported_and_declared():
    lib = C.CDLL(sksffi.LIB_PATH)
    with open(os.path.join(ROOT, "include", "sks.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for s in ("sks_cluster", "sks_cluster_set"):
        assert hasattr(lib, s), s
        assert s in sksffi.EXPORTED
        assert re.search(r"\bint\s+%s\s*\(" % s, text), f"{s} is not declared in include/sks.h"
    assert lib.sks_abi_version() == 3


def test_null_context_is_refused_without_a_device():
    L = sksffi.lib()
    n = C.c_uint32(7)
    rc = L.sks_cluster_set(None, None, 0.5, 1, None, None, C.byref(n))
    assert rc == sksffi.SKS_E_ARG and n.value == 0
    assert b"sks_cluster_set: null ctx" in L.sks_last_error()
    n = C.c_uint32(7)
    rc = L.sks_cluster(None, None, None, None, 5, 10, 50, 1, 21, 0.5, 1, None, None, C.byref(n))
    assert rc == sksffi.SKS_E_ARG and n.value == 0
    assert b"sks_cluster: null ctx" in L.sks_last_error()
    # and without a place for the count
    assert L.sks_cluster_set(None, None, 0.5, 1, None, None, None) == sksffi.SKS_E_ARG
