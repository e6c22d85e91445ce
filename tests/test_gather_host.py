"""CPU: the gather entry points of the C ABI are exported and declared, a null
context is refused on the host, before any device is touched, with a message and
a zeroed hit count, and sks_gather_hit is 32 bytes."""
import ctypes as C
import os
import re

import sksffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported_and_declared():
    lib = C.CDLL(sksffi.LIB_PATH)
    with open(os.path.join(ROOT, "include", "sks.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for s in ("sks_gather", "sks_gather_sets", "sks_ctx_set_gather_rounds"):
        assert hasattr(lib, s), s
        assert s in sksffi.EXPORTED
        assert re.search(r"\bint\s+%s\s*\(" % s, text), f"{s} is not declared in include/sks.h"
    assert lib.sks_abi_version() == 3


def test_null_context_is_refused_without_a_device():
    L = sksffi.lib()
    n = C.c_uint64(7)
    un = C.c_uint32(0)
    rc = L.sks_gather_sets(None, None, 0, None, 1, 0, None, 0, C.byref(n), C.byref(un))
    assert rc == sksffi.SKS_E_ARG and n.value == 0
    assert b"sks_gather_sets: null ctx" in L.sks_last_error()
    n = C.c_uint64(7)
    rc = L.sks_gather(None, None, 5, None, None, None, 3, 10, 30, 1, 21, 1, 0, None, 0, C.byref(n), None)
    assert rc == sksffi.SKS_E_ARG and n.value == 0
    assert b"sks_gather: null ctx" in L.sks_last_error()
    # and without a place for the count
    assert L.sks_gather_sets(None, None, 0, None, 1, 0, None, 0, None, None) == sksffi.SKS_E_ARG
    assert L.sks_gather(None, None, 5, None, None, None, 3, 10, 30, 1, 21, 1, 0, None, 0, None, None) == \
        sksffi.SKS_E_ARG
    assert L.sks_ctx_set_gather_rounds(None, 1) == sksffi.SKS_E_ARG
    assert b"sks_ctx_set_gather_rounds: null ctx" in L.sks_last_error()


def test_hit_record_is_32_bytes():
    assert C.sizeof(sksffi.GatherHit) == 32
    assert sksffi.GATHER_HIT_DTYPE.itemsize == 32
    # the numpy view and the C structure agree field by field
    for name, _ in sksffi.GatherHit._fields_:
        assert getattr(sksffi.GatherHit, name).offset == sksffi.GATHER_HIT_DTYPE.fields[name][1], name
    with open(os.path.join(ROOT, "include", "sks.h")) as f:
        assert re.search(r"typedef struct sks_gather_hit \{\s*/\* 32 bytes \*/", f.read())
