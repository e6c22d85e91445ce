"""CPU: sks_sketch_set_filter refuses null arguments before any device is touched
(only the library is needed), and the binding lists the symbol and its kinds."""
import ctypes as C

import sksffi


def test_null_arguments_without_gpu():
    lib = sksffi.lib()
    fake = C.c_void_p(8)  # never dereferenced: a null argument is found first
    fo = (C.c_uint32 * 1)(0)
    for ctx, src, filt in [(None, None, None), (None, fake, fake), (fake, None, fake), (fake, fake, None)]:
        for kind in (sksffi.SKS_FILTER_SUBTRACT, sksffi.SKS_FILTER_INTERSECT):
            out = C.c_void_p(12345)
            assert lib.sks_sketch_set_filter(ctx, src, filt, fo, kind, C.byref(out)) == sksffi.SKS_E_ARG
            assert b"sks_sketch_set_filter" in lib.sks_last_error() and b"null" in lib.sks_last_error()
            assert out.value is None
    assert lib.sks_sketch_set_filter(fake, fake, fake, fo, 0, None) == sksffi.SKS_E_ARG
    assert b"null" in lib.sks_last_error()


def test_binding_names_the_symbol_and_kinds():
    assert "sks_sketch_set_filter" in sksffi.EXPORTED
    assert (sksffi.SKS_FILTER_SUBTRACT, sksffi.SKS_FILTER_INTERSECT) == (0, 1)
    assert sksffi.FILTER_NONE == 2**32 - 1
    for name in ("filter", "subtract", "intersect"):
        assert callable(getattr(sksffi.Context, name))
