"""Sketch files of counted sets (version 3 of the SKSKETCH format documented in
spaced-kmer-sketching_amd/csrc/persist.cpp): the round trip, the bytes of a set
without abundances (version 1, unchanged: rebuilt here from the documentation
by an independent writer), and damaged version-3 files."""
import struct

import numpy as np
import pytest

import sksffi
import synth
from test_abund import Segments, _same_counted, _with_repeats
from test_persist import fnv1a64

FRAC = sksffi.SKS_FRAC_MOD


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = sksffi.Context(0)
    yield torch, c
    c.close()


def _pad8(b):
    return b + b"\0" * (-len(b) % 8)


def _file_bytes(ss, version, names):
    """The documented layout, written from the set's accessors."""
    i = ss.info()
    sizes = ss.sizes()
    total = int(sizes.astype(np.int64).sum())
    table = b"".join(n.encode() + b"\0" for n in names) if names else b""
    mask = i["mask"]
    body = struct.pack("<8sIIiiiiQqQQQQQQ", b"SKSKETCH", version, i["elem_words"], i["window"], i["kind"],
                       i["flavour"], 0, i["param"], i["nonce"], mask & (2**64 - 1), mask >> 64, ss.n, total,
                       len(table), 0)
    body += _pad8(sizes.astype("<u4").tobytes()) + ss.windows().astype("<u8").tobytes()
    for g in range(ss.n):
        body += np.ascontiguousarray(ss.sketch(g)[:, :i["elem_words"]]).astype("<u8").tobytes()
    if version == 3:
        body += _pad8(b"".join(ss.abund(g).astype("<u4").tobytes() for g in range(ss.n)))
    body += table
    return body + struct.pack("<Q", fnv1a64(body))


def _sets(torch, ctx, w, k):
    mask = sksffi.mask_generate(w, k, 0)
    S = Segments(torch, ctx, [_with_repeats(synth.bases(900, 41)), b"", _with_repeats(synth.bases(700, 42)),
                              _with_repeats(synth.bases(500, 43))])
    return S.plain(w, mask, 3), S.counted(w, mask, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(31, 21), (45, 30)], ids=["narrow", "wide"])
def test_round_trip_and_layout(gpu, tmp_path, shape):
    torch, ctx = gpu
    plain, counted = _sets(torch, ctx, *shape)
    names = ["a.fa", "empty", "dir/c.fa", "d"]
    total = int(counted.sizes().astype(np.int64).sum())
    for with_names in (False, True):
        for s in (plain, counted):
            s.set_names(names if with_names else None)
        p_plain, p_counted = tmp_path / f"plain{with_names}.sks", tmp_path / f"counted{with_names}.sks"
        plain.save(p_plain)
        counted.save(p_counted)
        # a set without abundances: version 1, byte for byte the documented layout, same checksum
        raw = p_plain.read_bytes()
        assert struct.unpack_from("<I", raw, 8)[0] == 1
        assert raw == _file_bytes(plain, 1, names if with_names else None)
        # a counted set: version 3, the plain file's sections with the abundances between data and names
        raw3 = p_counted.read_bytes()
        assert struct.unpack_from("<I", raw3, 8)[0] == 3
        assert raw3 == _file_bytes(counted, 3, names if with_names else None)
        o_abund = 96 + ((4 * plain.n + 7) & ~7) + 8 * plain.n + 8 * total * plain.elem_words
        assert raw3[12:o_abund] == raw[12:o_abund]
        assert len(raw3) - len(raw) == (4 * total + 7) & ~7
        back = ctx.load_sketches(p_counted)
        _same_counted(back, counted)
        assert back.names() == (names if with_names else None)
        again = ctx.load_sketches(p_plain)
        assert again.has_abund() == 0
        # a loaded counted set is saved as it was
        back.save(tmp_path / "again.sks")
        assert (tmp_path / "again.sks").read_bytes() == raw3


def _resum(body):
    return body + struct.pack("<Q", fnv1a64(body))


@pytest.mark.gpu
def test_damaged_files(gpu, tmp_path):
    torch, ctx = gpu
    plain, counted = _sets(torch, ctx, 31, 21)
    p = tmp_path / "c.sks"
    counted.save(p)
    raw = p.read_bytes()
    total = int(counted.sizes().astype(np.int64).sum())
    o_abund = 96 + ((4 * counted.n + 7) & ~7) + 8 * counted.n + 8 * total
    assert total >= 100

    def refused(data, word=None):
        bad = tmp_path / "bad.sks"
        bad.write_bytes(data)
        with pytest.raises(sksffi.SksError) as e:
            ctx.load_sketches(bad)
        assert e.value.code == sksffi.SKS_E_IO
        assert word is None or word in str(e.value)

    ok = tmp_path / "ok.sks"
    ok.write_bytes(_resum(raw[:-8]))
    assert ctx.load_sketches(ok).has_abund() == 1  # _resum writes what the library wrote
    # truncated inside the abundance section, with and without a fresh checksum
    refused(raw[:o_abund + 40])
    refused(_resum(raw[:o_abund + 40]))
    # a zero abundance under a valid checksum
    zeroed = bytearray(raw[:-8])
    zeroed[o_abund + 4 * 7:o_abund + 4 * 8] = b"\0\0\0\0"
    refused(_resum(bytes(zeroed)), "abundance")
    # one flipped byte in the section
    flipped = bytearray(raw)
    flipped[o_abund + 13] ^= 0x40
    refused(bytes(flipped), "checksum")
    # version 1 in the header of a version-3 body: the length no longer matches
    as_v1 = bytearray(raw[:-8])
    as_v1[8:12] = struct.pack("<I", 1)
    refused(_resum(bytes(as_v1)))
