"""bin/sks-search subtract / intersect: a database filtered by the tool against
the union of a second database's sketches equals Context.filter with the merged
filter (names kept); a filter database of another scale is refused with the
library's message and no file."""
import os
import subprocess

import numpy as np
import pytest

import sksffi
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spaced-kmer-sketching_amd", "bin", "sks-search")


def _run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _fasta(tmp_path, name, seed, mut_seed, rate, n=30000):
    g = synth.bases(n, seed=seed, mut_seed=mut_seed, mut_rate=rate)
    p = tmp_path / f"{name}.fa"
    p.write_bytes(synth.fasta_text([(f"{name}_a", g[:12000]), (f"{name}_b", g[12000:])], width=70))
    return str(p)


@pytest.mark.gpu
def test_subtract_and_intersect(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    w, k = 31, 21
    samples = [_fasta(tmp_path, f"s{i}", seed, 80 + i, rate)
               for i, (seed, rate) in enumerate([(61, 0.0), (62, 0.02), (63, 0.0)])]
    hosts = [_fasta(tmp_path, f"h{i}", seed, 90 + i, rate) for i, (seed, rate) in enumerate([(61, 0.01), (62, 0.0)])]
    db, host, coarse = (str(tmp_path / n) for n in ("db.sks", "host.sks", "coarse.sks"))
    for out, c, files in ((db, 20, samples), (host, 20, hosts), (coarse, 40, hosts)):
        r = _run("index", out, w, k, c, *files)
        assert r.returncode == 0, r.stdout + r.stderr

    ctx = sksffi.Context(0)
    D, H = ctx.load_sketches(db), ctx.load_sketches(host)
    united = ctx.merge([H], [list(range(H.n))])
    total = int(D.sizes().sum())
    kept = {}
    for mode, kind in (("subtract", sksffi.SKS_FILTER_SUBTRACT), ("intersect", sksffi.SKS_FILTER_INTERSECT)):
        out = str(tmp_path / f"{mode}.sks")
        r = _run(mode, db, host, out)
        assert r.returncode == 0, r.stdout + r.stderr
        want = ctx.filter(D, united, kind)
        kept[mode] = int(want.sizes().sum())
        assert r.stdout.strip() == f"3 sketches, {kept[mode]} elements -> {out}"
        got = ctx.load_sketches(out)
        assert got.names() == samples and got.info() == D.info()
        assert np.array_equal(got.sizes(), want.sizes()) and np.array_equal(got.windows(), D.windows())
        for i in range(3):
            assert np.array_equal(got.sketch(i), want.sketch(i)), i
    assert 0 < kept["intersect"] < total and kept["subtract"] + kept["intersect"] == total
    # sample 2 shares nothing with the hosts
    assert ctx.load_sketches(str(tmp_path / "intersect.sks")).sizes()[2] == 0

    # a filter database of another scale: the library's refusal, and no output file
    for mode in ("subtract", "intersect"):
        bad = tmp_path / f"bad_{mode}.sks"
        r = _run(mode, db, coarse, bad)
        assert r.returncode != 0
        assert "policy param" in r.stderr
        assert not bad.exists()
        # the usage line names the mode
        r = _run(mode, db)
        assert r.returncode == 64 and f"{mode} <db.sks> <filter.sks> <out.sks>" in r.stderr
    ctx.close()
