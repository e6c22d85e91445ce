"""bin/sks-search downsample: a database indexed at 1/20, downsampled to 1/100 by
the tool, equals a database indexed at 1/100 directly (names kept); a parameter
that is no multiple is refused with the library's message and no file; and
`query` runs on the downsampled database."""
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


@pytest.mark.gpu
def test_downsample_then_query(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    w, k = 31, 21
    files = []
    for i, (seed, rate) in enumerate([(61, 0.0), (61, 0.01), (61, 0.04), (62, 0.0)]):
        g = synth.bases(30000 + 1000 * i, seed=seed, mut_seed=70 + i, mut_rate=rate)
        p = tmp_path / f"g{i}.fa"
        p.write_bytes(synth.fasta_text([(f"g{i}_a", g[:12000]), (f"g{i}_b", g[12000:])], width=70))
        files.append(str(p))
    db_files, unrelated = files[:3], files[3]
    db, small, direct = (str(tmp_path / n) for n in ("db.sks", "small.sks", "direct.sks"))
    r = _run("index", db, w, k, 20, *db_files)
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run("downsample", db, 100, small)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"3 sketches -> {small}"
    r = _run("index", direct, w, k, 100, *db_files)
    assert r.returncode == 0, r.stdout + r.stderr

    ctx = sksffi.Context(0)
    S, D, full = ctx.load_sketches(small), ctx.load_sketches(direct), ctx.load_sketches(db)
    assert S.names() == db_files
    assert S.info()["param"] == 100 and S.info() == D.info()
    assert np.array_equal(S.sizes(), D.sizes()) and np.array_equal(S.windows(), D.windows())
    assert 0 < S.sizes().sum() < full.sizes().sum()
    for i in range(3):
        assert np.array_equal(S.sketch(i), D.sketch(i)), i

    # 30 is no multiple of 20: the library's refusal, and no output file
    bad = tmp_path / "x.sks"
    r = _run("downsample", db, 30, bad)
    assert r.returncode != 0
    assert "policy param" in r.stderr
    assert not bad.exists()
    # the usage line names the mode
    r = _run("downsample", db)
    assert r.returncode == 64 and "downsample <in.sks> <c> <out.sks>" in r.stderr

    # query against the downsampled database: the rows Context.search gives on the same sketches
    q_files = db_files + [unrelated]
    streams = [sksffi.Fasta(f).stream() for f in q_files]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
    dev = torch.from_numpy(np.concatenate(streams)).to("cuda:0")
    info = S.info()
    Q = ctx.sketch_build(dev.data_ptr(), int(offs[-1]), offs, w, info["mask"], info["kind"], info["param"],
                         nonce=info["nonce"], flavour=info["flavour"])
    want = ctx.search(Q, S)
    assert len(want) >= 3
    out = tmp_path / "hits.csv"
    r = _run("query", small, "0", out, *q_files)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = out.read_text().splitlines()
    assert lines[0] == "Query,Reference,Shared,Containment,ANI"
    rows = [ln.split(",") for ln in lines[1:]]
    assert len(rows) == len(want)
    for row, h in zip(rows, want):
        assert row[0] == q_files[h["query"]] and row[1] == db_files[h["ref"]]
        assert int(row[2]) == h["shared"]
        assert float(row[3]) == h["containment"] and float(row[4]) == h["ani"]
    ctx.close()
