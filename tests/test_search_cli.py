"""bin/sks-search: `index` three FASTA files into a sketch database, `query`
them plus an unrelated file; the CSV must hold exactly the rows Context.search
gives on the same sketches, doubles surviving their %.17g text form."""
import os
import subprocess

import numpy as np
import pytest

import sksffi
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spaced-kmer-sketching_amd", "bin", "sks-search")


@pytest.mark.gpu
def test_index_then_query(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    w, k, c = 31, 21, 50
    files = []
    for i, (seed, rate) in enumerate([(51, 0.0), (51, 0.01), (51, 0.04), (52, 0.0)]):
        g = synth.bases(30000 + 1000 * i, seed=seed, mut_seed=90 + i, mut_rate=rate)
        p = tmp_path / f"g{i}.fa"
        p.write_bytes(synth.fasta_text([(f"g{i}_a", g[:12000]), (f"g{i}_b", g[12000:])], width=70))
        files.append(str(p))
    db_files, unrelated = files[:3], files[3]
    db = str(tmp_path / "db.sks")
    r = subprocess.run([BIN, "index", db, str(w), str(k), str(c)] + db_files, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr

    ctx = sksffi.Context(0)
    R = ctx.load_sketches(db)
    info = R.info()
    assert R.names() == db_files
    assert (info["window"], info["mask"], info["kind"], info["param"]) == \
        (w, sksffi.mask_generate(w, k, 0), sksffi.SKS_FRAC_MOD, c)
    # the queries, sketched here the way the tool does: one segment per file's record stream
    q_files = db_files + [unrelated]
    streams = [sksffi.Fasta(f).stream() for f in q_files]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
    dev = torch.from_numpy(np.concatenate(streams)).to("cuda:0")
    Q = ctx.sketch_build(dev.data_ptr(), int(offs[-1]), offs, w, info["mask"], info["kind"], info["param"],
                         nonce=info["nonce"], flavour=info["flavour"])
    every = ctx.search(Q, R)
    conts = np.unique(every["containment"])
    assert len(conts) >= 3
    thr = float((conts[0] + conts[1]) / 2)  # rejects the most distant sharing pair only
    assert np.abs(every["containment"] - thr).min() > 1e-9
    want = ctx.search(Q, R, min_containment=thr)
    assert 0 < len(want) < len(every)

    out = tmp_path / "hits.csv"
    r = subprocess.run([BIN, "query", db, repr(thr), str(out)] + q_files, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = out.read_text().splitlines()
    assert lines[0] == "Query,Reference,Shared,Containment,ANI"
    rows = [ln.split(",") for ln in lines[1:]]
    assert len(rows) == len(want)
    for row, h in zip(rows, want):
        assert row[0] == q_files[h["query"]] and row[1] == db_files[h["ref"]]
        assert int(row[2]) == h["shared"]
        assert float(row[3]) == h["containment"] and float(row[4]) == h["ani"]
    assert unrelated not in [row[0] for row in rows]
    assert {row[0] for row in rows} == set(db_files)
    ctx.close()
