"""bin/sks-search: `index` three FASTA files into a sketch database, `top` with
k = 2 on them plus an unrelated file; the CSV must hold exactly the filled slots
Context.search_topk gives on the same sketches, doubles surviving their %.17g
text form, and no row for the unrelated file."""
import os
import subprocess

import numpy as np
import pytest

import sksffi
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spaced-kmer-sketching_amd", "bin", "sks-search")


@pytest.mark.gpu
def test_index_then_top(tmp_path):
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
    # the queries, sketched here the way the tool does: one segment per file's record stream
    q_files = db_files + [unrelated]
    streams = [sksffi.Fasta(f).stream() for f in q_files]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
    dev = torch.from_numpy(np.concatenate(streams)).to("cuda:0")
    Q = ctx.sketch_build(dev.data_ptr(), int(offs[-1]), offs, w, info["mask"], info["kind"], info["param"],
                         nonce=info["nonce"], flavour=info["flavour"])
    hits, counts = ctx.search_topk(Q, R, 2)
    assert counts.tolist() == [2, 2, 2, 0]  # three related references, two slots; nothing for the unrelated file
    want = [h for q in range(4) for h in hits[q, :counts[q]]]

    out = tmp_path / "top.csv"
    r = subprocess.run([BIN, "top", db, "2", str(out)] + q_files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = out.read_text().splitlines()
    assert lines[0] == "Query,Rank,Reference,Shared,Score,ANI"
    rows = [ln.split(",") for ln in lines[1:]]
    assert len(rows) == len(want) == 6
    for row, h in zip(rows, want):
        assert row[0] == q_files[h["query"]] and int(row[1]) == h["rank"] and row[2] == db_files[h["ref"]]
        assert int(row[3]) == h["shared"]
        assert float(row[4]) == h["score"] and float(row[5]) == h["ani"]
    assert [int(row[1]) for row in rows] == [0, 1] * 3
    assert rows[0][2] == db_files[0] and float(rows[0][4]) == 1.0  # a file's best reference is itself
    assert unrelated not in [row[0] for row in rows]
    # k outside 1 .. 64 is refused before anything runs
    for bad in ("65",):
        r = subprocess.run([BIN, "top", db, bad, str(out)] + q_files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "bad k" in r.stderr
    ctx.close()
