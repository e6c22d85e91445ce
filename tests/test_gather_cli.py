"""bin/sks-search gather: `index` ten FASTA files into a sketch database, `gather`
one mixture file against it; the CSV must hold exactly the rows Context.gather
gives on the same sketches, doubles surviving their %.17g text form, then the
query's `unexplained` line.  Bad usage exits with status 64."""
import os
import subprocess

import numpy as np
import pytest

import sksffi
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spaced-kmer-sketching_amd", "bin", "sks-search")


@pytest.mark.gpu
def test_index_then_gather(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    w, k, c = 31, 21, 50
    # five ancestors, each with a 2 % descendant
    genomes = [synth.bases(30000 + 500 * i, seed=61 + i // 2, mut_seed=80 + i, mut_rate=0.02 * (i % 2))
               for i in range(10)]
    db_files = []
    for i, g in enumerate(genomes):
        p = tmp_path / f"g{i}.fa"
        p.write_bytes(synth.fasta_text([(f"g{i}", g)], width=70))
        db_files.append(str(p))
    # the mixture: an ancestor, a descendant of another, a fresh descendant of a third, and noise
    mix = tmp_path / "mix.fa"
    mix.write_bytes(synth.fasta_text([("a", genomes[0]), ("b", genomes[3]),
                                      ("c", synth.bases(31000, seed=63, mut_seed=99, mut_rate=0.01)),
                                      ("noise", synth.bases(20000, seed=77))], width=70))
    db = str(tmp_path / "db.sks")
    r = subprocess.run([BIN, "index", db, str(w), str(k), str(c)] + db_files, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr

    ctx = sksffi.Context(0)
    R = ctx.load_sketches(db)
    info = R.info()
    assert R.names() == db_files
    # the query, sketched here the way the tool does: one segment per file's record stream
    stream = sksffi.Fasta(str(mix)).stream()
    dev = torch.from_numpy(np.asarray(stream)).to("cuda:0")
    Q = ctx.sketch_build(dev.data_ptr(), len(stream), [0, len(stream)], w, info["mask"], info["kind"], info["param"],
                         nonce=info["nonce"], flavour=info["flavour"])
    want, unexplained = ctx.gather(Q, 0, R, min_shared=3)
    assert len(want) >= 3 and unexplained > 0

    out = tmp_path / "gather.csv"
    r = subprocess.run([BIN, "gather", db, "3", str(out), str(mix)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = out.read_text().splitlines()
    assert lines[0] == "Query,Round,Reference,Shared,SharedNew,RefSize,FQueryNew,ANI"
    rows = [ln.split(",") for ln in lines[1:-1]]
    assert len(rows) == len(want)
    for i, (row, h) in enumerate(zip(rows, want)):
        assert row[0] == str(mix) and int(row[1]) == i and row[2] == db_files[h["ref"]]
        assert (int(row[3]), int(row[4]), int(row[5])) == (h["shared"], h["shared_new"], h["ref_size"])
        assert float(row[6]) == h["f_query_new"] and float(row[7]) == h["ani"]
    assert lines[-1] == f"{mix},-,unexplained,{unexplained},,,,"
    ctx.close()

    # bad usage: too few arguments, an unknown mode
    for args in (["gather", db, "3", str(out)], ["gather"], ["collect", db, "3", str(out), str(mix)]):
        r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 64, args
        assert "gather <db.sks> <min_shared> <out.csv>" in r.stderr
