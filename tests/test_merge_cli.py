"""bin/sks-search merge: three genomes, each indexed as two one-record FASTA files
spread over two databases, merged by a groups file, equal a database indexed
from three two-record FASTA files (names: the group names); an unknown sketch
name is refused with the name and no file; and `query` runs on the result."""
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
def test_merge_then_query(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    w, k, c = 31, 21, 20
    parts, whole = {}, []
    for i, (seed, rate) in enumerate([(81, 0.0), (81, 0.02), (82, 0.0)]):
        g = synth.bases(30000 + 1000 * i, seed=seed, mut_seed=90 + i, mut_rate=rate)
        records = [(f"g{i}_a", g[:12000]), (f"g{i}_b", g[12000:])]
        for name, seq in records:
            p = tmp_path / f"{name}.fa"
            p.write_bytes(synth.fasta_text([(name, seq)], width=70))
            parts[name] = str(p)
        p = tmp_path / f"g{i}.fa"
        p.write_bytes(synth.fasta_text(records, width=70))
        whole.append(str(p))
    db1, db2, merged, direct = (str(tmp_path / n) for n in ("one.sks", "two.sks", "merged.sks", "direct.sks"))
    r = _run("index", db1, w, k, c, parts["g0_a"], parts["g0_b"], parts["g1_a"])
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run("index", db2, w, k, c, parts["g1_b"], parts["g2_a"], parts["g2_b"])
    assert r.returncode == 0, r.stdout + r.stderr
    # groups in order of first appearance: G1, G0, G2; G1's members lie in different databases
    lines = [("G1", "g1_a"), ("G0", "g0_a"), ("G1", "g1_b"), ("G2", "g2_b"), ("G0", "g0_b"), ("G2", "g2_a")]
    tsv = tmp_path / "groups.tsv"
    tsv.write_text("".join(f"{g}\t{parts[s]}\n" for g, s in lines))
    r = _run("merge", merged, tsv, db1, db2)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"3 sketches -> {merged}"
    r = _run("index", direct, w, k, c, whole[1], whole[0], whole[2])
    assert r.returncode == 0, r.stdout + r.stderr

    ctx = sksffi.Context(0)
    M, D = ctx.load_sketches(merged), ctx.load_sketches(direct)
    assert M.names() == ["G1", "G0", "G2"]
    info_m, info_d = M.info(), D.info()
    assert info_m == info_d and info_m["param"] == c and info_m["n"] == 3
    assert np.array_equal(M.sizes(), D.sizes()) and np.array_equal(M.windows(), D.windows())
    assert M.sizes().min() > 0
    for i in range(3):
        assert np.array_equal(M.sketch(i), D.sketch(i)), i

    # a sketch name no input holds: refused with the name, and no output file
    bad = tmp_path / "x.sks"
    tsv_bad = tmp_path / "bad.tsv"
    tsv_bad.write_text(f"G0\t{parts['g0_a']}\nG0\tno_such_sketch\n")
    r = _run("merge", bad, tsv_bad, db1, db2)
    assert r.returncode != 0
    assert "no_such_sketch" in r.stderr
    assert not bad.exists()
    # a sketch name found in two inputs
    r = _run("merge", bad, tsv, db1, db1)
    assert r.returncode != 0 and "twice" in r.stderr and not bad.exists()
    # the usage line names the mode
    r = _run("merge", merged)
    assert r.returncode == 64 and "merge <out.sks> <groups.tsv> <in.sks> [<in.sks> ...]" in r.stderr

    # query against the merged database: the rows Context.search gives on the same sketches
    q_files = [whole[0], whole[2]]
    streams = [sksffi.Fasta(f).stream() for f in q_files]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
    dev = torch.from_numpy(np.concatenate(streams)).to("cuda:0")
    Q = ctx.sketch_build(dev.data_ptr(), int(offs[-1]), offs, w, info_m["mask"], info_m["kind"], info_m["param"],
                         nonce=info_m["nonce"], flavour=info_m["flavour"])
    want = ctx.search(Q, M)
    assert len(want) >= 3
    out = tmp_path / "hits.csv"
    r = _run("query", merged, "0", out, *q_files)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split(",") for ln in out.read_text().splitlines()[1:]]
    assert len(rows) == len(want)
    names = M.names()
    for row, h in zip(rows, want):
        assert row[0] == q_files[h["query"]] and row[1] == names[h["ref"]]
        assert int(row[2]) == h["shared"]
        assert float(row[3]) == h["containment"] and float(row[4]) == h["ani"]
    ctx.close()
