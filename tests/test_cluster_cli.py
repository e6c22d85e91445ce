"""bin/sks-search cluster: nine genomes (three families: an ancestor and
descendants at 1% and 2% substitutions) indexed from FASTA files, clustered at
the midpoint of the widest gap between their pairwise containments.  The TSV
and the summary line equal what the host reference (tests/cluster_ref.py) gives
on the database's sketches; the representatives database holds each
representative's sketch to the element, with its windows and name, and `query`
runs on it; a bad threshold is refused with a message and no file."""
import os
import subprocess

import numpy as np
import pytest

import cluster_ref as R
import sksffi
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spaced-kmer-sketching_amd", "bin", "sks-search")


def _run(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.gpu
def test_cluster_then_query(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    w, k, c = 31, 21, 50
    files = []
    for i in range(9):  # genome i: family i % 3; the ancestors come first, the longest genomes last
        fam, gen = i % 3, i // 3
        g = synth.bases(24000 + 3000 * i, seed=60 + fam, mut_seed=600 + i, mut_rate=[0.0, 0.01, 0.02][gen])
        p = tmp_path / f"g{i}.fa"
        p.write_bytes(synth.fasta_text([(f"g{i}", g)], width=70))
        files.append(str(p))
    db, tsv, reps_db = (str(tmp_path / n) for n in ("db.sks", "clusters.tsv", "reps.sks"))
    r = _run("index", db, w, k, c, *files)
    assert r.returncode == 0, r.stdout + r.stderr

    ctx = sksffi.Context(0)
    D = ctx.load_sketches(db)
    sizes = D.sizes().astype(np.int64)
    shared = R.shared_matrix(R.keys_of(D))
    thr = R.threshold(shared, sizes)
    labels, reps = R.components(R.links(shared, sizes, thr), sizes)
    assert 1 < len(reps) < 9 and (reps != np.array([np.nonzero(labels == c_)[0][0] for c_ in range(len(reps))])).any()

    r = _run("cluster", db, repr(thr), tsv, reps_db)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"9 sketches, {len(reps)} clusters -> {tsv}"
    want = "".join(f"{labels[i]}\t{files[reps[labels[i]]]}\t{files[i]}\n" for i in range(9))
    with open(tsv) as f:
        assert f.read() == want

    # the representatives, in cluster order: the source's sketches with their windows and names
    P = ctx.load_sketches(reps_db)
    assert P.n == len(reps) and P.names() == [files[x] for x in reps]
    info_p, info_d = P.info(), D.info()
    assert {**info_p, "n": 0} == {**info_d, "n": 0}
    assert np.array_equal(P.sizes(), D.sizes()[reps]) and np.array_equal(P.windows(), D.windows()[reps])
    for c_, x in enumerate(reps):
        assert np.array_equal(P.sketch(c_), D.sketch(int(x))), c_
    ctx.close()

    # without the fourth argument: the same TSV, no database
    tsv2 = str(tmp_path / "again.tsv")
    r = _run("cluster", db, repr(thr), tsv2)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(tsv2) as f:
        assert f.read() == want

    # a member that is not its cluster's representative finds the representative
    member = next(i for i in range(9) if reps[labels[i]] != i)
    out = tmp_path / "hits.csv"
    r = _run("query", reps_db, "0", out, files[member])
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split(",") for ln in out.read_text().splitlines()[1:]]
    assert [files[member], files[reps[labels[member]]]] in [row[:2] for row in rows]

    # a bad threshold: exit 1 with a message, no file; the usage line names the mode
    bad = tmp_path / "bad.tsv"
    r = _run("cluster", db, "0.5x", bad)
    assert r.returncode == 1 and "bad min_containment: 0.5x" in r.stderr and not bad.exists()
    r = _run("cluster", db)
    assert r.returncode == 64 and "cluster <db.sks> <min_containment> <out.tsv> [<reps.sks>]" in r.stderr
