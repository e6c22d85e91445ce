"""The input of tools/bench_topk.py (1000 x 5 Mb, FracMinHash 1/200), 5 sks_search_sets size
queries of the set against itself, then 6 sks_search_topk_sets calls (k = 10, SKS_RANK_QUERY,
skip_same_index), each followed by a synchronise and a 2 ms pause so that a kernel trace shows the
calls apart:
    bash tools/gpu/run.sh trace topk_trace tools/trace_topk.py
profiles/topk/timeline.txt is the per-kernel timeline of the last call of each kind from such a trace."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spaced-kmer-sketching_amd"))
import sksffi  # noqa: E402

n, length, c, k = 1000, 5_000_000, 200, 10
ctx = sksffi.Context(0)
mask = sksffi.mask_generate(31, 21, 0)
seg = [0]
for _ in range(n):
    seg.append(seg[-1] + length + 1)
buf = torch.full((seg[-1],), ord("\n"), dtype=torch.uint8, device="cuda")
for g in range(n):
    fam, member = divmod(g, 8)
    ctx.synth_bases(buf.data_ptr() + seg[g], length, 4000 + fam, 9000 + g, 0.005 * member)
torch.cuda.synchronize()
refs = ctx.sketch_build(buf.data_ptr(), seg[-1], seg, 31, mask, sksffi.SKS_FRAC_MOD, c)
ctx.synchronize()
d_hits = torch.zeros(n * k * 40, dtype=torch.uint8, device="cuda")
d_counts = torch.zeros(n, dtype=torch.int32, device="cuda")
for _ in range(5):
    ctx.search_sets_raw(refs, refs, 0.0, 1, 0, 0)
    torch.cuda.synchronize()
    time.sleep(0.002)
for _ in range(6):
    sksffi.check(ctx.search_topk_sets_raw(refs, refs, sksffi.SKS_RANK_QUERY, k, 0.0, 1, True,
                                          d_hits.data_ptr(), d_counts.data_ptr()))
    torch.cuda.synchronize()
    time.sleep(0.002)
print("done", int(d_counts.sum()))
