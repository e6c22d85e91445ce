"""Host reference of sks_gather shared by the gather tests: a greedy loop over
Python sets of the sketches' elements.  Each round picks the reference with the
most still unexplained query elements, ties to the smallest index, reports it
while that count is at least max(min_shared, 1) and fewer than max_rounds rounds
were reported, and removes its elements from the query.  Every value is an
integer or one float64 division of integers; the ANI is the library's host
function (sksffi.ani_from_counts)."""
import numpy as np

import sksffi


def as_set(keys):
    """A sketch (cluster_ref.keys_of form, or any 1-D array / (n, 2) array) as a Python set."""
    a = np.asarray(keys)
    if a.dtype.names:
        return set(zip(a["hi"].tolist(), a["lo"].tolist()))
    if a.ndim == 2:
        return set(zip(a[:, 1].tolist(), a[:, 0].tolist()))
    return set(a.tolist())


def greedy(query, refs, k, min_shared=1, max_rounds=0):
    """(hits as a GATHER_HIT_DTYPE array in round order, n_unexplained, info);
    info counts the candidates, the rounds whose winner tied on `new` with a
    larger index, and the rounds with shared_new < shared."""
    thr = max(int(min_shared), 1)
    Q = set(query)
    R = [set(r) for r in refs]
    shared = [len(Q & r) for r in R]
    rem = set(Q)
    rows, ties, partial = [], 0, 0
    live = [i for i in range(len(R)) if shared[i] >= thr]
    n_cand = len(live)
    while True:
        new = {i: len(rem & R[i]) for i in live}
        if not new:
            break
        best = max(new.values())
        if best < thr or (max_rounds and len(rows) >= max_rounds):
            break
        winners = [i for i in live if new[i] == best]
        r = winners[0]  # live is ascending: the smallest index
        ties += len(winners) > 1
        partial += best < shared[r]
        rows.append((r, shared[r], best, len(R[r])))
        rem -= R[r]
        live = [i for i in live if i != r and new[i] >= thr]  # counts never grow
    out = np.zeros(len(rows), dtype=sksffi.GATHER_HIT_DTYPE)
    if rows:
        a = np.array(rows, dtype=np.int64)
        out["ref"], out["shared"], out["shared_new"], out["ref_size"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
        out["f_query_new"] = a[:, 2].astype(np.float64) / np.float64(len(Q))
        out["ani"] = sksffi.ani_from_counts(a[:, 1], a[:, 3], k)[1]
    return out, len(rem), {"candidates": n_cand, "ties": ties, "partial": partial}
