"""Host reference of sks_cluster shared by the cluster tests: the shared-element
matrix of a set's sketches (np.intersect1d), the link rule in float64, a plain
union-find, clusters numbered by ascending smallest member and representatives
by (size, -index); and the threshold the tests cluster at."""
import numpy as np


def keys_of(ss):
    """Each sketch of the set as a 1-D array intersect1d can compare."""
    out = []
    for i in range(ss.n):
        a = np.ascontiguousarray(ss.sketch(i))
        out.append(a[:, 0].copy() if ss.elem_words == 1
                   else a.view([("lo", "<u8"), ("hi", "<u8")]).ravel())
    return out


def shared_matrix(keys):
    n = len(keys)
    m = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        for j in range(i + 1, n):
            if len(keys[i]) and len(keys[j]):
                m[i, j] = m[j, i] = len(np.intersect1d(keys[i], keys[j], assume_unique=True))
    return m


def threshold(shared, sizes):
    """Midpoint of the widest gap between adjacent distinct values of
    shared / min(size_i, size_j) over the sharing pairs; none within 1e-9."""
    i, j = np.nonzero(np.triu(shared, 1))
    val = shared[i, j].astype(np.float64) / np.minimum(sizes[i], sizes[j]).astype(np.float64)
    u = np.unique(val)
    assert len(u) >= 2
    g = int(np.argmax(np.diff(u)))
    thr = (u[g] + u[g + 1]) / 2
    assert np.abs(val - thr).min() > 1e-9
    assert (val >= thr).any() and (val < thr).any()
    return float(thr)


def links(shared, sizes, min_containment=0.0, min_shared=1):
    """The link rule in float64: both containments of every pair."""
    sz = np.maximum(sizes, 1).astype(np.float64)
    sh = shared.astype(np.float64)
    ci, cj = sh / sz[:, None], sh / sz[None, :]
    ok = (shared >= max(min_shared, 1)) & (np.maximum(ci, cj) >= min_containment)
    np.fill_diagonal(ok, False)
    return ok


def components(link, sizes):
    """(labels, reps) of the graph `link`: a plain union-find, clusters numbered
    by ascending smallest member, the representative by (size, -index)."""
    n = len(sizes)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in zip(*np.nonzero(np.triu(link, 1))):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    roots = [find(i) for i in range(n)]
    ids = {}
    for r in roots:  # ascending i: a root is first met at its smallest member
        ids.setdefault(r, len(ids))
    labels = np.array([ids[r] for r in roots], dtype=np.uint32)
    reps = np.zeros(len(ids), dtype=np.uint32)
    for c in range(len(ids)):
        members = np.nonzero(labels == c)[0]
        reps[c] = max(members, key=lambda m: (int(sizes[m]), -int(m)))
    return labels, reps
