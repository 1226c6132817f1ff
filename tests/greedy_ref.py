"""Reference of the greedy representatives (include/dashing_hip.h, dsh_greedy_threshold*): priority is slot order; x is a
representative iff no earlier representative hits it, and every other slot is labelled with the SMALLEST representative
that hits it.  Two independent statements of that, held to each other by tests/test_greedy_ref.py; nothing here is shared
with the code under test.  Plain helper module, importable without a device."""
import numpy as np


def labels(n, row_ptr, col):
    """(labels uint32 [n], n_reps): the sequential pass over a CSR as dist_threshold returns it for rows [0, n) -- hit h of
    row i (row_ptr[i] <= h < row_ptr[i + 1]) is the pair (i, col[h]) with col[h] > i.  Row i is a representative iff no
    earlier row has claimed it; a representative claims its columns that nobody has claimed yet (rows ascend: the first to
    claim is the smallest)."""
    n = int(n)
    rp = np.asarray(row_ptr, np.int64).reshape(-1)
    cl = np.asarray(col, np.int64).reshape(-1)
    assert rp.size == n + 1 or (n == 0 and rp.size <= 1)
    lab = list(range(n))
    for i in range(n):
        if lab[i] != i:
            continue
        for j in cl[rp[i] : rp[i + 1]].tolist():
            assert i < j < n
            if lab[j] == j:
                lab[j] = i
    out = np.array(lab, np.uint32).reshape(n)
    return out, int((out == np.arange(n, dtype=np.uint32)).sum())


def labels_from_definition(n, hit_matrix):
    """the same for small n, from the definition: hit_matrix is a dense boolean [n, n] of which only the entries (i, j),
    i < j, are read.  R by the recursion (x in R iff no r in R, r < x, hits x), then every label as the minimum over the
    representative neighbours."""
    n = int(n)
    h = np.asarray(hit_matrix, bool).reshape(n, n)
    rep = np.zeros(n, bool)
    for x in range(n):
        rep[x] = not (rep[:x] & h[:x, x]).any()
    out = np.arange(n, dtype=np.uint32)
    for x in range(n):
        if not rep[x]:
            out[x] = np.flatnonzero(rep[:x] & h[:x, x]).min()
    return out, int(rep.sum())


def csr_of_edges(n, lhs, rhs):
    """(row_ptr, col) of the graph with the edges (lhs[e], rhs[e]) normalised to i < j, self loops dropped, repeated edges
    kept once, columns ascending: the form dist_threshold gives"""
    a = np.asarray(lhs, np.int64).reshape(-1)
    b = np.asarray(rhs, np.int64).reshape(-1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    keep = lo != hi
    code = np.unique(lo[keep] * max(int(n), 1) + hi[keep])
    lo, hi = code // max(int(n), 1), code % max(int(n), 1)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(lo, minlength=int(n)))]).astype(np.uint64)
    return row_ptr, hi.astype(np.uint32)


def hit_matrix(n, row_ptr, col):
    h = np.zeros((int(n), int(n)), bool)
    rp = np.asarray(row_ptr, np.int64)
    rows = np.repeat(np.arange(int(n)), np.diff(rp))
    h[rows, np.asarray(col, np.int64)] = True
    return h
