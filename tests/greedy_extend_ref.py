"""Reference of dsh_greedy_extend* (include/dashing_hip.h): the greedy representatives continued behind a labelling of the
slots [0, m), with the covered slots given to the FIRST or to the BEST representative that hits them.  Two independent
statements, held to each other by tests/test_greedy_extend_ref.py; nothing here is shared with the code under test.
Values are compared as numpy float32 scalars: -0.0 equals +0.0 and a NaN is no hit.  Plain helper module, importable without
a device."""
import numpy as np

FIRST, BEST = 0, 1


def labels(n, row_ptr, col, val, first_new=0, labels_in=None, mode=FIRST, similarity=True):
    """(labels uint32 [n], n_reps): the sequential pass over a CSR with values as dist_threshold returns it for rows [0, n)
    -- hit h of row i is the pair (i, col[h]), col[h] > i, with the value val[h].  Old slots keep labels_in.  Rows ascend:
    a row that is a representative claims its unclaimed NEW columns; in BEST it also takes over a claimed new column where
    its value is STRICTLY better than what the column holds (so among equal values the smallest row stays)."""
    n, m = int(n), int(first_new)
    rp = np.asarray(row_ptr, np.int64).reshape(-1)
    cl = np.asarray(col, np.int64).reshape(-1)
    vl = np.asarray(val, np.float32).reshape(-1)
    assert rp.size == n + 1 or (n == 0 and rp.size <= 1)
    assert 0 <= m <= n and (m == 0 or len(labels_in) == m)
    lab = [int(x) for x in (labels_in if m else [])] + list(range(m, n))
    held = [None] * n  # the value a covered new slot holds
    for i in range(n):
        if lab[i] != i:
            continue
        for h in range(int(rp[i]), int(rp[i + 1])):
            j, v = int(cl[h]), vl[h]
            assert i < j < n
            if j < m:
                continue  # old slots are never re-judged
            if held[j] is None:
                assert lab[j] == j
                lab[j], held[j] = i, v
            elif mode == BEST and (v > held[j] if similarity else v < held[j]):
                lab[j], held[j] = i, v
    out = np.array(lab, np.uint32).reshape(n)
    return out, int((out == np.arange(n, dtype=np.uint32)).sum())


def labels_fast(n, row_ptr, col, val, first_new=0, labels_in=None, mode=FIRST, similarity=True):
    """labels() with one numpy step per representative row (the GPU tests walk millions of hits); held to labels() by
    tests/test_greedy_extend_ref.py"""
    n, m = int(n), int(first_new)
    rp = np.asarray(row_ptr, np.int64).reshape(-1)
    cl = np.asarray(col, np.int64).reshape(-1)
    vl = np.asarray(val, np.float32).reshape(-1)
    lab = np.arange(n, dtype=np.int64)
    if m:
        lab[:m] = np.asarray(labels_in, np.int64)
    covered = np.zeros(n, bool)
    held = np.zeros(n, np.float32)
    for i in range(n):
        if lab[i] != i or rp[i] == rp[i + 1]:
            continue
        j, v = cl[rp[i] : rp[i + 1]], vl[rp[i] : rp[i + 1]]  # (the columns of a row are distinct)
        take = ~covered[j]
        if mode == BEST:
            take |= (v > held[j]) if similarity else (v < held[j])
        take &= j >= m
        j, v = j[take], v[take]
        lab[j], held[j], covered[j] = i, v, True
    out = lab.astype(np.uint32)
    return out, int((out == np.arange(n, dtype=np.uint32)).sum())


def labels_from_definition(n, values, threshold, first_new=0, labels_in=None, mode=FIRST, similarity=True):
    """the same for small n, from the definition: values is a dense float32 [n, n] of which only the entries (i, j), i < j,
    are read.  R_old as given, R by the recursion, then every new label as the minimum (FIRST) or as the smallest of the
    best-valued (BEST) over the representative neighbours."""
    n, m = int(n), int(first_new)
    v = np.asarray(values, np.float32).reshape(n, n)
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        h = (v >= t) if similarity else (v <= t)
    out = np.arange(n, dtype=np.uint32)
    if m:
        out[:m] = np.asarray(labels_in, np.uint32)
    rep = np.zeros(n, bool)
    rep[:m] = out[:m] == np.arange(m)
    for x in range(m, n):
        rep[x] = not (rep[:x] & h[:x, x]).any()
    for x in range(m, n):
        if rep[x]:
            continue
        cand = np.flatnonzero(rep[:x] & h[:x, x])
        if mode == BEST:
            vals = v[cand, x]
            top = vals.max() if similarity else vals.min()
            cand = cand[vals == top]
        out[x] = cand.min()
    return out, int((out == np.arange(n, dtype=np.uint32)).sum())


def csr_of_values(n, values, threshold, similarity=True):
    """(row_ptr, col, val) of the pairs i < j of a dense float32 [n, n] that pass: the form dist_threshold gives"""
    n = int(n)
    v = np.asarray(values, np.float32).reshape(n, n)
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        h = np.triu((v >= t) if similarity else (v <= t), 1)
    rows, cols = np.nonzero(h)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.uint64)
    return row_ptr, cols.astype(np.uint32), v[rows, cols]


def dense_of_csr(n, row_ptr, col, val, fill):
    """dense float32 [n, n] with the hits' values at (i, j), i < j, and `fill` (a value that does not pass) elsewhere"""
    n = int(n)
    v = np.full((n, n), fill, np.float32)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(row_ptr, np.int64)))
    v[rows, np.asarray(col, np.int64)] = np.asarray(val, np.float32)
    return v


def random_labelling(m, rng, p_rep=0.4):
    """an arbitrary VALID labelling of m slots: labels[x] <= x and labels[labels[x]] == labels[x]"""
    lab = np.arange(m, dtype=np.uint32)
    reps = []
    for x in range(m):
        if reps and rng.random() >= p_rep:
            lab[x] = reps[int(rng.integers(len(reps)))]
        else:
            reps.append(x)
    return lab


def check_consequences(n, values, threshold, first_new, labels_in, lab, mode, similarity, what=""):
    """what the header promises of a result, read off the dense values"""
    n, m = int(n), int(first_new)
    v = np.asarray(values, np.float32).reshape(n, n)
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        h = (v >= t) if similarity else (v <= t)
    l = np.asarray(lab, np.int64)
    x = np.arange(n)
    assert (l <= x).all() and (l[l] == l).all(), what
    if m:
        assert np.array_equal(l[:m], np.asarray(labels_in, np.int64)), what
    reps = np.flatnonzero(l == x)
    new_reps = reps[reps >= m]
    assert not np.triu(h, 1)[np.ix_(reps, new_reps)].any(), what  # no representative hits a NEW representative
    for c in np.flatnonzero((l != x) & (x >= m)).tolist():
        r = l[c]
        assert r < c and h[r, c], (what, c)
        others = reps[(reps < c) & h[reps, c]]
        if mode == BEST:
            strictly = v[others, c] > v[r, c] if similarity else v[others, c] < v[r, c]
            assert not strictly.any(), (what, c)
            assert r == others[v[others, c] == v[r, c]].min(), (what, c)
        else:
            assert r == others.min(), (what, c)
