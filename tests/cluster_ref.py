"""numpy reference of the threshold clusters (include/dashing_hip.h, dsh_cluster_*): the connected components of a graph
on the nodes 0..n-1, every node labelled with the SMALLEST node of its component.  A plain sequential union-find (union by
smaller root, path halving); nothing here is shared with the code under test.  Plain helper module, importable without a
device."""
import numpy as np


def labels(n, lhs, rhs, labels_in=None):
    """(labels uint32 [n], n_clusters) of the graph with the edges (lhs[e], rhs[e]); labels_in: x starts united with
    labels_in[x].  Self loops and repeated edges are legal."""
    n = int(n)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    if labels_in is not None:
        for x, l in enumerate(np.asarray(labels_in).reshape(-1).tolist()):
            unite(x, l)
    for a, b in zip(np.asarray(lhs).reshape(-1).tolist(), np.asarray(rhs).reshape(-1).tolist()):
        assert 0 <= a < n and 0 <= b < n
        unite(a, b)
    out = np.array([find(x) for x in range(n)], np.uint32).reshape(n)
    return out, int((out == np.arange(n, dtype=np.uint32)).sum())


def labels_fast(n, lhs, rhs, labels_in=None):
    """the same result for long edge lists, in whole-array steps: every edge pulls the labels of its two ends and of
    their current representatives down to the smaller one, then every label jumps to its label's label, until nothing
    changes.  tests/test_cluster_ref.py holds it to labels()."""
    n = int(n)
    a = np.asarray(lhs, np.int64).reshape(-1)
    b = np.asarray(rhs, np.int64).reshape(-1)
    if labels_in is not None:
        a = np.concatenate([a, np.arange(n, dtype=np.int64)])
        b = np.concatenate([b, np.asarray(labels_in, np.int64).reshape(-1)])
    assert a.size == b.size and (a.size == 0 or (min(a.min(), b.min()) >= 0 and max(a.max(), b.max()) < n))
    lab = np.arange(n, dtype=np.int64)
    while True:
        la, lb = lab[a], lab[b]
        mn = np.minimum(la, lb)
        new = lab.copy()
        for idx in (a, b, la, lb):
            np.minimum.at(new, idx, mn)
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, lab):
            break
        lab = new
    out = lab.astype(np.uint32)
    return out, int((lab == np.arange(n)).sum())


def csr_edges(row_ptr, col, row_begin=0):
    """(lhs, rhs) of the hits of a CSR as dist_threshold gives it: hit h of row r is the edge (row_begin + r, col[h])"""
    rp = np.asarray(row_ptr, np.int64)
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))
    return (rows + row_begin).astype(np.uint32), np.asarray(col, np.uint32)[int(rp[0]) : int(rp[-1])]


def is_labelling(lab):
    """what every result must satisfy whatever the graph: labels[x] <= x and labels[labels[x]] == labels[x]"""
    lab = np.asarray(lab, np.int64)
    return bool((lab <= np.arange(lab.size)).all() and (lab[lab] == lab).all())


# ---- the graphs of tests/test_cluster_host.py and tests/test_gpu_cluster.py ------------------------------------------
def chain(n):
    a = np.arange(n - 1, dtype=np.uint32)
    return a, a + 1


def star(n, hub):
    a = np.array([x for x in range(n) if x != hub], np.uint32)
    return np.full(a.size, hub, np.uint32), a


def two_cliques(m):
    """two cliques of m nodes (0..m-1 and m..2m-1) and the ONE edge that joins them, returned apart"""
    i, j = np.triu_indices(m, 1)
    lhs = np.concatenate([i, i + m]).astype(np.uint32)
    rhs = np.concatenate([j, j + m]).astype(np.uint32)
    return lhs, rhs, (np.array([m - 1], np.uint32), np.array([2 * m - 1], np.uint32))


def random_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, m).astype(np.uint32), rng.integers(0, n, m).astype(np.uint32)


def small_graphs():
    """(name, n, lhs, rhs): the hand cases and small instances of every family"""
    e = np.zeros(0, np.uint32)
    out = [("no nodes", 0, e, e), ("one node", 1, e, e), ("one node, self loop", 1, np.array([0], np.uint32), np.array([0], np.uint32)),
           ("no edges", 7, e, e), ("self loops", 5, np.arange(5, dtype=np.uint32), np.arange(5, dtype=np.uint32))]
    out.append(("chain", 10) + chain(10))
    a, b = chain(10)
    out.append(("chain descending", 10, b[::-1].copy(), a[::-1].copy()))
    out.append(("deep chain", 10, np.array([8, 6, 4, 2, 0, 7, 5, 3, 1], np.uint32), np.array([9, 7, 5, 3, 1, 8, 6, 4, 2], np.uint32)))
    out.append(("star, hub last", 9) + star(9, 8))
    out.append(("star, hub first", 9) + star(9, 0))
    l, r, (jl, jr) = two_cliques(6)
    out.append(("cliques apart", 12, l, r))
    out.append(("cliques joined last", 12, np.concatenate([l, jl]), np.concatenate([r, jr])))
    out.append(("cliques joined first", 12, np.concatenate([jl, l]), np.concatenate([jr, r])))
    l, r = random_graph(40, 25, 3)
    out.append(("random, each edge four times", 40, np.tile(l, 4), np.tile(r, 4)))
    for s in range(4):
        for m in (50, 100, 200, 800):
            out.append(("random n=200 m=%d seed=%d" % (m, s), 200) + random_graph(200, m, 100 * m + s))
    return out
