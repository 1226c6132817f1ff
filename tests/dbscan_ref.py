"""numpy reference of the density clusters at a threshold (include/dashing_hip.h, dsh_dbscan_*), from an edge list: the
edges are the unordered pairs that pass the threshold, each ONCE, val[e] its float32 value.
  degree[x]   the edges at x (bincount over both ends)
  core        degree[x] + 1 >= min_pts (the point counts itself)
  clusters    the connected components of the core-core edges (cluster_ref.labels_fast), labelled with their smallest core
  border      a non-core with a core neighbour: "first" takes the smallest one, "best" the one with the best value (equal float32
              values, -0.0 equal to +0.0, to the smaller core) -- one lexsort each
  noise       every other non-core, labelled with itself
Nothing here is shared with the code under test.  Plain helper module, importable without a device."""
import numpy as np

import cluster_ref

NOISE, BORDER, CORE = 0, 1, 2


def degrees(n, lhs, rhs):
    a = np.asarray(lhs, np.int64).reshape(-1)
    b = np.asarray(rhs, np.int64).reshape(-1)
    assert a.size == b.size and not (a == b).any()
    return (np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(np.uint32)


def core_labels(n, lhs, rhs, core):
    """labels of the graph restricted to the edges between two cores (a non-core keeps itself), as int64"""
    a = np.asarray(lhs, np.int64).reshape(-1)
    b = np.asarray(rhs, np.int64).reshape(-1)
    cc = core[a] & core[b]
    return cluster_ref.labels_fast(n, a[cc], b[cc])[0].astype(np.int64)


def dbscan(n, lhs, rhs, val, min_pts, assign="first", descending=True, core_lab=None, deg=None):
    """(labels uint32 [n], kind uint8 [n], degree uint32 [n], n_clusters, n_noise).  deg, core_lab: degrees() of the same graph and
    core_labels() of it under the same min_pts, where the caller has them already (long edge lists)"""
    assert assign in ("first", "best") and min_pts >= 1
    n = int(n)
    a = np.asarray(lhs, np.int64).reshape(-1)
    b = np.asarray(rhs, np.int64).reshape(-1)
    v = np.asarray(val, np.float32).reshape(-1)
    assert a.size == b.size == v.size and not np.isnan(v).any()
    deg = degrees(n, a, b) if deg is None else np.asarray(deg, np.uint32)
    core = deg.astype(np.int64) + 1 >= int(min_pts)
    lab = core_labels(n, a, b, core) if core_lab is None else np.asarray(core_lab, np.int64).copy()
    kind = np.where(core, CORE, NOISE).astype(np.uint8)
    # the edges with exactly one core end, as (border candidate, core, value)
    one = core[a] != core[b] if core.any() and not core.all() else np.zeros(a.size, bool)  # (no edge has ends of two kinds)
    bo = np.where(core[a[one]], b[one], a[one])
    co = np.where(core[a[one]], a[one], b[one])
    if bo.size:
        vv = v[one].astype(np.float64) + 0.0  # (-0.0 becomes +0.0; float64 holds every float32, the infinities included)
        rank = -vv if descending else vv      # smaller = better
        order = np.lexsort((co, bo)) if assign == "first" else np.lexsort((co, rank, bo))
        bo, co = bo[order], co[order]
        firsts = np.concatenate([[True], bo[1:] != bo[:-1]])
        lab[bo[firsts]] = lab[co[firsts]]
        kind[bo[firsts]] = BORDER
    n_clusters = int((core & (lab == np.arange(n))).sum())
    return lab.astype(np.uint32), kind, deg, n_clusters, int((kind == NOISE).sum())


def tri_edges(n, tri, threshold, descending):
    """(lhs, rhs, val) of the packed triangle's values that pass: v >= t (descending) or v <= t; NaN never"""
    tri = np.asarray(tri, np.float32).reshape(-1)
    i, j = np.triu_indices(n, 1)
    with np.errstate(invalid="ignore"):
        hit = (tri >= np.float32(threshold)) if descending else (tri <= np.float32(threshold))
    return i[hit].astype(np.uint32), j[hit].astype(np.uint32), tri[hit]


def is_labelling(lab):
    """labels[labels[x]] == labels[x] (a border's label may be larger than its slot)"""
    lab = np.asarray(lab, np.int64)
    return bool((lab[lab] == lab).all())


# ---- the hand graphs of tests/test_dbscan_ref.py and tests/test_gpu_dbscan.py: (lhs, rhs, val) with lhs < rhs ----------
def edge_list(pairs, vals=None):
    p = np.array(sorted((min(x), max(x)) for x in pairs), np.int64).reshape(-1, 2)
    if vals is None:
        v = np.ones(p.shape[0], np.float32)
    else:
        d = {(min(x), max(x)): w for x, w in zip(pairs, vals)}
        v = np.array([d[(int(x), int(y))] for x, y in p], np.float32)
    return p[:, 0].astype(np.uint32), p[:, 1].astype(np.uint32), v


def chain(n):
    return edge_list([(x, x + 1) for x in range(n - 1)])


def star(n, hub):
    return edge_list([(hub, x) for x in range(n) if x != hub])


def bridged_cliques(m, where, va=1.0, vb=1.0):
    """two cliques of m nodes and one bridge node adjacent to ONE member of each, with the values va (first clique) and vb;
    where: "first" (the bridge is slot 0), "middle" (slot m) or "last" (slot 2m).  Returns (n, bridge, (ca, cb), edges):
    ca, cb the clique members the bridge touches"""
    n = 2 * m + 1
    bridge = {"first": 0, "middle": m, "last": 2 * m}[where]
    rest = [x for x in range(n) if x != bridge]
    A, B = rest[:m], rest[m:]
    pairs = [(A[x], A[y]) for x in range(m) for y in range(x + 1, m)] + [(B[x], B[y]) for x in range(m) for y in range(x + 1, m)]
    vals = [1.0] * len(pairs)
    ca, cb = A[m // 2], B[m // 2]
    pairs += [(bridge, ca), (bridge, cb)]
    vals += [va, vb]
    return n, bridge, (ca, cb), edge_list(pairs, vals)


def to_tri(n, lhs, rhs, val, fill=0.0):
    """the packed triangle (dsh_tri_index order) that holds val at the edges and `fill` elsewhere"""
    m = np.full((n, n), fill, np.float32)
    m[np.asarray(lhs, np.int64), np.asarray(rhs, np.int64)] = np.asarray(val, np.float32)
    return m[np.triu_indices(n, 1)]
