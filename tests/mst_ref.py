"""Reference models of the minimum spanning tree of the pair values (dsh_mst*, include/dashing_hip.h), sharing nothing with the
code under test.

The definition: values are float32 in dsh_tri_index order (np.triu_indices(n, 1)); the pair {x, y} is an edge iff its value is
not NaN and passes the cutoff (>= for similarities = descending, <= for distances); edge (i, j), i < j, is better than another
iff it comes first by (the better value, the smaller i, the smaller j), -0.0 equal to +0.0; the result is the forest Kruskal's
algorithm builds from the edges in that order, listed best first, with a zero reported as +0.0.

  kruskal   the definition, literally: sort, then union-find
  prim      numpy, for large n: Prim's algorithm from the smallest unvisited node over packed uint64 ranks (key, i, j); the
            strict total order makes its forest the same one
  linkage   the sorted edge list as a merge table (scipy's Z convention, the two ids of a row ordered)
and the matrix families of the tests."""
import numpy as np

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def no_cutoff(descending):
    return -np.inf if descending else np.inf


def vkey(v, descending):
    """uint32, larger = better; equal floats (-0.0 == +0.0) have equal keys.  NaN entries are meaningless."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    u = np.where(neg, ~u, u | np.uint32(0x80000000))
    return u if descending else ~u


def passing(tri, descending, cutoff):
    tri = np.asarray(tri, np.float32)
    c = np.float32(cutoff)
    return ~np.isnan(tri) & ((tri >= c) if descending else (tri <= c))


def kruskal(n, tri, descending, cutoff):
    """(lhs, rhs, val, labels)"""
    tri = np.ascontiguousarray(tri, np.float32)
    iu, ju = np.triu_indices(n, 1)
    key = vkey(tri, descending).astype(np.int64)
    order = np.lexsort((ju, iu, -key))
    order = order[passing(tri, descending, cutoff)[order]]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    took = []
    for e in order.tolist():
        a, b = find(int(iu[e])), find(int(ju[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            took.append(e)
            if len(took) == n - 1:
                break
    took = np.array(took, np.int64)
    labels = np.array([find(x) for x in range(n)], np.uint32)
    return iu[took].astype(np.uint32), ju[took].astype(np.uint32), tri[took] + np.float32(0), labels


def prim(n, tri, descending, cutoff):
    """(lhs, rhs, val, labels), O(n^2) numpy"""
    tri = np.ascontiguousarray(tri, np.float32)
    b = max((n - 1).bit_length(), 1)
    assert 32 + 2 * b <= 64
    inv = (np.uint64(0xFFFFFFFF) - vkey(tri, descending).astype(np.uint64)) << np.uint64(2 * b)  # smaller = better
    inv[~passing(tri, descending, cutoff)] = NONE
    ar = np.arange(n, dtype=np.int64)
    off = ar * n - ar * (ar + 1) // 2 - (ar + 1)  # tri index of (i, j), i < j: off[i] + j

    def row(x):
        r = np.full(n, NONE, np.uint64)
        lo = inv[off[:x] + x]
        r[:x] = np.where(lo == NONE, NONE, lo | (ar[:x].astype(np.uint64) << np.uint64(b)) | np.uint64(x))
        hi = inv[off[x] + x + 1 : off[x] + n] if x + 1 < n else inv[:0]
        r[x + 1 :] = np.where(hi == NONE, NONE, hi | (np.uint64(x) << np.uint64(b)) | ar[x + 1 :].astype(np.uint64))
        return r

    best = np.full(n, NONE, np.uint64)
    in_tree = np.zeros(n, bool)
    labels = np.zeros(n, np.uint32)
    ranks = []
    for s in range(n):
        if in_tree[s]:
            continue
        y = s
        while True:
            in_tree[y] = True
            labels[y] = s
            best = np.minimum(best, row(y))
            best[in_tree] = NONE
            y = int(np.argmin(best))
            if best[y] == NONE:
                break
            ranks.append(best[y])
    ranks = np.sort(np.array(ranks, np.uint64))
    mask = np.uint64((1 << b) - 1)
    lhs, rhs = ((ranks >> np.uint64(b)) & mask).astype(np.int64), (ranks & mask).astype(np.int64)
    return lhs.astype(np.uint32), rhs.astype(np.uint32), tri[off[lhs] + rhs] + np.float32(0), labels


def linkage(n, lhs, rhs):
    """(za, zb, zsize) of the edge list taken in its order"""
    parent, cid, size = list(range(n)), list(range(n)), [1] * n

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    za, zb, zs = [], [], []
    for s, (a, b) in enumerate(zip(np.asarray(lhs).tolist(), np.asarray(rhs).tolist())):
        a, b = find(a), find(b)
        assert a != b
        za.append(min(cid[a], cid[b]))
        zb.append(max(cid[a], cid[b]))
        parent[b] = a
        size[a] += size[b]
        cid[a] = n + s
        zs.append(size[a])
    return np.array(za, np.uint32), np.array(zb, np.uint32), np.array(zs, np.uint32)


# ---- the matrix families

def span(n):
    return n * (n - 1) // 2


def ties(n, seed):
    """four distinct floats (heavy ties), 20 % NaN (forests), and both zeros and both infinities present where there is room"""
    rng = np.random.default_rng(seed)
    tri = rng.choice(np.array([0.125, 0.25, 0.5, 0.75], np.float32), span(n))
    tri[rng.random(span(n)) < 0.2] = np.nan
    special = np.array([0.0, -0.0, np.inf, -np.inf, -0.0, 0.0], np.float32)
    at = rng.permutation(span(n))[: special.size]
    tri[at] = special[: at.size]
    return tri


def tie_free(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.permutation(span(n)).astype(np.float32) + 1) / np.float32(span(n) + 1)


def all_nan(n):
    return np.full(span(n), np.nan, np.float32)


def all_equal(n, v=0.5):
    return np.full(span(n), v, np.float32)


def ultrametric(n, descending):
    """v(i, j) = the bit length of i ^ j as a distance; negated as a similarity, so that in both directions the best partner
    differs in the lowest bit.  Every round pairs the components up: n = 2^r takes exactly r rounds"""
    iu, ju = np.triu_indices(n, 1)
    x = iu ^ ju
    bl = np.zeros(x.size, np.float32)
    while x.any():
        bl += x > 0
        x = x >> 1
    return -bl if descending else bl


def families():
    """(name, n, tri) of the host and device tests"""
    out = [("empty", 0, np.zeros(0, np.float32)), ("one", 1, np.zeros(0, np.float32)), ("two", 2, np.array([0.5], np.float32)),
           ("two-nan", 2, all_nan(2)), ("three", 3, np.array([0.5, 0.25, 0.5], np.float32)), ("all-nan", 20, all_nan(20)),
           ("all-equal", 50, all_equal(50))]
    for k, n in enumerate((5, 9, 17, 40, 200)):
        out.append(("ties-%d" % n, n, ties(n, 40 + k)))
    out.append(("tie-free-33", 33, tie_free(33, 7)))
    return out


def cutoffs(tri, descending):
    fin = tri[np.isfinite(tri)]
    return [no_cutoff(descending), float(np.median(fin)) if fin.size else 0.5, float("nan")]
