"""Reference of dsh_group_stats* (include/dashing_hip.h): the statistics of a labelling over a FULL symmetric float32 matrix
V (V[x][y] = V[y][x] = the value of the pair; the diagonal is never read).  Two forms written from the header's sentences,
held to each other by tests/test_group_stats_ref.py; nothing here is shared with the code under test.

  included(x, y)  x != y, labels equal, V[x][y] not NaN and |V[x][y]| < 2
  q(v)            rint(float64(v) * 2^30): round to nearest even of an exact product
  cnt[x]          included pairs of x                               uint32
  sum[x]          sum of q over them                                int64
  worst[x]        the smallest (similarity) / largest (distance) included value as float32, -0.0 taken as +0.0; NaN: none
  medoid[x]       the member of x's group with the largest cnt, then the best sum (largest / smallest), then the smallest slot
"""
import numpy as np

FRAC_BITS = 30
SIMILARITY = (1, 5, 7)  # JI, CONTAINMENT_INDEX, SYMMETRIC_CONTAINMENT_INDEX: a larger value is better


def square(tri, n):
    """the full symmetric matrix of a packed triangle (row i: the columns i + 1 ...), diagonal NaN"""
    V = np.full((n, n), np.nan, np.float32)
    i, j = np.triu_indices(n, 1)
    V[i, j] = tri
    V[j, i] = tri
    return V


def q(v):
    return np.rint(np.asarray(v, np.float32).astype(np.float64) * float(1 << FRAC_BITS)).astype(np.int64)


class Ref:
    """what does not depend on the labels, computed once per matrix"""

    def __init__(self, V, descending):
        V = np.asarray(V, np.float32)
        n = V.shape[0]
        assert V.shape == (n, n)
        self.n, self.descending = n, bool(descending)
        with np.errstate(invalid="ignore"):
            self.valid = ~np.isnan(V) & (np.abs(V) < 2)
        self.valid[np.arange(n), np.arange(n)] = False
        self.q = np.where(self.valid, q(np.where(self.valid, V, 0)), 0)
        self.vz = np.where(self.valid, V + np.float32(0.0), np.float32(np.inf if descending else -np.inf))  # (-0.0 + 0.0 = +0.0)

    def stats(self, labels):
        """(medoid uint32, cnt uint32, sum int64, worst float32)"""
        n = self.n
        lab = np.asarray(labels, np.int64).reshape(-1)
        assert lab.size == n and ((lab >= 0) & (lab < max(n, 1))).all()
        inc = self.valid & (lab[:, None] == lab[None, :])
        cnt = inc.sum(1).astype(np.uint32)
        sm = np.where(inc, self.q, 0).sum(1).astype(np.int64)
        pad = np.float32(np.inf if self.descending else -np.inf)
        w = np.where(inc, self.vz, pad)
        worst = (w.min(1) if self.descending else w.max(1)).astype(np.float32) if n else np.zeros(0, np.float32)
        worst[cnt == 0] = np.nan
        return medoids(lab, cnt, sm, self.descending), cnt, sm, worst


def medoids(lab, cnt, sm, descending):
    n = lab.size
    # best first inside every group: label, then cnt descending, then the better sum, then the slot
    order = np.lexsort((np.arange(n), -sm if descending else sm, -cnt.astype(np.int64), lab))
    first = np.ones(n, bool)
    first[1:] = lab[order][1:] != lab[order][:-1]
    best = np.zeros(max(n, 1), np.int64)
    best[lab[order][first]] = order[first]
    return best[lab].astype(np.uint32)[:n]


def brute(V, labels, descending):
    """the same with Python loops and Python integers, for n <= 64"""
    V = np.asarray(V, np.float32)
    n = V.shape[0]
    assert n <= 64
    cnt, sm, worst = [0] * n, [0] * n, [float("nan")] * n
    for x in range(n):
        for y in range(n):
            v = V[x, y]
            if x == y or labels[x] != labels[y] or v != v or not abs(float(v)) < 2:
                continue
            cnt[x] += 1
            sm[x] += int(np.rint(np.float64(v) * 2.0**FRAC_BITS))
            f = float(v) + 0.0
            if worst[x] != worst[x] or (f < worst[x] if descending else f > worst[x]):
                worst[x] = f
    med = [0] * n
    for x in range(n):
        members = [m for m in range(n) if labels[m] == labels[x]]
        med[x] = min(members, key=lambda m: (-cnt[m], -sm[m] if descending else sm[m], m))
    return (np.array(med, np.uint32), np.array(cnt, np.uint32), np.array(sm, np.int64), np.array(worst, np.float32))


def same(got, want):
    """exact equality of the four arrays, worst as float values with NaN == NaN (so -0.0 == +0.0)"""
    return (all(np.array_equal(np.asarray(g), np.asarray(w)) for g, w in zip(got[:3], want[:3]))
            and np.array_equal(np.asarray(got[3], np.float32), np.asarray(want[3], np.float32), equal_nan=True))


def diameter(labels, worst, descending):
    """per slot the worst `worst` of its group; NaN: the group has no included pair"""
    lab = np.asarray(labels, np.int64)
    out = np.full(lab.size, np.nan, np.float32)
    for g in np.unique(lab):
        w = worst[lab == g]
        w = w[~np.isnan(w)]
        if w.size:
            out[lab == g] = w.min() if descending else w.max()
    return out
