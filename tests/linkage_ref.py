"""Reference models of the linkage clusters at a threshold (include/dashing_hip.h, dsh_linkage_*).  Two
models that share nothing with the code under test and little with each other:

  literal(n, tri, descending, t, linkage)   the definition as it is written: D of every pair of current clusters recomputed
                                            from the member pairs at every step, Python integers and Fractions for the
                                            rationals.  O(n^4): for n <= 24.
  labels(n, tri, descending, t, linkage)    Lance-Williams updates on numpy matrices with a per-row best partner, for the
                                            sizes the GPU tests use.  Keys and sums are integers, so it is exact; float64
                                            ratios only shortlist the AVERAGE candidates, Python integers decide.

tri holds the n (n - 1) / 2 float32 values in dsh_tri_index order (np.triu_indices(n, 1)).  Both return
(labels uint32 [n], n_clusters).  tests/test_linkage_ref.py holds them to each other.  Plain helper module, importable
without a device."""
from fractions import Fraction

import numpy as np

SINGLE, COMPLETE, AVERAGE = 0, 1, 2
NAMES = {"single": SINGLE, "complete": COMPLETE, "average": AVERAGE}
FRAC = 30


def keys(v, descending):
    """value_key32 of an array of float32: larger = better, -0.0 = +0.0, NaN -> 0"""
    v = np.ascontiguousarray(v, np.float32)
    u = v.view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    u = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    if not descending:
        u = ~u & 0xFFFFFFFF
    return np.where(np.isnan(v), 0, u).astype(np.uint32)


def q(v):
    """llrint((double)v * 2^30), round half to even; the product is exact in double"""
    with np.errstate(invalid="ignore"):  # (what NaN and inf become is never read: they are blocked or refused before)
        return np.rint(np.asarray(v, np.float32).astype(np.float64) * float(1 << FRAC)).astype(np.int64)


def thr_pass(v, t, descending):
    v, t = np.float32(v), np.float32(t)
    return bool(v >= t) if descending else bool(v <= t)


def square(n, tri):
    v = np.zeros((n, n), np.float32)
    i, j = np.triu_indices(n, 1)
    tri = np.asarray(tri, np.float32).reshape(-1)
    assert tri.size == i.size
    v[i, j] = tri
    v[j, i] = tri
    return v


def _finish(n, members):
    lab = np.arange(n, dtype=np.uint32)
    for ms in members:
        lab[list(ms)] = min(ms)
    return lab, int((lab == np.arange(n)).sum())


def literal(n, tri, descending, t, linkage):
    n = int(n)
    t = np.float32(t)
    if n == 0 or np.isnan(t):
        return np.arange(n, dtype=np.uint32), n
    v = square(n, tri)
    ky = keys(v, descending).astype(np.int64)
    qq = q(np.where(np.isnan(v), 0, v))
    excl = np.isnan(v) | ~(np.abs(v) < 2)
    Q = int(q(t))
    clusters = [[x] for x in range(n)]  # each sorted; label = first member
    while True:
        best = None  # (value to maximise, -label a, -label b) -> pair
        for ia in range(len(clusters)):
            for ib in range(ia + 1, len(clusters)):
                A, B = clusters[ia], clusters[ib]
                la, lb = (A[0], B[0]) if A[0] < B[0] else (B[0], A[0])
                sub = np.ix_(A, B)
                if linkage == SINGLE:
                    k = int(ky[sub].max())  # NaN has key 0, below every value
                    if k == 0:
                        continue
                    x, y = np.argwhere(ky[sub] == k)[0]
                    if not thr_pass(v[A[x], B[y]], t, descending):
                        continue
                    val = k
                elif linkage == COMPLETE:
                    k = int(ky[sub].min())
                    if k == 0:
                        continue
                    x, y = np.argwhere(ky[sub] == k)[0]
                    if not thr_pass(v[A[x], B[y]], t, descending):
                        continue
                    val = k
                else:
                    if excl[sub].any():
                        continue
                    S, c = sum(int(z) for z in qq[sub].reshape(-1)), len(A) * len(B)
                    if not (S >= Q * c if descending else S <= Q * c):
                        continue
                    val = Fraction(S, c) if descending else -Fraction(S, c)
                cand = (val, -la, -lb)
                if best is None or cand > best[0]:
                    best = (cand, ia, ib)
        if best is None:
            break
        _, ia, ib = best
        merged = sorted(clusters[ia] + clusters[ib])
        clusters = [c for x, c in enumerate(clusters) if x not in (ia, ib)] + [merged]
    return _finish(n, clusters)


class _Keyed:
    """SINGLE / COMPLETE: uint32 keys, 0 = blocked"""

    def __init__(self, v, descending, t, linkage):
        self.c = keys(v, descending).astype(np.int64)
        np.fill_diagonal(self.c, 0)
        self.tkey = int(keys(np.array([t], np.float32), descending)[0])
        self.merge = np.maximum if linkage == SINGLE else np.minimum

    def rescan(self, rows, alive, size):
        sub = np.where(alive[None, :], self.c[rows], 0)
        sub[np.arange(len(rows)), rows] = 0
        j = sub.argmax(axis=1)  # the first of equal maxima: the smaller partner
        val = sub[np.arange(len(rows)), j]
        return np.where(val > 0, j, -1), val

    def better_new(self, k, new, a, nn, nnv, size):
        """rows k (nn[k] not among the merged) whose new cell with a beats what they hold"""
        return (new > 0) & ((nn[k] < 0) | (new > nnv[k]) | ((new == nnv[k]) & (a < nn[k])))

    def best(self, rows, nn, nnv, size):
        val = nnv[rows]
        top = rows[val == val.max()]
        lo, hi = np.minimum(top, nn[top]), np.maximum(top, nn[top])
        x = np.lexsort((hi, lo))[0]
        return int(lo[x]), int(hi[x])

    def passes(self, a, b, size):
        return int(self.c[a, b]) >= self.tkey


class _Averaged:
    """AVERAGE: int64 sums, a mask for blocked; a value is the rational S / (size product)"""
    TOL = 1e-3  # float64 ratios of |S / c| < 2^31 are off by less than 2^-20: everything within TOL is decided exactly

    def __init__(self, v, descending, t):
        bad = np.isnan(v) | ~(np.abs(v) < 2)
        self.c = q(np.where(bad, 0, v))
        self.blocked = bad
        np.fill_diagonal(self.blocked, True)
        self.Q = int(q(np.float32(t)))
        self.sign = 1 if descending else -1

    def merge(self, x, y):
        return x + y

    def exact_best(self, I, J, size):
        """the best of the candidates (I[x], J[x]) under the exact order, ties to the smaller (min, max): one Fraction per
        DISTINCT (S, c), so that a matrix of equal values costs no more than one of different ones"""
        I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
        sc = np.stack([self.c[I, J], size[I] * size[J]], axis=1)
        uniq, inv = np.unique(sc, axis=0, return_inverse=True)
        vals = [self.sign * Fraction(int(S), int(c)) for S, c in uniq]
        top = max(vals)
        tied = np.flatnonzero(np.array([v == top for v in vals])[inv.reshape(-1)])
        lo, hi = np.minimum(I[tied], J[tied]), np.maximum(I[tied], J[tied])
        x = tied[np.lexsort((hi, lo))[0]]
        return int(I[x]), int(J[x])

    def rescan(self, rows, alive, size):
        ok = alive[None, :] & ~self.blocked[rows]
        ratio = np.where(ok, self.sign * self.c[rows] / (size[rows][:, None] * size[None, :]).astype(np.float64), -np.inf)
        top = ratio.max(axis=1)
        near = ratio >= (top - self.TOL)[:, None]
        out = np.where(top == -np.inf, -1, ratio.argmax(axis=1)).astype(np.int64)
        for x in np.flatnonzero((near.sum(axis=1) > 1) & (top > -np.inf)):
            short = np.flatnonzero(near[x])
            out[x] = self.exact_best(np.full(short.size, rows[x]), short, size)[1]
        val = np.where(out >= 0, self.c[rows, np.maximum(out, 0)], 0)
        return out, val

    def better_new(self, k, new, a, nn, nnv, size):
        ok = ~self.blocked[a, k]
        rn = self.sign * new / (size[k] * size[a]).astype(np.float64)
        has = nn[k] >= 0
        rc = np.where(has, self.sign * nnv[k] / (size[k] * size[np.maximum(nn[k], 0)]).astype(np.float64), -np.inf)
        res = ok & (rn > rc + self.TOL)
        for x in np.flatnonzero(ok & has & (np.abs(rn - rc) <= self.TOL)):
            kk = int(k[x])
            res[x] = self.exact_best([kk, kk], [a, int(nn[kk])], size)[1] == a
        return res

    def best(self, rows, nn, nnv, size):
        ratio = self.sign * nnv[rows] / (size[rows] * size[nn[rows]]).astype(np.float64)
        short = rows[ratio >= ratio.max() - self.TOL]
        i, j = self.exact_best(short, nn[short], size)
        return min(i, j), max(i, j)

    def passes(self, a, b, size):
        S, c = int(self.c[a, b]), int(size[a]) * int(size[b])
        return S >= self.Q * c if self.sign > 0 else S <= self.Q * c


def labels(n, tri, descending, t, linkage):
    n = int(n)
    t = np.float32(t)
    if n < 2 or np.isnan(t):
        return np.arange(n, dtype=np.uint32), n
    v = square(n, tri)
    M = _Averaged(v, descending, t) if linkage == AVERAGE else _Keyed(v, descending, t, linkage)
    alive = np.ones(n, bool)
    size = np.ones(n, np.int64)
    root = np.arange(n)
    ar = np.arange(n)
    nn, nnv = M.rescan(ar, alive, size)
    while True:
        rows = np.flatnonzero(alive & (nn >= 0))
        if not rows.size:
            break
        a, b = M.best(rows, nn, nnv, size)
        if not M.passes(a, b, size):
            break
        k = np.flatnonzero(alive & (ar != a) & (ar != b))
        new = M.merge(M.c[a, k], M.c[b, k])
        M.c[a, k] = new
        M.c[k, a] = new
        if linkage == AVERAGE:
            blk = M.blocked[a, k] | M.blocked[b, k]
            M.blocked[a, k] = blk
            M.blocked[k, a] = blk
        alive[b] = False
        size[a] += size[b]
        root[root == b] = a
        nn[b] = -1
        stale = (nn[k] == a) | (nn[k] == b)
        keep = k[~stale]
        if keep.size:
            win = M.better_new(keep, M.c[a, keep], a, nn, nnv, size)
            nn[keep[win]] = a
            nnv[keep[win]] = M.c[a, keep[win]]
        again = np.concatenate([k[stale], [a]])
        nn[again], nnv[again] = M.rescan(again, alive, size)
    lab = root.astype(np.uint32)
    return lab, int((lab == ar).sum())


# ---- the matrices of the tests ---------------------------------------------------------------------------------------
def tri_of(v):
    v = np.asarray(v, np.float32)
    return np.ascontiguousarray(v[np.triu_indices(v.shape[0], 1)])


def path(n, good=0.1, bad=0.9):
    """distances: consecutive slots at `good`, every other pair at `bad`"""
    v = np.full((n, n), bad, np.float32)
    i = np.arange(n - 1)
    v[i, i + 1] = good
    return tri_of(v)


def two_blocks(m, inside=0.1, across=0.9, bridge=0.1, seed=None):
    """distances: two blocks of m slots, `inside` within a block (with a seed: different values within 0.05 of it),
    `across` between them but for the one pair (m - 1, 2 m - 1) at `bridge`"""
    v = np.full((2 * m, 2 * m), across, np.float32)
    v[:m, :m] = inside
    v[m:, m:] = inside
    if seed is not None:
        j = (np.random.default_rng(seed).random((2 * m, 2 * m)) * 0.1 - 0.05).astype(np.float32)
        v = np.where(v == np.float32(inside), v + np.minimum(j, j.T), v)
    v[m - 1, 2 * m - 1] = v[2 * m - 1, m - 1] = bridge
    return tri_of(v)


def funnel(n):
    """distances under which, at every step and under all three linkages, the nearest neighbour of EVERY cluster is the
    cluster of slot 0: d(x, y) = (y + x / (2 n)) / (2 n) for x < y, which the larger slot dominates.  The cluster {0 .. k} is
    then nearer to x > k than any slot between them or behind x, step k merges it with k + 1, and every row's nearest
    neighbour is one of the merged two each time: the rescans at their worst.  All values lie in [0, 0.51)."""
    x = np.arange(n, dtype=np.float64)
    lo, hi = np.minimum(x[:, None], x[None, :]), np.maximum(x[:, None], x[None, :])
    return tri_of(((hi + lo / (2.0 * n)) / (2.0 * n)).astype(np.float32))


def distinct_tri(n, seed):
    """distances in [0, 1) that are all different: a random order of the cells of a grid, each moved inside its cell"""
    rng = np.random.default_rng(seed)
    N = n * (n - 1) // 2
    return ((rng.permutation(N) + 0.5 * rng.random(N)) / max(N, 1)).astype(np.float32)


def random_tri(n, seed, special=True):
    """uniform distances in [0, 1) with, where `special`, NaN, +-0.0, +-inf, values at and above 2, ties, and values whose
    q sits at an exact half"""
    rng = np.random.default_rng(seed)
    t = rng.random(n * (n - 1) // 2).astype(np.float32)
    if special and t.size:
        pick = lambda frac: rng.random(t.size) < frac
        t[pick(0.02)] = np.nan
        t[pick(0.02)] = 0.0
        t[pick(0.02)] = -0.0
        t[pick(0.01)] = np.inf
        t[pick(0.01)] = -np.inf
        t[pick(0.02)] = 2.0
        t[pick(0.01)] = -2.5
        h = pick(0.05)
        t[h] = ((rng.integers(0, 1 << 20, int(h.sum())) * 2 + 1) * 2.0**-31).astype(np.float32)  # q at an exact half
        d = pick(0.1)
        t[d] = np.round(t[d] * 8) / 8  # ties
    return t
