"""CPU: the numpy model of the density clusters (tests/dbscan_ref.py) held to a textbook DBSCAN -- seed and expand over region
queries, written here independently -- and to the single-linkage reference at min_pts 1 and 2.  A textbook DBSCAN gives a
border to whichever cluster reaches it first, so the comparison is: equal core sets, an equal partition of the cores, an equal
noise set, and every border in a cluster that holds one of its core neighbours."""
import numpy as np
import pytest

import cluster_ref
import dbscan_ref


def textbook(n, lhs, rhs, min_pts):
    """(cluster id per node or -1, core flags): Ester et al. 1996, the point itself counted in its neighbourhood"""
    nb = [[] for _ in range(n)]
    for a, b in zip(np.asarray(lhs).tolist(), np.asarray(rhs).tolist()):
        nb[a].append(b)
        nb[b].append(a)
    UNSEEN, NOISE = -2, -1
    cid = [UNSEEN] * n
    core = [len(nb[x]) + 1 >= min_pts for x in range(n)]
    nxt = 0
    for x in range(n):
        if cid[x] != UNSEEN:
            continue
        if not core[x]:
            cid[x] = NOISE
            continue
        cid[x] = nxt
        seeds = list(nb[x])
        while seeds:
            y = seeds.pop()
            if cid[y] == NOISE:
                cid[y] = nxt  # a border
            if cid[y] != UNSEEN:
                continue
            cid[y] = nxt
            if core[y]:
                seeds.extend(nb[y])
        nxt += 1
    return np.array(cid), np.array(core, bool)


def graphs():
    out = []
    for name, n, lhs, rhs in cluster_ref.small_graphs():
        lo, hi = np.minimum(lhs, rhs).astype(np.int64), np.maximum(lhs, rhs).astype(np.int64)
        keep = lo != hi
        e = np.unique(lo[keep] * max(n, 1) + hi[keep])  # every pair once, no self loops
        out.append((name, n, (e // max(n, 1)).astype(np.uint32), (e % max(n, 1)).astype(np.uint32), None))
    out.append(("chain 50", 50) + dbscan_ref.chain(50))
    for hub in (0, 10, 20):
        out.append(("star hub %d" % hub, 21) + dbscan_ref.star(21, hub))
    for where in ("first", "middle", "last"):
        n, _, _, e = dbscan_ref.bridged_cliques(8, where, 0.9, 0.8)
        out.append(("bridged " + where, n) + e)
    rng = np.random.default_rng(2024)
    for g in range(300):
        n = int(rng.integers(2, 60))
        dens = (1.0 / n, 5.0 / n, 0.5)[g % 3]
        i, j = np.triu_indices(n, 1)
        keep = rng.random(i.size) < dens
        val = rng.integers(1, 5, int(keep.sum())).astype(np.float32) / 4  # few distinct values: exact ties are common
        out.append(("random %d" % g, n, i[keep].astype(np.uint32), j[keep].astype(np.uint32), val))
    return out


GRAPHS = graphs()


def check_against_textbook(name, n, lhs, rhs, val, min_pts):
    val = np.ones(len(lhs), np.float32) if val is None else val
    cid, core = textbook(n, lhs, rhs, min_pts)
    for assign in ("first", "best"):
        for desc in (True, False):
            lab, kind, deg, nc, nn = dbscan_ref.dbscan(n, lhs, rhs, val, min_pts, assign, desc)
            what = (name, min_pts, assign, desc)
            assert np.array_equal(kind == dbscan_ref.CORE, core), what
            assert np.array_equal(kind == dbscan_ref.NOISE, cid == -1), what
            assert dbscan_ref.is_labelling(lab), what
            # an equal partition of the cores: the pairs (label, textbook id) over the cores are a bijection
            pairs = set(zip(lab[core].tolist(), cid[core].tolist()))
            assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}) == nc, what
            assert all(lab[l] == l and core[l] and l == np.flatnonzero(lab == l)[core[lab == l]].min() for l, _ in pairs), what
            assert nn == int((cid == -1).sum()) and (lab[cid == -1] == np.flatnonzero(cid == -1)).all(), what
            # every border in a cluster that holds one of its core neighbours; "best" means no neighbouring core has a better value
            for x in np.flatnonzero(kind == dbscan_ref.BORDER).tolist():
                at = [(int(b if a == x else a), float(v)) for a, b, v in zip(lhs.tolist(), rhs.tolist(), val.tolist()) if x in (a, b)]
                cn = [(c, v) for c, v in at if core[c]]
                assert cn and len(at) + 1 < min_pts, what
                assert lab[x] in {lab[c] for c, _ in cn}, what
                if assign == "first":
                    assert lab[x] == lab[min(c for c, _ in cn)], what
                else:
                    bestv = max(v for _, v in cn) if desc else min(v for _, v in cn)
                    assert lab[x] == lab[min(c for c, v in cn if v == bestv)], what


@pytest.mark.parametrize("min_pts", [1, 2, 3, 4, 6])
def test_model_equals_a_textbook_dbscan(min_pts):
    for name, n, lhs, rhs, val in GRAPHS:
        if n:
            check_against_textbook(name, n, lhs, rhs, val, min_pts)


def test_model_against_sklearn_where_it_is_installed():
    sk = pytest.importorskip("sklearn.cluster")
    for name, n, lhs, rhs, val in GRAPHS[::7]:
        if n < 2:
            continue
        d = np.full((n, n), 2.0)
        d[lhs, rhs] = d[rhs, lhs] = 0.5
        np.fill_diagonal(d, 0.0)
        for min_pts in (1, 2, 3, 5):
            m = sk.DBSCAN(eps=1.0, min_samples=min_pts, metric="precomputed").fit(d)
            lab, kind, _, _, _ = dbscan_ref.dbscan(n, lhs, rhs, np.ones(len(lhs), np.float32), min_pts)
            core = np.zeros(n, bool)
            core[m.core_sample_indices_] = True
            assert np.array_equal(kind == dbscan_ref.CORE, core), (name, min_pts)
            assert np.array_equal(kind == dbscan_ref.NOISE, m.labels_ == -1), (name, min_pts)


def test_min_pts_one_and_two_are_the_components():
    for name, n, lhs, rhs, val in GRAPHS:
        want, wc = cluster_ref.labels(n, lhs, rhs)
        v = np.ones(len(lhs), np.float32)
        lab, kind, deg, nc, nn = dbscan_ref.dbscan(n, lhs, rhs, v, 1)
        assert np.array_equal(lab, want) and nc == wc and nn == 0 and (kind == dbscan_ref.CORE).all(), name
        lab, kind, deg, nc, nn = dbscan_ref.dbscan(n, lhs, rhs, v, 2, "best")
        assert np.array_equal(lab, want) and nc == wc - nn and nn == int((deg == 0).sum()), name
        assert not (kind == dbscan_ref.BORDER).any(), name
        lab, kind, deg, nc, nn = dbscan_ref.dbscan(n, lhs, rhs, v, n + 1)
        assert nc == 0 and nn == n and np.array_equal(lab, np.arange(n, dtype=np.uint32)), name


def test_cores_shrink_with_min_pts_and_a_non_core_has_few_edges():
    for name, n, lhs, rhs, val in GRAPHS:
        v = np.ones(len(lhs), np.float32)
        before = np.ones(n, bool)
        for min_pts in range(1, 9):
            _, kind, deg, _, _ = dbscan_ref.dbscan(n, lhs, rhs, v, min_pts)
            core = kind == dbscan_ref.CORE
            assert not (core & ~before).any(), (name, min_pts)
            assert (deg[~core].astype(np.int64) <= min_pts - 2).all(), (name, min_pts)
            before = core


def test_the_hand_graphs():
    # chain: at 3 the ends are borders of the one cluster, whose label is its smallest CORE, 1; at 4 all is noise
    lhs, rhs, val = dbscan_ref.chain(30)
    lab, kind, deg, nc, nn = dbscan_ref.dbscan(30, lhs, rhs, val, 3)
    assert (lab == 1).all() and nc == 1 and nn == 0 and kind[0] == kind[29] == dbscan_ref.BORDER and (kind[1:29] == dbscan_ref.CORE).all()
    assert dbscan_ref.dbscan(30, lhs, rhs, val, 4)[4] == 30
    # the bridge is a border and the cliques stay two clusters, while single linkage welds them
    for where in ("first", "middle", "last"):
        n, bridge, (ca, cb), (lhs, rhs, val) = dbscan_ref.bridged_cliques(8, where, 0.9, 0.8)
        assert cluster_ref.labels(n, lhs, rhs)[1] == 1
        for assign, desc, to in (("first", True, min(ca, cb)), ("best", True, ca), ("best", False, cb)):
            lab, kind, deg, nc, nn = dbscan_ref.dbscan(n, lhs, rhs, val, 8, assign, desc)
            assert nc == 2 and nn == 0 and kind[bridge] == dbscan_ref.BORDER and lab[bridge] == lab[to] != lab[ca if to == cb else cb]
