"""CPU: the two reference models of the linkage clusters (tests/linkage_ref.py) against each other, against hand examples,
against the single-linkage reference (tests/cluster_ref.py) and against scipy.cluster.hierarchy on tie-free matrices."""
import numpy as np
import pytest

import cluster_ref
import linkage_ref as R

LINKAGES = (R.SINGLE, R.COMPLETE, R.AVERAGE)


def both(n, tri, desc, t, linkage):
    a, na = R.literal(n, tri, desc, t, linkage)
    b, nb = R.labels(n, tri, desc, t, linkage)
    assert np.array_equal(a, b) and na == nb, (n, desc, t, linkage)
    assert cluster_ref.is_labelling(a)
    return a, na


@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("seed", range(6))
def test_models_agree_on_random_matrices(seed, linkage):
    """NaN, +-0.0, +-inf, values at and above 2, ties and q at exact halves, both directions, thresholds at values of
    the matrix (so that "equal to t" happens) and between them"""
    n = (5, 9, 13, 17, 20, 24)[seed]
    tri = R.random_tri(n, 100 + seed)
    fin = tri[np.isfinite(tri) & (np.abs(tri) < 2)]
    for desc in (0, 1):
        for t in (0.0, float(np.quantile(fin, 0.2)), float(fin[0]), 0.5, 0.625, float(np.quantile(fin, 0.8)), 1.5, float("nan")):
            both(n, tri, desc, t, linkage)
    if linkage != R.AVERAGE:  # (AVERAGE takes |t| < 2 only)
        for desc in (0, 1):
            for t in (float("inf"), float("-inf"), 2.0):
                both(n, tri, desc, t, linkage)


def test_a_path_under_complete_linkage_pairs_up():
    """consecutive pairs pass, all others fail: every passing merge is a tie, the rule takes (0, 1), then (2, 3), ..."""
    for n in (2, 3, 8, 9):
        lab, nc = both(n, R.path(n), 0, 0.5, R.COMPLETE)
        assert lab.tolist() == [x - x % 2 for x in range(n)] and nc == (n + 1) // 2
        lab, nc = both(n, R.path(n), 0, 0.5, R.SINGLE)
        assert not lab.any() and nc == 1
    # AVERAGE: (0, 1), (2, 3), ... too; {0, 1} with {2, 3} has the mean (0.1 + 3 * 0.9) / 4 = 0.7
    lab, nc = both(8, R.path(8), 0, 0.5, R.AVERAGE)
    assert lab.tolist() == [0, 0, 2, 2, 4, 4, 6, 6]
    lab, nc = both(8, R.path(8), 0, 0.75, R.AVERAGE)
    assert nc < 4


def test_all_values_equal():
    for n in (1, 2, 7, 16):
        tri = np.full(n * (n - 1) // 2, 0.25, np.float32)
        for linkage in LINKAGES:
            for desc, t, one in ((0, 0.25, True), (0, 0.2, False), (1, 0.25, True), (1, 0.3, False)):
                lab, nc = both(n, tri, desc, t, linkage)
                assert nc == (1 if one else n) and (not lab.any() if one else lab.tolist() == list(range(n)))


def test_a_nan_blocks_one_merge():
    """three slots, all close, but (0, 2) is NaN: COMPLETE and AVERAGE merge (0, 1) and then cannot take 2; SINGLE can"""
    tri = np.array([0.1, np.nan, 0.1], np.float32)  # (0,1) (0,2) (1,2)
    assert both(3, tri, 0, 0.5, R.COMPLETE)[0].tolist() == [0, 0, 2]
    assert both(3, tri, 0, 0.5, R.AVERAGE)[0].tolist() == [0, 0, 2]
    assert both(3, tri, 0, 0.5, R.SINGLE)[0].tolist() == [0, 0, 0]
    # a value of 2 blocks AVERAGE alone (and fails the threshold under COMPLETE; passes nothing under SINGLE)
    tri = np.array([0.1, 2.0, 0.1], np.float32)
    assert both(3, tri, 0, 1.9, R.AVERAGE)[0].tolist() == [0, 0, 2]
    assert both(3, tri, 0, 2.0, R.COMPLETE)[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("seed", range(4))
def test_single_equals_the_components_of_the_passing_edges(seed):
    n = 60
    tri = R.random_tri(n, 300 + seed)
    i, j = np.triu_indices(n, 1)
    for desc in (0, 1):
        for t in (0.02, 0.1, 0.9):
            with np.errstate(invalid="ignore"):
                hit = (tri >= np.float32(t)) if desc else (tri <= np.float32(t))
            want, wc = cluster_ref.labels(n, i[hit], j[hit])
            got, gc = R.labels(n, tri, desc, t, R.SINGLE)
            assert np.array_equal(got, want) and gc == wc


@pytest.mark.parametrize("seed", range(4))
def test_refinement_of_single_linkage(seed):
    n = 80
    tri = R.random_tri(n, 400 + seed)
    for desc in (0, 1):
        for t in (0.05, 0.3, 0.7):
            single = R.labels(n, tri, desc, t, R.SINGLE)[0]
            for linkage in (R.COMPLETE, R.AVERAGE):
                lab = R.labels(n, tri, desc, t, linkage)[0]
                assert np.array_equal(single[lab], single)  # x and its label share a single-linkage cluster


@pytest.mark.parametrize("method", ["complete", "average"])
@pytest.mark.parametrize("seed", range(4))
def test_against_scipy(seed, method):
    """tie-free random distances; t in the middle of a gap of scipy's merge heights that is at least 1e-6 wide, so that
    scipy's float means cannot decide differently from the exact rationals"""
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    n = 150
    tri = R.distinct_tri(n, 500 + seed)
    assert np.unique(tri).size == tri.size
    Z = hier.linkage(tri.astype(np.float64), method=method)
    h = Z[:, 2]
    tried = 0
    for frac in (0.2, 0.5, 0.8, 0.95):
        x = int(frac * (h.size - 1))
        while x + 1 < h.size and h[x + 1] - h[x] < 1e-6:
            x += 1
        if x + 1 >= h.size:
            continue
        t = np.float32((h[x] + h[x + 1]) / 2)
        assert h[x] + 4e-7 < t < h[x + 1] - 4e-7
        flat = hier.fcluster(Z, float(t), criterion="distance")
        first = {}
        want = np.array([first.setdefault(c, k) for k, c in enumerate(flat)], np.uint32)
        got, gc = R.labels(n, tri, 0, float(t), R.NAMES[method])
        assert np.array_equal(got, want) and gc == len(first)
        tried += 1
    assert tried >= 3


def test_worst_case_and_block_matrices_are_what_they_claim():
    n = 40
    f = R.funnel(n)
    for linkage in LINKAGES:
        lab, nc = both(24, R.funnel(24), 0, 1.0, linkage)
        assert nc == 1
        cut = R.labels(n, f, 0, 0.25, linkage)[0]  # d(x, y) <= 0.25 iff max(x, y) <= about n / 2: a prefix merges
        k = int((cut == 0).sum())
        assert 2 < k < n and not cut[:k].any() and cut[k:].tolist() == list(range(k, n))
    tri = R.two_blocks(6)
    assert R.labels(12, tri, 0, 0.5, R.SINGLE)[1] == 1
    assert both(12, tri, 0, 0.5, R.COMPLETE)[0].tolist() == [0] * 6 + [6] * 6
    assert both(12, tri, 0, 0.5, R.AVERAGE)[0].tolist() == [0] * 6 + [6] * 6
