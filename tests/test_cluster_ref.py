"""CPU: the numpy reference of the threshold clusters (tests/cluster_ref.py) on hand cases, against a second, independent
formulation (label propagation to a fixed point), and the invariance of the label definition under edge order."""
import numpy as np

import cluster_ref


def propagate(n, lhs, rhs):
    """min-label propagation until nothing changes: the definition itself, with no union-find"""
    lab = np.arange(n, dtype=np.int64)
    lhs, rhs = np.asarray(lhs, np.int64), np.asarray(rhs, np.int64)
    while True:
        new = lab.copy()
        np.minimum.at(new, lhs, lab[rhs])
        np.minimum.at(new, rhs, lab[lhs])
        if np.array_equal(new, lab):
            return lab.astype(np.uint32)
        lab = new


def test_hand_cases():
    u = lambda *a: np.array(a, np.uint32)
    lab, nc = cluster_ref.labels(6, u(4, 1), u(5, 3))
    assert lab.tolist() == [0, 1, 2, 1, 4, 4] and nc == 4
    lab, nc = cluster_ref.labels(6, u(4, 1, 5, 2), u(5, 3, 3, 2))
    assert lab.tolist() == [0, 1, 2, 1, 1, 1] and nc == 3
    lab, nc = cluster_ref.labels(0, u(), u())
    assert lab.size == 0 and lab.dtype == np.uint32 and nc == 0
    lab, nc = cluster_ref.labels(1, u(0), u(0))
    assert lab.tolist() == [0] and nc == 1
    lab, nc = cluster_ref.labels(10, *cluster_ref.chain(10))
    assert lab.tolist() == [0] * 10 and nc == 1
    lab, nc = cluster_ref.labels(9, *cluster_ref.star(9, 8))
    assert lab.tolist() == [0] * 9 and nc == 1
    l, r, (jl, jr) = cluster_ref.two_cliques(6)
    assert cluster_ref.labels(12, l, r)[0].tolist() == [0] * 6 + [6] * 6
    assert cluster_ref.labels(12, np.concatenate([l, jl]), np.concatenate([r, jr])) [0].tolist() == [0] * 12


def test_labels_in_continues_an_earlier_labelling():
    u = lambda *a: np.array(a, np.uint32)
    first, _ = cluster_ref.labels(6, u(4), u(5))
    lab, nc = cluster_ref.labels(6, u(1), u(3), labels_in=first)
    assert lab.tolist() == [0, 1, 2, 1, 4, 4] and nc == 4
    # labels_in need not be a labelling in normal form: any node of the same set serves
    lab, nc = cluster_ref.labels(4, u(), u(), labels_in=u(3, 1, 2, 3))
    assert lab.tolist() == [0, 1, 2, 0] and nc == 3


def test_csr_edges():
    lhs, rhs = cluster_ref.csr_edges(np.array([0, 2, 2, 3], np.uint64), np.array([5, 6, 7], np.uint32), row_begin=2)
    assert lhs.tolist() == [2, 2, 4] and rhs.tolist() == [5, 6, 7]


def test_equal_to_label_propagation_and_order_free():
    rng = np.random.default_rng(11)
    for name, n, lhs, rhs in cluster_ref.small_graphs():
        want = propagate(n, lhs, rhs)
        got, nc = cluster_ref.labels(n, lhs, rhs)
        assert got.dtype == np.uint32 and np.array_equal(got, want), name
        assert nc == np.unique(want).size and cluster_ref.is_labelling(got), name
        for _ in range(3):  # any order of the edges, either orientation of each
            perm = rng.permutation(lhs.size)
            flip = rng.integers(0, 2, lhs.size).astype(bool)
            a, b = np.where(flip, rhs, lhs)[perm], np.where(flip, lhs, rhs)[perm]
            assert np.array_equal(cluster_ref.labels(n, a, b)[0], want), name


def test_fast_form_equals_the_plain_one():
    for name, n, lhs, rhs in cluster_ref.small_graphs():
        a, b = cluster_ref.labels(n, lhs, rhs), cluster_ref.labels_fast(n, lhs, rhs)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and b[0].dtype == np.uint32, name
    rng = np.random.default_rng(2)
    n = 20_000
    lhs, rhs = cluster_ref.chain(n)
    perm = rng.permutation(lhs.size)
    assert not cluster_ref.labels_fast(n, lhs[perm], rhs[perm])[0].any()
    for m in (n // 4, n // 2, n, 4 * n):
        lhs, rhs = cluster_ref.random_graph(n, m, m + 1)
        a, b = cluster_ref.labels(n, lhs, rhs), cluster_ref.labels_fast(n, lhs, rhs)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        first = cluster_ref.labels(n, lhs[: m // 2], rhs[: m // 2])[0]
        assert np.array_equal(cluster_ref.labels_fast(n, lhs[m // 2 :], rhs[m // 2 :], labels_in=first)[0], a[0])
