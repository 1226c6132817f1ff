"""The two references of the greedy representatives (tests/greedy_ref.py) held to each other and to the consequences the
header states, on the small graphs of tests/cluster_ref.py and on random graphs."""
import numpy as np
import pytest

import cluster_ref
import greedy_ref


def graphs():
    out = [(name, n, lhs, rhs) for name, n, lhs, rhs in cluster_ref.small_graphs()]
    for s in range(6):
        for n, m in ((30, 20), (90, 200), (200, 150), (200, 600), (200, 4000)):
            out.append(("random n=%d m=%d seed=%d" % (n, m, s), n) + cluster_ref.random_graph(n, m, 7000 + 10 * m + s))
    return out


@pytest.mark.parametrize("g", range(len(graphs())))
def test_sequential_pass_equals_the_definition_and_its_consequences(g):
    name, n, lhs, rhs = graphs()[g]
    rp, col = greedy_ref.csr_of_edges(n, lhs, rhs)
    h = greedy_ref.hit_matrix(n, rp, col)
    lab, nr = greedy_ref.labels(n, rp, col)
    want, wr = greedy_ref.labels_from_definition(n, h)
    assert lab.dtype == np.uint32 and np.array_equal(lab, want) and nr == wr, name
    l = lab.astype(np.int64)
    x = np.arange(n)
    assert (l <= x).all() and (l[l] == l).all()  # labels[x] <= x; idempotence
    reps = np.flatnonzero(l == x)
    assert nr == reps.size
    assert not h[np.ix_(reps, reps)].any()  # independence: no two representatives hit each other
    cov = np.flatnonzero(l != x)
    assert h[l[cov], cov].all()  # coverage: every other slot hits its label
    for m in sorted({0, 1, n // 3, n // 2, max(n - 1, 0)}):  # prefix property
        if m <= n:
            sub, _ = greedy_ref.labels_from_definition(m, h[:m, :m])
            assert np.array_equal(sub, lab[:m]), (name, m)
    # every greedy cluster lies inside one component
    comp, nc = cluster_ref.labels(n, lhs, rhs)
    assert np.array_equal(comp[l], comp) and nr >= nc


def test_path_of_three_chains_but_is_not_covered():
    rp, col = greedy_ref.csr_of_edges(3, [0, 1], [1, 2])
    assert cluster_ref.labels(3, [0, 1], [1, 2])[0].tolist() == [0, 0, 0]
    assert greedy_ref.labels(3, rp, col)[0].tolist() == [0, 0, 2]
    assert greedy_ref.labels_from_definition(3, greedy_ref.hit_matrix(3, rp, col))[0].tolist() == [0, 0, 2]
    # the smallest representative, not the first hit in any other order: 3 is hit by the representatives 0 and 2
    rp, col = greedy_ref.csr_of_edges(4, [2, 0, 0], [3, 3, 1])
    lab, nr = greedy_ref.labels(4, rp, col)
    assert lab.tolist() == [0, 0, 2, 0] and nr == 2
