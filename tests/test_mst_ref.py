"""CPU: the two reference models of the minimum spanning tree (tests/mst_ref.py) against each other on every matrix family,
and -- on tie-free matrices, where any correct algorithm must agree -- against scipy where it imports."""
import numpy as np
import pytest

import mst_ref as R


def same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_prim_equals_kruskal_on_every_family():
    fams = R.families() + [("ultra-d", 64, R.ultrametric(64, 0)), ("ultra-s", 64, R.ultrametric(64, 1))]
    for name, n, tri in fams:
        for desc in (0, 1):
            for cut in R.cutoffs(tri, desc):
                k, p = R.kruskal(n, tri, desc, cut), R.prim(n, tri, desc, cut)
                assert same(k, p), (name, desc, cut)
                assert len(k[0]) == n - len(np.unique(k[3])) and np.all(k[0] < k[1])


def test_hand_examples():
    lhs, rhs, val, lab = R.kruskal(50, R.all_equal(50), 0, np.inf)
    assert lhs.tolist() == [0] * 49 and rhs.tolist() == list(range(1, 50)) and not lab.any()
    lhs, rhs, val, lab = R.kruskal(3, np.array([-0.0, np.nan, 0.0], np.float32), 1, -np.inf)
    assert (lhs.tolist(), rhs.tolist()) == ([0, 1], [1, 2]) and val.view(np.uint32).tolist() == [0, 0]
    assert R.kruskal(4, R.tie_free(4, 1), 0, np.nan)[3].tolist() == [0, 1, 2, 3]
    za, zb, zs = R.linkage(4, [2, 0, 0], [3, 1, 2])
    assert (za.tolist(), zb.tolist(), zs.tolist()) == ([2, 0, 4], [3, 1, 5], [2, 2, 4])


@pytest.mark.parametrize("n,seed", [(12, 1), (60, 2), (150, 3)])
def test_tie_free_matrices_against_scipy(n, seed):
    pytest.importorskip("scipy")
    from scipy.cluster.hierarchy import linkage
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree

    tri = R.tie_free(n, seed)
    lhs, rhs, val, lab = R.kruskal(n, tri, 0, np.inf)
    iu, ju = np.triu_indices(n, 1)
    t = minimum_spanning_tree(csr_matrix((tri.astype(np.float64), (iu, ju)), shape=(n, n))).tocoo()
    assert sorted(zip(t.row.tolist(), t.col.tolist())) == sorted(zip(lhs.tolist(), rhs.tolist()))
    Z = linkage(tri.astype(np.float64), method="single")
    za, zb, zs = R.linkage(n, lhs, rhs)
    assert np.array_equal(np.minimum(Z[:, 0], Z[:, 1]), za) and np.array_equal(np.maximum(Z[:, 0], Z[:, 1]), zb)
    assert np.array_equal(Z[:, 2], val.astype(np.float64)) and np.array_equal(Z[:, 3], zs)
