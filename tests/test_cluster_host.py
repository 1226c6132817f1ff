"""CPU: the union-find the device kernels compile (dashing_amd/csrc/uf.h), built sequentially into libdashing_host.so as
dsh_plan_uf_labels, against the numpy reference; and its give-up path -- a step bound that is too small ends with an
error code, not a loop -- which is tested HERE ONLY: no GPU test may try to reach it."""
import ctypes as C
import os

import numpy as np
import pytest

import cluster_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def uf():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    lib.dsh_plan_uf_labels.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    lib.dsh_plan_uf_labels.restype = C.c_int

    def run(n, lhs, rhs, step_cap=None):
        lhs = np.ascontiguousarray(lhs, np.uint32)
        rhs = np.ascontiguousarray(rhs, np.uint32)
        out = np.full(max(n, 1), 0xC0DEC0DE, np.uint32)
        rc = lib.dsh_plan_uf_labels(n, lhs.ctypes.data, rhs.ctypes.data, lhs.size, n + 1 if step_cap is None else step_cap, out.ctypes.data)
        return rc, out[:n]

    return run


def test_equal_to_the_reference(uf):
    for name, n, lhs, rhs in cluster_ref.small_graphs():
        rc, got = uf(n, lhs, rhs)
        assert rc == 0, name
        assert np.array_equal(got, cluster_ref.labels(n, lhs, rhs)[0]), name


def test_larger_graphs_and_edge_orders(uf):
    rng = np.random.default_rng(5)
    n = 5000
    a, b = cluster_ref.chain(n)
    perm = rng.permutation(a.size)
    for lhs, rhs in ((a, b), (b[::-1], a[::-1]), (a[perm], b[perm])):
        rc, got = uf(n, lhs, rhs)
        assert rc == 0 and not got.any()
    for m in (n // 4, n // 2, n, 4 * n):
        lhs, rhs = cluster_ref.random_graph(n, m, m)
        rc, got = uf(n, lhs, rhs)
        assert rc == 0 and np.array_equal(got, cluster_ref.labels(n, lhs, rhs)[0])


def test_an_edge_out_of_range_is_refused(uf):
    assert uf(4, [1], [4])[0] == -1


def test_step_cap_gives_up_with_an_error(uf):
    """a chain of 10 nodes whose first four edges arrive descending -- every hook puts a root under a smaller root and no
    find meets a path it could shorten, so node 4 ends 4 links deep -- and whose fifth edge starts at node 4"""
    lhs = np.array([3, 2, 1, 0, 4, 5, 6, 7, 8], np.uint32)
    rhs = np.array([4, 3, 2, 1, 5, 6, 7, 8, 9], np.uint32)
    assert sorted(zip(lhs.tolist(), rhs.tolist())) == [(i, i + 1) for i in range(9)]
    rc, got = uf(10, lhs, rhs)  # the bound every caller passes (n + 1) is never met
    assert rc == 0 and got.tolist() == [0] * 10
    rc, got = uf(10, lhs, rhs, step_cap=4)
    assert rc == 0 and got.tolist() == [0] * 10
    rc, _ = uf(10, lhs, rhs, step_cap=2)
    assert rc == 1  # kUfErrFind: the find of node 4 gave up after 2 of its 4 links
