"""CPU: the step logic the MST kernels compile (dashing_amd/csrc/mst.h), built sequentially into libdashing_host.so as
dsh_plan_mst, against the literal model (tests/mst_ref.py: kruskal); dsh_mst_linkage, which is pure host; and the give-up
path -- a round bound that is too small ends with an error code -- which is tested HERE ONLY: no GPU test may try to reach
it."""
import ctypes as C
import os

import numpy as np
import pytest

import dashing_amd
import mst_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS_CODE = 3  # kMstErrRounds


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    vp = C.c_void_p
    lib.dsh_plan_mst.argtypes = [C.c_uint64, vp, C.c_int, C.c_float, C.c_uint32, vp, vp, vp, C.POINTER(C.c_uint64), vp, C.POINTER(C.c_uint32)]
    lib.dsh_plan_mst.restype = C.c_int
    return lib


def run(lib, n, tri, desc, cutoff, round_cap=34):
    tri = np.ascontiguousarray(tri, np.float32)
    assert tri.size == R.span(n)
    m = max(n - 1, 1)
    lhs, rhs, val = np.full(m, 0xC0DEC0DE, np.uint32), np.full(m, 0xC0DEC0DE, np.uint32), np.full(m, 7.0, np.float32)
    lab = np.full(max(n, 1), 0xC0DEC0DE, np.uint32)
    ne, rounds = C.c_uint64(12345), C.c_uint32(99)
    rc = lib.dsh_plan_mst(n, tri.ctypes.data if tri.size else None, desc, cutoff, round_cap, lhs.ctypes.data, rhs.ctypes.data, val.ctypes.data,
                          C.byref(ne), lab.ctypes.data, C.byref(rounds))
    e = int(ne.value)
    return rc, (lhs[:e], rhs[:e], val[:e], lab[:n]), int(rounds.value)


def check(lib, n, tri, desc, cutoff):
    rc, got, rounds = run(lib, n, tri, desc, cutoff)
    want = R.kruskal(n, tri, desc, cutoff)
    assert rc == 0, (n, desc, cutoff)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (n, desc, cutoff)
    assert rounds <= max(n, 1).bit_length()
    return got, rounds


@pytest.mark.parametrize("name,n,tri", R.families(), ids=[f[0] for f in R.families()])
def test_equal_to_kruskal(lib, name, n, tri):
    for desc in (0, 1):
        for cut in R.cutoffs(tri, desc):
            check(lib, n, tri, desc, cut)


def test_all_equal_values_give_the_star(lib):
    for desc in (0, 1):
        (lhs, rhs, val, lab), rounds = check(lib, 50, R.all_equal(50), desc, R.no_cutoff(desc))
        assert lhs.tolist() == [0] * 49 and rhs.tolist() == list(range(1, 50)) and not lab.any() and rounds == 1


def test_nothing_passes(lib):
    for n in (0, 1, 2, 3, 20):
        (lhs, rhs, val, lab), rounds = check(lib, n, R.all_nan(n), 0, np.inf)
        assert lhs.size == 0 and lab.tolist() == list(range(n)) and rounds == 0
    assert check(lib, 9, R.tie_free(9, 3), 1, 2.0)[0][0].size == 0


def test_zero_is_reported_positive(lib):
    (lhs, rhs, val, lab), _ = check(lib, 3, np.array([-0.0, np.nan, 0.0], np.float32), 1, -np.inf)
    assert (lhs.tolist(), rhs.tolist()) == ([0, 1], [1, 2]) and val.view(np.uint32).tolist() == [0, 0]


def test_the_ultrametric_matrix_takes_exactly_eight_rounds(lib):
    for desc in (0, 1):
        tri = R.ultrametric(256, desc)
        (lhs, rhs, val, lab), rounds = check(lib, 256, tri, desc, R.no_cutoff(desc))
        assert rounds == 8 and lhs.size == 255


def test_round_cap_gives_up_with_an_error(lib):
    tri = R.ultrametric(256, 0)
    assert run(lib, 256, tri, 0, np.inf, round_cap=2)[0] == ROUNDS_CODE
    assert run(lib, 256, tri, 0, np.inf, round_cap=7)[0] == ROUNDS_CODE
    assert run(lib, 256, tri, 0, np.inf, round_cap=8)[0] == 0


def test_bad_arguments(lib):
    ne, rounds = C.c_uint64(), C.c_uint32()
    assert lib.dsh_plan_mst(3, None, 0, 0.5, 34, None, None, None, C.byref(ne), None, C.byref(rounds)) == -1


def test_mst_linkage_against_the_model(lib):
    for name, n, tri in R.families():
        for desc in (0, 1):
            lhs, rhs, val, _ = R.kruskal(n, tri, desc, R.no_cutoff(desc))
            za, zb, zv, zs = dashing_amd.mst_linkage(n, lhs, rhs, val)
            wa, wb, ws = R.linkage(n, lhs, rhs)
            assert np.array_equal(za, wa) and np.array_equal(zb, wb) and np.array_equal(zs, ws), name
            assert np.array_equal(zv.view(np.uint32), val.view(np.uint32)) and np.all(za < zb)
    za, zb, zv, zs = dashing_amd.mst_linkage(4, [2, 0, 0], [3, 1, 2], [0.1, 0.2, 0.3])
    assert (za.tolist(), zb.tolist(), zs.tolist()) == ([2, 0, 4], [3, 1, 5], [2, 2, 4])


def test_mst_linkage_refuses_what_is_not_a_forest():
    for lhs, rhs in (([0, 1, 0], [1, 2, 2]), ([0, 0], [1, 1]), ([0], [4]), ([5], [1]), ([1], [1])):
        with pytest.raises(dashing_amd.DshError) as e:
            dashing_amd.mst_linkage(4, lhs, rhs, np.zeros(len(lhs), np.float32))
        assert e.value.code == -22
    assert dashing_amd.mst_linkage(0, [], [], [])[0].size == 0 and dashing_amd.mst_linkage(3, [], [], [])[0].size == 0
