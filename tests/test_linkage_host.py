"""CPU: the step logic the linkage kernel compiles (dashing_amd/csrc/linkage.h), built sequentially into libdashing_host.so
as dsh_plan_linkage_labels, against the reference models; the loose threshold of the AVERAGE partition; and the give-up
path -- a step bound that is too small ends with an error code -- which is tested HERE ONLY: no GPU test may try to
reach it."""
import ctypes as C
import os

import numpy as np
import pytest

import linkage_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINKAGES = (R.SINGLE, R.COMPLETE, R.AVERAGE)


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    lib.dsh_plan_linkage_labels.argtypes = [C.c_uint64, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
    lib.dsh_plan_linkage_labels.restype = C.c_int
    lib.dsh_plan_linkage_loose.argtypes = [C.c_float, C.c_int]
    lib.dsh_plan_linkage_loose.restype = C.c_float
    lib.dsh_plan_linkage_q.argtypes = [C.c_float]
    lib.dsh_plan_linkage_q.restype = C.c_int64
    return lib


def run(lib, n, tri, desc, t, linkage, step_cap=None):
    tri = np.ascontiguousarray(tri, np.float32)
    assert tri.size == n * (n - 1) // 2
    out = np.full(max(n, 1), 0xC0DEC0DE, np.uint32)
    nc = C.c_uint64(12345)
    rc = lib.dsh_plan_linkage_labels(n, tri.ctypes.data if tri.size else None, desc, t, linkage, out.ctypes.data, C.byref(nc),
                                     n + 1 if step_cap is None else step_cap)
    return rc, out[:n], int(nc.value)


def check(lib, n, tri, desc, t, linkage, model=R.labels):
    rc, got, gc = run(lib, n, tri, desc, t, linkage)
    want, wc = model(n, tri, desc, t, linkage)
    assert rc == 0 and np.array_equal(got, want) and gc == wc, (n, desc, t, linkage)
    return got


@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("seed", range(6))
def test_equal_to_the_literal_model_on_random_matrices(lib, seed, linkage):
    n = (5, 9, 13, 17, 20, 24)[seed]
    tri = R.random_tri(n, 100 + seed)
    fin = tri[np.isfinite(tri) & (np.abs(tri) < 2)]
    ts = [0.0, float(np.quantile(fin, 0.2)), float(fin[0]), 0.5, 0.625, float(np.quantile(fin, 0.8)), 1.5, float("nan")]
    if linkage != R.AVERAGE:
        ts += [float("inf"), float("-inf"), 2.0]
    for desc in (0, 1):
        for t in ts:
            check(lib, n, tri, desc, t, linkage, R.literal)


@pytest.mark.parametrize("linkage", LINKAGES)
def test_equal_to_the_numpy_model_on_larger_matrices(lib, linkage):
    for n, seed in ((63, 1), (130, 2), (257, 3)):
        tri = R.random_tri(n, 700 + seed)
        for desc in (0, 1):
            for t in (0.05, 0.4, 0.8):
                check(lib, n, tri, desc, t, linkage)
    check(lib, 200, R.funnel(200), 0, 1.0, linkage)
    check(lib, 200, R.funnel(200), 0, 0.25, linkage)
    check(lib, 120, R.two_blocks(60), 0, 0.5, linkage)


def test_hand_examples(lib):
    for n in (1, 2, 3, 8, 9):
        assert check(lib, n, R.path(n), 0, 0.5, R.COMPLETE).tolist() == [x - x % 2 for x in range(n)]
    assert check(lib, 8, R.path(8), 0, 0.5, R.AVERAGE).tolist() == [0, 0, 2, 2, 4, 4, 6, 6]
    nan = np.array([0.1, np.nan, 0.1], np.float32)
    assert check(lib, 3, nan, 0, 0.5, R.COMPLETE).tolist() == [0, 0, 2]
    assert check(lib, 3, nan, 0, 0.5, R.AVERAGE).tolist() == [0, 0, 2]
    assert check(lib, 3, nan, 0, 0.5, R.SINGLE).tolist() == [0, 0, 0]
    for n in (2, 7, 16):
        tri = np.full(n * (n - 1) // 2, 0.25, np.float32)
        for linkage in LINKAGES:
            assert not check(lib, n, tri, 0, 0.25, linkage).any()
            assert check(lib, n, tri, 1, 0.3, linkage).tolist() == list(range(n))
    rc, got, nc = run(lib, 0, np.zeros(0, np.float32), 0, 0.5, R.COMPLETE)
    assert rc == 0 and nc == 0


def test_bad_arguments(lib):
    tri = np.zeros(3, np.float32)
    assert run(lib, 3, tri, 0, 0.5, 3)[0] == -1
    assert run(lib, 3, tri, 0, 0.5, -1)[0] == -1
    assert run(lib, 3, tri, 0, 2.0, R.AVERAGE)[0] == -1
    assert run(lib, 3, tri, 0, -2.0, R.AVERAGE)[0] == -1
    assert run(lib, 3, tri, 0, float("inf"), R.AVERAGE)[0] == -1
    rc, got, nc = run(lib, 3, tri, 0, float("nan"), R.AVERAGE)
    assert rc == 0 and got.tolist() == [0, 1, 2] and nc == 3


def test_q_is_the_rounding_of_group_stats(lib):
    vals = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0**-31, 3 * 2.0**-31, -(2.0**-31), 1.9999999, 1e-9, 0.123456789], np.float32)
    for v in vals:
        assert lib.dsh_plan_linkage_q(float(v)) == int(R.q(v)), v
    assert lib.dsh_plan_linkage_q(float(np.float32(2.0**-31))) == 0 and lib.dsh_plan_linkage_q(float(np.float32(3 * 2.0**-31))) == 2  # half to even


def test_loose_threshold(lib):
    """t' passes -- q(t') is on the right side of Q -- and its float32 neighbour on the worse side does not; t itself is
    never worse than t'"""
    ts = [1e-9, 2.0**-31, 3 * 2.0**-31, 2.0**-30, 5e-9, 1e-7, 1e-5, 1e-3, 2.0**-7, 0.015624999, 0.1, 0.5, 1.0, 1.5, 1.99, 1.9999999]
    ts += list(np.random.default_rng(3).random(200).astype(np.float32) * 2.0 ** -np.random.default_rng(4).integers(0, 30, 200))
    ts += [0.0] + [-float(t) for t in ts[:16]]
    for t in ts:
        t = np.float32(t)
        Q = int(R.q(t))
        for desc in (0, 1):
            lo = np.float32(lib.dsh_plan_linkage_loose(float(t), desc))
            worse = np.nextafter(lo, np.float32(-np.inf) if desc else np.float32(np.inf))
            if desc:
                assert int(R.q(lo)) >= Q > int(R.q(worse)) and lo <= t, (t, lo)
            else:
                assert int(R.q(lo)) <= Q < int(R.q(worse)) and lo >= t, (t, lo)


def test_step_cap_gives_up_with_an_error(lib):
    """a chain of 10 nodes takes 9 merges under SINGLE linkage and 5 under the other two: a bound of 2 steps ends with the
    step code (1), a bound that the merges fit does not"""
    tri = R.path(10)
    for linkage in LINKAGES:
        rc, got, nc = run(lib, 10, tri, 0, 0.5, linkage)  # the bound every caller passes (m + 1) is never met
        assert rc == 0
        assert run(lib, 10, tri, 0, 0.5, linkage, step_cap=2)[0] == 1
    rc, got, nc = run(lib, 10, tri, 0, 0.5, R.SINGLE, step_cap=9)
    assert rc == 0 and not got.any() and nc == 1
    assert run(lib, 10, tri, 0, 0.5, R.SINGLE, step_cap=8)[0] == 1
    assert run(lib, 10, tri, 0, 0.5, R.COMPLETE, step_cap=5)[0] == 0  # (0,1) (2,3) (4,5) (6,7) (8,9), then nothing passes
