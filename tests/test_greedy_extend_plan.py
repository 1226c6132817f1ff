"""The old-row bands of dsh_greedy_extend* (plan::greedy_old_band, through dshh_greedy_extend_bands of
csrc/host/plan_capi.cpp): the rectangle rule of dsh_dist_rect_threshold -- at most band_bytes of float32 (one row at
least), at most 2^20 rows -- on the rows that have something to say: a band starts and ends at a representative and a
stretch without one is not computed."""
import ctypes as C
import os

import numpy as np
import pytest

import greedy_extend_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    lib.dshh_greedy_extend_bands.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.dshh_greedy_extend_bands.restype = C.c_int64
    return lib


def bands(host, labels_in, n, band_bytes):
    li = np.ascontiguousarray(labels_in, np.uint32)
    out = np.zeros(2 * li.size + 2, np.uint64)
    nb = host.dshh_greedy_extend_bands(li.ctypes.data if li.size else None, li.size, n, band_bytes, out.ctypes.data, out.size)
    assert nb >= 0
    return out[: 2 * nb].astype(np.int64).reshape(nb, 2)


def check(host, labels_in, n, band_bytes):
    li = np.asarray(labels_in, np.int64)
    m = li.size
    b = bands(host, li, n, band_bytes)
    what = (m, n, band_bytes)
    reps = np.flatnonzero(li == np.arange(m))
    if reps.size == 0:
        assert b.shape[0] == 0, what
        return b
    assert (b[:, 0] < b[:, 1]).all() and (b[1:, 0] >= b[:-1, 1]).all() and b[-1, 1] <= m, what  # in order, disjoint
    inside = np.concatenate([np.arange(lo, hi) for lo, hi in b])
    assert np.array_equal(np.intersect1d(inside, reps), reps), what  # every representative, once (the bands are disjoint)
    assert (li[b[:, 0]] == b[:, 0]).all() and (li[b[:, 1] - 1] == b[:, 1] - 1).all(), what  # from one to one: no band without
    max_rows = min(max(max(band_bytes // 4, 1) // max(n - m, 1), 1), 1 << 20)
    assert (b[:, 1] - b[:, 0] <= max_rows).all(), what  # the byte budget (one row at least)
    # greedy: the next band's first representative did not fit the band before it
    assert (b[1:, 0] - b[:-1, 0] >= max_rows).all(), what
    return b


def test_bands_hold_every_old_representative_once_within_the_budget(host):
    rng = np.random.default_rng(0x01DBA2D)
    for m in (1, 2, 77, 128, 1000, 5000):
        for extra in (0, 1, 300, 10_000):
            n = m + extra
            for p_rep in (0.02, 0.4, 1.0):
                li = X.random_labelling(m, rng, p_rep)
                for band_bytes in (4, 1000, 64 << 10, 1 << 20, 1 << 30):
                    check(host, li, n, band_bytes)


def test_edge_cases(host):
    # m = 0: nothing to do
    assert bands(host, [], 100, 1 << 30).shape[0] == 0
    # no representative at all (not a valid labelling -- the entry points refuse it -- but the rule is a pure function)
    assert bands(host, np.full(50, 0xFFFFFFFF, np.uint32), 100, 1 << 30).shape[0] == 0
    # representatives only at 0 and m - 1
    m, n = 1000, 1100
    li = np.zeros(m, np.uint32)
    li[m - 1] = m - 1
    assert check(host, li, n, 1 << 30).tolist() == [[0, m]]  # one band holds both
    assert check(host, li, n, 400 * 100).tolist() == [[0, 1], [m - 1, m]]  # 100 rows per band: the stretch between is skipped
    assert check(host, li, n, 4).tolist() == [[0, 1], [m - 1, m]]
    # m > n is refused
    out = np.zeros(8, np.uint64)
    assert host.dshh_greedy_extend_bands(li.ctypes.data, m, m - 1, 1 << 30, out.ctypes.data, out.size) == -1
