"""The planner of dsh_union_curve* (csrc/curve_plan.h, through dshh_curve_plan of csrc/host/plan_capi.cpp): the segments
tile an order, a forced segment length is respected, the planner's own is never below min(len, 64), a batch holds at
least one order and stays within the scratch budget wherever one order fits it."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (0, 1, 63, 64, 65, 10_000, 100_000)
MIB = 1 << 20


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    lib.dshh_curve_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.dshh_curve_plan.restype = C.c_int
    return lib


def plan(host, n_orders, length, p, budget=256 * MIB, forced=0):
    info = np.zeros(5, np.uint64)
    assert host.dshh_curve_plan(n_orders, length, p, budget, forced, info.ctypes.data, None, 0) == 0
    S, nseg, batch, order_bytes, scratch = (int(x) for x in info)
    bounds = np.zeros(nseg + 1, np.uint64)
    assert host.dshh_curve_plan(n_orders, length, p, budget, forced, info.ctypes.data, bounds.ctypes.data, nseg + 1) == 0
    if nseg:
        assert host.dshh_curve_plan(n_orders, length, p, budget, forced, info.ctypes.data, bounds.ctypes.data, nseg) == -2
    return S, nseg, batch, order_bytes, scratch, bounds.astype(np.int64)


def order_bytes_model(length, p, nseg):
    nchunk = -(-length // 128)
    return length * 256 + length * 64 * (2 if p <= 15 else 4) + ((nseg << p) if nseg > 1 else 0) + (nchunk * 256 if nchunk > 1 else 0)


@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("p", (4, 10, 14, 18))
def test_segments_tile_the_order(host, length, p):
    for n_orders in (1, 3, 100):
        for forced in (0, 1, 2, 5, 64, 1000, 10**9):
            if forced == 1 and length > 10_000:
                continue
            S, nseg, batch, ob, scratch, b = plan(host, n_orders, length, p, forced=forced)
            assert nseg == -(-length // S) and b[0] == 0 and b[-1] == length
            lens = np.diff(b)
            assert (lens > 0).all() and (lens[:-1] == S).all() and (lens <= S).all()
            if forced:
                assert S == min(forced, max(length, 1))
            else:
                assert S >= min(length, 64)
            assert 1 <= batch <= n_orders
            assert ob == order_bytes_model(length, p, nseg) and scratch == batch * ob


def test_the_batch_respects_the_budget(host):
    for p in (10, 14, 18):
        for length in (1, 65, 10_000):
            for n_orders in (1, 17, 1000):
                one = order_bytes_model(length, p, -(-length // 64))  # (no plan needs more per order than segments of 64)
                for budget in (1, one // 2, one, 3 * one + 5, 64 * MIB, 1 << 40):
                    S, nseg, batch, ob, scratch, _ = plan(host, n_orders, length, p, budget=budget)
                    assert batch >= 1
                    if ob <= budget:
                        assert scratch <= budget
                    else:
                        assert batch == 1
    # a budget of 3.x orders holds three
    ob = order_bytes_model(37, 10, 1)
    assert plan(host, 17, 37, 10, budget=3 * ob + 5, forced=37)[2] == 3


def test_one_long_order_is_cut_to_fill_the_device(host):
    # 100 000 rows of 1 KiB: about 2048 workgroups of four units each, no segment below 64 members
    S, nseg, batch, *_ = plan(host, 1, 100_000, 10)
    assert S >= 64 and 1024 <= nseg <= 8192 and batch == 1
    # a hundred orders at p = 14 fill it on their own
    S, nseg, *_ = plan(host, 100, 10_000, 14, budget=1 << 40)
    assert nseg <= 8 and S >= 64


def test_arguments(host):
    info = np.zeros(5, np.uint64)
    assert host.dshh_curve_plan(1, 1, 3, 1, 0, info.ctypes.data, None, 0) == -1
    assert host.dshh_curve_plan(1, 1, 10, 1, 0, None, None, 0) == -1
