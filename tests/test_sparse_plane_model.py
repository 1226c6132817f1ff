"""CPU: the sparse outer planes of the compare path (dashing_amd/csrc/plan.h, Tuning::sparse_planes).

The top plane of a tile, C(T) = #{t : a_t < T and b_t < T}, is counted from the complement sets U = {t : a_t >= T} as
m - |U_i| - |U_j| + |U_i & U_j| (kernels_sparseplane.hip).  Here: the numpy statement of that route
(tools/path_census.py, sparse_plane_counts: sets, the column block's table, the formula) against popcount(A_v & B_v), and
the planner's side through dshh_plan_check_sparse (csrc/host/plan_capi.cpp), which builds layout and plan as engine.hip
does and checks that every (tile, plane) is in exactly one route, that a routed plane's sets fit the cap for every sketch
of its two blocks, and that rounds and fragments are planned on the dense remainder."""
import ctypes as C
import os

import numpy as np
import pytest

import sparse_cases as sc
from sparse_cases import pcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dense_counts(rows, cols, v):
    """popcount(A_v & B_v): the tile kernel's statement"""
    a, b = np.asarray(rows) < v, np.asarray(cols) < v
    return (a[:, None, :] & b[None, :, :]).sum(axis=2)


def test_route_equals_and_popcount_hand_made():
    rows = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [7, 7, 7, 7, 7, 7, 7, 7], [0, 0, 0, 0, 0, 0, 0, 0], [3, 3, 4, 4, 3, 3, 4, 4]], np.uint8)
    cols = np.array([[7, 6, 5, 4, 3, 2, 1, 0], [4, 4, 4, 4, 4, 4, 4, 4], [0, 9, 0, 9, 0, 9, 0, 9]], np.uint8)
    for v in range(0, 11):
        got = pcs.sparse_plane_counts(rows, cols, v)
        assert (got == dense_counts(rows, cols, v)).all(), v
    # the extremes: every set empty (C = m), every set full (C = 0)
    assert (pcs.sparse_plane_counts(rows, cols, 10) == 8).all() and (pcs.sparse_plane_counts(rows, cols, 0) == 0).all()


@pytest.mark.parametrize("p", (6, 9, 13))
def test_route_equals_and_popcount_random(p):
    rng = np.random.default_rng(p)
    m = 1 << p
    rows = rng.integers(0, 12, (9, m)).astype(np.uint8)
    cols = rng.integers(0, 12, (7, m)).astype(np.uint8)
    cols[0] = rows[0]  # the intersection is the whole set
    cols[1] = 0        # an empty set at every v > 0
    for v in (1, 5, 10, 11, 12):
        assert (pcs.sparse_plane_counts(rows, cols, v) == dense_counts(rows, cols, v)).all(), v


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    u64, i32, u32, vp = C.c_uint64, C.c_int, C.c_uint32, C.c_void_p
    lib.dshh_plan_check_sparse.argtypes = [u64, vp, vp, i32, i32, u64, u64, u32, i32, i32, u64, u32, i32, u32, vp, vp, u64, C.c_char_p, C.c_size_t]
    lib.dshh_plan_check_ri.argtypes = [u64, vp, i32, i32, u64, u64, u64, u64, u32, i32, i32, u64, i32, i32, i32, u32, vp, C.c_char_p, C.c_size_t]
    return lib


NAMES = ("tiles", "bands", "items", "parts", "planes_x100", "npad", "P", "rounds", "frags", "round", "sparse_items", "slabs")


def plan(host, keys, gcnt, p, sparse_planes, sparse_cap=pcs.SPARSE_CAP, rb=0, re=None, nparts=1, want_parts=0, budget=8 << 30, round_items=768):
    n = len(keys)
    stats = np.zeros(12, np.uint64)
    nt = (n + 127) // 128
    routes = np.zeros((nt * (nt + 1) // 2, 5), np.uint32)
    err = C.create_string_buffer(512)
    rc = host.dshh_plan_check_sparse(n, keys.ctypes.data, None if gcnt is None else gcnt.ctypes.data, 0, 1, rb, n if re is None else re, nparts,
                                     want_parts, p, budget, round_items, sparse_planes, sparse_cap, stats.ctypes.data, routes.ctypes.data,
                                     len(routes), err, 512)
    assert rc == 0, err.value.decode()
    st = dict(zip(NAMES, (int(x) for x in stats)))
    return st, routes[: st["tiles"]]


def parent_plan(host, keys, p, round_items=768, budget=8 << 30):
    n = len(keys)
    stats = np.zeros(10, np.uint64)
    err = C.create_string_buffer(512)
    rc = host.dshh_plan_check_ri(n, keys.ctypes.data, 0, 1, 0, n, 0, 0, 1, 0, p, budget, 1, 0, 64, round_items, stats.ctypes.data, err, 512)
    assert rc == 0, err.value.decode()
    return dict(zip(NAMES[:10], (int(x) for x in stats)))


_cache = {}


def case(kind, n, p):
    if (kind, n, p) not in _cache:
        regs, cap = sc.collection(kind, n, p)
        _cache[(kind, n, p)] = (regs, cap, *sc.keys_and_counts(regs, p))
    return _cache[(kind, n, p)]


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("n,p", ((131, 13), (257, 14), (257, 16)))
def test_every_plane_in_exactly_one_route(host, kind, n, p):
    """dshh_plan_check_sparse holds the plan to its contract; its routes are the model's, tile by tile"""
    regs, cap, keys, gcnt = case(kind, n, p)
    cap = pcs.SPARSE_CAP if cap is None else cap
    off = parent_plan(host, keys, p)
    for k in (1, 2):
        st, routes = plan(host, keys, gcnt, p, k, cap)
        c = pcs.census(regs, p, sparse_planes=k, sparse_cap=cap)
        model = {(t["bi"], t["bj"]): (t["planes"], t["sparse"]) for t in c.tiles}
        got = {(int(r[0]), int(r[1])): (int(r[3] - r[2]), int(r[4])) for r in routes}
        assert got == model, (kind, k)
        assert st["sparse_items"] == c.plan["sparse_items"] and st["tiles"] == off["tiles"] and st["planes_x100"] == off["planes_x100"]
        # the tile kernel's items are planned on what remains: whole planes, or fragments of the last ones
        dense = c.plan["dense_planes"]
        assert st["items"] - st["frags"] <= dense <= st["items"], (st, dense)
        if kind == "constant":
            assert st["sparse_items"] == 0
        if kind in ("survey", "near_duplicates"):
            assert st["sparse_items"] == k * st["tiles"], st  # every tile's top planes go
    # without the counts, or with the route off, the plan is the parent's
    for st in (plan(host, keys, None, p, 2, cap)[0], plan(host, keys, gcnt, p, 0, cap)[0]):
        assert st["sparse_items"] == 0 and st["slabs"] == 0
        assert {x: st[x] for x in off} == off


@pytest.mark.parametrize("n,p", ((131, 13), (257, 14)))
def test_a_block_one_above_the_cap_stays_dense(host, n, p):
    regs, cap, odd = sc.cap_boundary(n, p, 0x5A0000 + 131 * p + n)
    keys, gcnt = sc.keys_and_counts(regs, p)
    st, routes = plan(host, keys, gcnt, p, 1, cap)
    c = pcs.census(regs, p, sparse_planes=1, sparse_cap=cap)
    odd_block = next(b for b, blk in enumerate(c.blocks) if odd in blk["cols"])
    assert 0 < st["sparse_items"] < st["tiles"]
    for r in routes:
        assert int(r[4]) == (0 if odd_block in (int(r[0]), int(r[1])) else 1), r
    # one more in the cap and everything goes; one less and nothing does
    assert plan(host, keys, gcnt, p, 1, cap + 1)[0]["sparse_items"] == st["tiles"]
    assert plan(host, keys, gcnt, p, 1, cap - 1)[0]["sparse_items"] == 0


def test_automatic_rule(host):
    """p >= 13 and a band of more than 512 planes; the rounds shrink with the planes that leave"""
    from dashing_amd import synth

    p = 14
    regs = synth.survey_sketches(1400, p, seed=0x5A1400)[0]
    keys, gcnt = sc.keys_and_counts(regs, p)
    off = parent_plan(host, keys, p)
    auto, _ = plan(host, keys, gcnt, p, -1)
    assert auto["sparse_items"] == pcs.SPARSE_AUTO_PLANES * auto["tiles"] and auto["items"] < off["items"] and auto["rounds"] <= off["rounds"]
    # a small band keeps its planes (300 sketches: 6 tiles), and so does p = 12 at any size
    small, _ = plan(host, keys[:300].copy(), gcnt[:300].copy(), p, -1)
    assert small["sparse_items"] == 0
    regs12 = synth.survey_sketches(1400, 12, seed=0x5A1200)[0]
    keys12, gcnt12 = sc.keys_and_counts(regs12, 12)
    assert plan(host, keys12, gcnt12, 12, -1)[0]["sparse_items"] == 0
    assert plan(host, keys12, gcnt12, 12, 1)[0]["sparse_items"] > 0  # (forced: the gate is ignored, never the cap)
    # two bands (a small C(v) budget), a row range, parts: still one route per plane
    for kw in (dict(budget=40 << 20), dict(rb=130, re=900), dict(rb=0, re=1400, nparts=3, want_parts=1)):
        st, _ = plan(host, keys, gcnt, p, 2, **kw)
        assert st["sparse_items"] > 0, kw
