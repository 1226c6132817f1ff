"""CPU: the sided route of the sparse planes (dashing_amd/csrc/plan.h, Tuning::sparse_sided).

The counting kernel walks ONE side's position lists and reads the other side's bits from a table, so only the list side
has to be sparse, in either polarity -- U(v) = {a >= v} or A(v) = {a < v}.  Here: the numpy statement of the four formulas
(tools/path_census.py, sided_plane_counts) against popcount(A_v & B_v); the planner through dshh_plan_check_sparse_sided
(csrc/host/plan_capi.cpp), which holds the plan to its contract -- every (tile, plane) in exactly one route, the dense
remainder one range, every item's list block within its bound in the item's polarity -- against the model, tile by tile;
the bound against the registers themselves; the cap's boundary; a stale cap; and the option's settings.

The model's sided route was written beside the planner's and states the same rule (depth, polarity, the tie to the row
block): a shared misreading of the rule would pass test_plan_is_the_models.  The checks that do not share it are
test_bound_against_the_registers and test_cap_boundary here (set sizes counted from the registers), the contract inside
dshh_plan_check_sparse_sided, and the byte equality with the dense path in tests/test_gpu_sparse_sided.py."""
import ctypes as C
import os

import numpy as np
import pytest

import sparse_cases as sc
from sparse_cases import pcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 128
SIZES = ((131, 13), (257, 14), (257, 15), (131, 16))
KINDS = ("mixed_thresholds", "survey", "near_duplicates")


def dense_counts(rows, cols, v):
    """popcount(A_v & B_v): the tile kernel's statement"""
    a, b = np.asarray(rows) < v, np.asarray(cols) < v
    return (a[:, None, :] & b[None, :, :]).sum(axis=2)


def all_four(lists, tables, v):
    want = dense_counts(lists, tables, v)
    for la in (0, 1):
        for ta in (0, 1):
            assert (pcs.sided_plane_counts(lists, tables, v, la, ta) == want).all(), (v, la, ta)


def test_formulas_hand_made():
    rows = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [7, 7, 7, 7, 7, 7, 7, 7], [0, 0, 0, 0, 0, 0, 0, 0], [3, 3, 4, 4, 3, 3, 4, 4]], np.uint8)
    cols = np.array([[7, 6, 5, 4, 3, 2, 1, 0], [4, 4, 4, 4, 4, 4, 4, 4], [0, 9, 0, 9, 0, 9, 0, 9], [0, 1, 2, 3, 4, 5, 6, 7]], np.uint8)
    for v in range(0, 11):  # (v = 0: every A empty, every U full; v = 10: the reverse; cols[3] = rows[0]: a full intersection)
        all_four(rows, cols, v)


@pytest.mark.parametrize("p", (6, 9, 13))
def test_formulas_random_and_at_the_cap(p):
    rng = np.random.default_rng(p)
    m = 1 << p
    rows = rng.integers(0, 12, (9, m)).astype(np.uint8)
    cols = rng.integers(0, 12, (7, m)).astype(np.uint8)
    cols[0] = rows[0]  # the intersection is the whole set
    cols[1] = 0        # an empty U at every v > 0, a full A
    cap = m // 8
    rows[2] = 3        # sets of exactly `cap` positions at v = 5: U = the first cap positions ...
    rows[2, :cap] = 7
    rows[3] = 7        # ... and A = the last cap
    rows[3, m - cap :] = 3
    vU, vA = pcs.sided_thresholds(rows[2:4], cap)
    assert (int((rows[2] >= 5).sum()), int((rows[3] < 5).sum())) == (cap, cap) and vU[0] == 4 and vA[1] == 7
    for v in (0, 1, 5, 10, 11, 12):
        all_four(rows, cols, v)


def test_thresholds_are_the_definition():
    regs, _ = sc.collection("mixed_thresholds", 19, 13)
    for cap in (0, 1, 200, 1280, 2040, 1 << 13):
        vU, vA = pcs.sided_thresholds(regs, cap)
        for r, u, a in zip(regs, vU, vA):
            assert (r >= u).sum() <= cap and (u == 0 or (r >= u - 1).sum() > cap)
            assert (r < a).sum() <= cap and (a == 64 or (r < a + 1).sum() > cap)


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    u64, i32, u32, vp = C.c_uint64, C.c_int, C.c_uint32, C.c_void_p
    lib.dshh_plan_check_sparse.argtypes = [u64, vp, vp, i32, i32, u64, u64, u32, i32, i32, u64, u32, i32, u32, vp, vp, u64, C.c_char_p, C.c_size_t]
    lib.dshh_plan_check_sparse_sided.argtypes = [u64, vp, vp, vp, u32, i32, i32, u64, u64, u32, i32, i32, u64, u32, i32, i32, u32, vp, vp, u64, vp, u64,
                                                 vp, u64, C.c_char_p, C.c_size_t]
    return lib


NAMES = ("tiles", "bands", "items", "parts", "planes_x100", "npad", "P", "rounds", "frags", "round", "sparse_items", "slabs", "sided_items",
         "transposed_items", "table_slabs")


def thr_words(regs, cap):
    vU, vA = pcs.sided_thresholds(regs, cap)
    return np.ascontiguousarray(vU.astype(np.uint32) | (vA.astype(np.uint32) << 8), np.uint32)


def plan(host, keys, gcnt, thr, thr_cap, p, sided, cap=pcs.SPARSE_CAP, planes=0, round_items=768, budget=8 << 30):
    """(stats, routes [tiles][bi, bj, pb, pe, below, above], items [items][tile, plane, flags, slab, slab], slabs [slabs][block, plane, flags])"""
    n = len(keys)
    stats = np.zeros(15, np.uint64)
    nt = (n + TILE - 1) // TILE
    ntiles = nt * (nt + 1) // 2
    routes, items, slabs = np.zeros((ntiles, 6), np.uint32), np.zeros((ntiles * 64, 5), np.uint32), np.zeros((nt * 64, 3), np.uint32)
    err = C.create_string_buffer(512)
    rc = host.dshh_plan_check_sparse_sided(n, keys.ctypes.data, gcnt.ctypes.data, None if thr is None else thr.ctypes.data, thr_cap, 0, 1, 0, n, 1, 0, p,
                                           budget, round_items, planes, sided, cap, stats.ctypes.data, routes.ctypes.data, len(routes),
                                           items.ctypes.data, len(items), slabs.ctypes.data, len(slabs), err, 512)
    assert rc == 0, err.value.decode()
    st = dict(zip(NAMES, (int(x) for x in stats)))
    return st, routes[: st["tiles"]], items[: st["sparse_items"]], slabs[: st["slabs"]]


_cache = {}


def case(kind, n, p):
    if (kind, n, p) not in _cache:
        regs, _ = sc.collection(kind, n, p)
        _cache[(kind, n, p)] = (regs, *sc.keys_and_counts(regs, p), thr_words(regs, pcs.SPARSE_CAP))
    return _cache[(kind, n, p)]


def kinds_of(census):
    """how often each kind of the sided route occurs in a model plan"""
    k = dict.fromkeys(("uu_beyond_two", "aa", "mixed", "transposed"), 0)
    for t in census.tiles:
        k["uu_beyond_two"] += sum(1 for x, it in enumerate(t["sided"][: t["sparse"]]) if x >= 2 and it[1:3] == (0, 0))
        k["aa"] += sum(1 for it in t["sided"] if it[1:3] == (1, 1))
        k["mixed"] += sum(1 for it in t["sided"] if it[1] != it[2])
        k["transposed"] += sum(it[3] for it in t["sided"])
    k["table_slabs"] = census.plan["sparse_table_slabs"]
    return k


@pytest.mark.parametrize("n,p", SIZES)
def test_inputs_hold_every_kind(n, p):
    """asserted before anything else: what the other tests (and tests/test_gpu_sparse_sided.py) rely on the inputs for"""
    regs = case("mixed_thresholds", n, p)[0]
    k = kinds_of(pcs.census(regs, p, sparse_planes=0, sparse_sided=1))
    assert all(v >= 1 for v in k.values()), k
    near = pcs.census(case("near_duplicates", n, p)[0], p, sparse_planes=0, sparse_sided=1)
    kn = kinds_of(near)
    assert kn["transposed"] == 0 and kn["table_slabs"] == 0, kn
    # A x A on the diagonal -- except at (257, 15), where the sets {a < v} of the copies' lowest plane are above the cap
    diagonal_aa = any(t["bi"] == t["bj"] and any(it[1:3] == (1, 1) for it in t["sided"]) for t in near.tiles)
    assert diagonal_aa == ((n, p) != (257, 15)), kn


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,p", SIZES)
def test_plan_is_the_models(host, kind, n, p):
    regs, keys, gcnt, thr = case(kind, n, p)
    c = pcs.census(regs, p, sparse_planes=0, sparse_sided=1)
    st, routes, items, slabs = plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, 1)
    assert st["sparse_items"] == c.plan["sparse_items"] == st["sided_items"] and st["transposed_items"] == c.plan["sparse_transposed_items"]
    assert st["table_slabs"] == c.plan["sparse_table_slabs"] == int((slabs[:, 2] & 2 != 0).sum())
    model = {(t["bi"], t["bj"]): t for t in c.tiles}
    tile_at = {}
    for ti, r in enumerate(routes):
        t = model[(int(r[0]), int(r[1]))]
        assert (int(r[2]), int(r[3]), int(r[4]), int(r[5])) == (t["Lp"] - c.plan["pbase"], t["T"] - c.plan["pbase"], t["below"], t["sparse"]), (r, t)
        tile_at[ti] = t
    got = {}
    for it in items:
        got.setdefault(int(it[0]), set()).add((int(it[1]), int(it[2]) & 1, int(it[2]) >> 1 & 1, int(it[2]) >> 2 & 1))
    for ti, t in tile_at.items():
        assert got.get(ti, set()) == set(t["sided"]), (ti, t)
    # the dense remainder: the tile kernel's items are the planes left over (one-plane items here, whole or in fragments)
    assert st["items"] - st["frags"] <= c.plan["dense_planes"] <= st["items"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,p", SIZES)
def test_bound_against_the_registers(host, kind, n, p):
    """every routed item's list block: the true sizes of its sets, from the registers, are within the cap"""
    regs, keys, gcnt, thr = case(kind, n, p)
    c = pcs.census(regs, p, sparse_planes=0, sparse_sided=1)
    st, routes, items, slabs = plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, 1)
    assert len(items) > 0
    for it in items:
        bi, bj = int(routes[it[0]][0]), int(routes[it[0]][1])
        v, la, tr = c.plan["pbase"] + 1 + int(it[1]), int(it[2]) & 1, int(it[2]) >> 2 & 1
        block = regs[c.blocks[bj if tr else bi]["cols"]]
        sizes = (block < v).sum(axis=1) if la else (block >= v).sum(axis=1)
        assert int(sizes.max()) <= pcs.SPARSE_CAP, (bi, bj, v, la, tr, int(sizes.max()))
        lslab = slabs[int(it[4] if tr else it[3])]
        assert (int(lslab[0]), int(lslab[1]), int(lslab[2])) == (bj if tr else bi, int(it[1]), la), "the list slab: its block, plane, polarity; with lists"


def one_over_the_cap(n=257, p=14, cap=pcs.SPARSE_CAP):
    """(regs, s, v): mixed_thresholds with sketch s given exactly cap + 1 registers >= v, the top plane of the tile (0, 1)"""
    regs = case("mixed_thresholds", n, p)[0].copy()
    c0 = pcs.census(regs, p, sparse_planes=0, sparse_sided=1)
    v = next(t for t in c0.tiles if (t["bi"], t["bj"]) == (0, 1))["T"]
    s = int(c0.blocks[0]["cols"][0])
    short = cap + 1 - int((regs[s] >= v).sum())
    assert short > 0
    regs[s, np.flatnonzero(regs[s] < v)[:short]] = v
    return regs, s, v


def test_cap_boundary(host):
    """a block with one sketch one entry above the cap at v is never the list side at v; it still serves as a table: the
    other block of the tile lists against it, its slab of that plane is built, U, and without lists (that the slab's lengths
    are the true set sizes is the device's to show: tests/test_gpu_sparse_sided.py runs this collection)"""
    n, p, cap = 257, 14, pcs.SPARSE_CAP
    regs, s, v = one_over_the_cap(n, p, cap)
    keys, gcnt = sc.keys_and_counts(regs, p)
    for use, lists in ((cap, False), (cap + 1, True)):
        c = pcs.census(regs, p, sparse_planes=0, sparse_cap=use, sparse_sided=1)
        b = next(k for k, blk in enumerate(c.blocks) if s in blk["cols"])
        sizes = {k: (regs[blk["cols"]] >= v).sum(axis=1) for k, blk in enumerate(c.blocks)}
        assert int(sizes[b].max()) == cap + 1 and int((sizes[b] > cap).sum()) == 1  # the one sketch, one entry over
        assert int((regs[c.blocks[b]["cols"]] < v).sum(axis=1).min()) > use                # (nor does the block qualify by A)
        st, routes, items, slabs = plan(host, keys, gcnt, thr_words(regs, use), use, p, 1, cap=use)
        assert st["sparse_items"] == c.plan["sparse_items"]
        pl = v - c.plan["pbase"] - 1
        at_v = [(int(routes[it[0]][0]), int(routes[it[0]][1]), int(it[2])) for it in items if int(it[1]) == pl]
        b_lists = [x for x in at_v if (x[0] == b and not x[2] >> 2 & 1) or (x[1] == b and x[2] >> 2 & 1)]
        assert bool(b_lists) == lists, (use, b_lists)
        if lists:
            continue
        # the blocks that qualify at v and share a tile with b whose range holds the plane: each lists against b's table
        others = [o for o in sizes if o != b and int(sizes[o].max()) <= use and
                  any(int(r[0]) == min(b, o) and int(r[1]) == max(b, o) and int(r[2]) <= pl < int(r[3]) for r in routes)]
        assert others, "no block qualifies beside the one over the cap: the case says nothing"
        for o in others:
            mine = [x for x in at_v if (x[0], x[1]) == (min(b, o), max(b, o))]
            assert len(mine) == 1 and (mine[0][2] >> 2 & 1) == int(b < o) and mine[0][2] & 3 == 0, (o, mine)  # o lists (U), b is the table (U)
        assert not any((x[0], x[1]) == (b, b) for x in at_v)  # b against itself stays dense at v
        s_b = [x for x in slabs if int(x[0]) == b and int(x[1]) == pl]
        assert len(s_b) == 1 and int(s_b[0][2]) == 2, s_b  # one slab: U, table only


def test_stale_cap_keeps_the_route_off(host):
    """thresholds belong to the cap they were computed for: at another sparse_cap the sided route is off for the call"""
    n, p = 257, 14
    regs, keys, gcnt, thr = case("mixed_thresholds", n, p)
    assert plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, 1)[0]["sparse_items"] > 0
    for cap in (pcs.SPARSE_CAP - 8, 640, pcs.SPARSE_CAP_MAX):
        st = plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, 1, cap=cap)[0]
        assert st["sparse_items"] == 0 and st["slabs"] == 0
        two = plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, 1, cap=cap, planes=2)[0]  # (the two-plane route has its own bound)
        assert two["sparse_items"] == pcs.census(regs, p, sparse_planes=2, sparse_cap=cap).plan["sparse_items"] and two["sided_items"] == 0
    assert plan(host, keys, gcnt, None, 0, p, 1)[0]["sparse_items"] == 0  # no thresholds: no sided route


@pytest.mark.parametrize("n,p", ((257, 14), (131, 16), (257, 12)))
def test_option_settings(host, n, p):
    """off (0) and automatic (-1) beside a forced or switched-off two-plane route: today's plan, through both entries; forced
    below p = 13: off; automatic beside the automatic two-plane rule: behind its gate"""
    regs, keys, gcnt, thr = case("mixed_thresholds", n, p)
    for planes in (-1, 0, 1, 2):
        stats = np.zeros(12, np.uint64)
        err = C.create_string_buffer(512)
        nt = (n + TILE - 1) // TILE
        routes = np.zeros((nt * (nt + 1) // 2, 5), np.uint32)
        rc = host.dshh_plan_check_sparse(n, keys.ctypes.data, gcnt.ctypes.data, 0, 1, 0, n, 1, 0, p, 8 << 30, 768, planes, pcs.SPARSE_CAP,
                                         stats.ctypes.data, routes.ctypes.data, len(routes), err, 512)
        assert rc == 0, err.value.decode()
        old = [int(x) for x in stats]
        assert old[10] == pcs.census(regs, p, sparse_planes=planes).plan["sparse_items"]
        for sided in ((0, -1) if planes >= 0 else (0,)):
            st = plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, sided, planes=planes)[0]
            assert [st[k] for k in NAMES[:12]] == old and st["sided_items"] == st["table_slabs"] == 0, (planes, sided)
    auto = plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, -1, planes=-1)[0]  # (a few tiles: the band is below the gate)
    assert auto["sparse_items"] == 0
    forced = plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, 1)[0]
    assert (forced["sided_items"] > 0) == (p >= 13)


def test_automatic_rule_behind_the_gate(host):
    n, p = 1400, 14
    from dashing_amd import synth

    regs = synth.survey_sketches(n, p, seed=0x5A1400)[0]
    keys, gcnt = sc.keys_and_counts(regs, p)
    thr = thr_words(regs, pcs.SPARSE_CAP)
    c = pcs.census(regs, p, sparse_planes=-1, sparse_sided=-1)
    st = plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, -1, planes=-1)[0]
    assert st["sparse_items"] == c.plan["sparse_items"] and st["sided_items"] == c.plan["sparse_sided_items"]
    assert (st["sided_items"] > 0) == pcs.SPARSE_SIDED_AUTO
