"""The sided route of the sparse planes on the device (kernels_sparseplane.hip; plan.h, Tuning::sparse_sided): a plane of a
tile counted from ONE block's position lists against the other block's table, in either polarity of either side, from both
ends of the tile's range, transposed where the sparse side is the column block -- into the C(v) slots of the tile kernel.

The route is FORCED (sparse_sided = 1) at these sizes, where the automatic rule is off.  Per collection
(tests/sparse_cases.py), size and precision: the four counters of `info` are the model's (tools/path_census.py); the output
bytes of the three estimators and of JI, SIZES and CONTAINMENT_INDEX equal the same context's run with every route off, in
both placements of the table; one triangle is within the suite's 1e-6 of the oracle.  Then the call forms that share the
plan, a cap changed between calls on one attached matrix (the thresholds are the per-sketch pass's: the route is off for a
call at another cap), and the automatic rule at a size where it engages.  tests/test_sparse_sided_model.py asserts that
these inputs hold every kind of item."""
import numpy as np
import pytest

import dashing_amd

import sparse_cases as sc
from sparse_cases import pcs
from test_gpu_sparse_planes import close, routed

pytestmark = pytest.mark.gpu
MEASURES = (dashing_amd.JI, dashing_amd.SIZES, dashing_amd.CONTAINMENT_INDEX)
SIZES = ((131, 13), (257, 14), (257, 15), (131, 16))
KINDS = ("mixed_thresholds", "survey", "near_duplicates")
KEYS = ("sparse_items", "sparse_sided_items", "sparse_transposed_items", "sparse_table_slabs")


class sided(routed):
    """test_gpu_sparse_planes.routed with the sided route's option: set for a block, and put back behind it"""

    def __init__(self, ctx, on, planes=0, cap=None, **more):
        routed.__init__(self, ctx, planes, cap, sparse_sided=on, **more)
        self.defaults["sparse_sided"] = -1


def counters(ctx):
    return tuple(ctx.info(k) for k in KEYS)


def model(regs, p, **kw):
    c = pcs.census(regs, p, **kw)
    return tuple(c.plan[k] for k in KEYS)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,p", SIZES)
def test_forced_route_bytes_and_oracle(ctx, oracle, kind, n, p):
    regs, _ = sc.collection(kind, n, p)
    ctx.set_sketches(regs)
    with sided(ctx, 0):
        off = {(e, m): ctx.dist_rows(estim=e, result_type=m) for e in (0, 1, 2) for m in MEASURES}
        assert counters(ctx) == (0, 0, 0, 0)
    close(off[(dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI)], oracle.dist_tri(regs, dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI, 31), (kind, n, p, "off"))
    want = model(regs, p, sparse_planes=0, sparse_sided=1)
    assert want[0] == want[1] > 0
    for lds in (1, 0):
        with sided(ctx, 1, sparse_lds=lds):
            for (e, m), ref in off.items():
                got = ctx.dist_rows(estim=e, result_type=m)
                assert counters(ctx) == want, (kind, n, p, lds)
                assert got.tobytes() == ref.tobytes(), (kind, n, p, lds, e, m)


def test_call_forms_share_the_route(ctx):
    """a row range in the layout made for it, two and three parts, two bands, and fragments beside routed planes: the bytes
    of the full call with the route off"""
    import torch

    n, p = 257, 14
    regs, _ = sc.collection("mixed_thresholds", n, p)
    ctx.set_sketches(regs)
    with sided(ctx, 0):
        full = ctx.dist_rows()
    rb, re = 37, n - 2
    a, b = dashing_amd.tri_span(n, 0, rb), dashing_amd.tri_span(n, 0, re)
    with sided(ctx, 1):
        assert ctx.dist_rows().tobytes() == full.tobytes() and ctx.info("sparse_transposed_items") > 0
    with sided(ctx, 1, range_sort_min_rows=1):
        assert ctx.dist_rows(rb, re).tobytes() == full[a:b].tobytes() and ctx.info("sparse_sided_items") > 0 and ctx.info("sorted") == 1
    dev = torch.device("cuda", 0)
    with sided(ctx, 1):
        for prb, pre, nparts in ((0, n, 2), (rb, re, 3)):
            a0, span = dashing_amd.tri_span(n, 0, prb), dashing_amd.tri_span(n, prb, pre)
            out = torch.full((span,), -3.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            ctx.dist_rows_parts_device_async(out.data_ptr(), prb, pre, nparts)
            ctx.wait()
            assert out.cpu().numpy().tobytes() == full[a0 : a0 + span].tobytes(), (prb, pre, nparts)
            assert ctx.info("sparse_sided_items") > 0
    with sided(ctx, 1, cum_budget_bytes=1 << 20):  # (a tile's C(v) is 32 KiB x planes: three tiles to a band)
        assert ctx.dist_rows().tobytes() == full.tobytes() and ctx.info("bands") >= 2 and ctx.info("sparse_sided_items") > 0
    with sided(ctx, 1, overflow_frag_permille=1000):
        assert ctx.dist_rows().tobytes() == full.tobytes() and ctx.info("frag_items") > 0 and ctx.info("sparse_sided_items") > 0


def test_block_over_the_cap_serves_as_table(ctx):
    """the collection of test_sparse_sided_model.test_cap_boundary: one sketch one entry above the cap at the top plane of its
    tiles.  Its block is the table of items the other blocks list, transposed where it is the row block, and its slab is
    built without lists: the bytes are those of the dense path only if that slab's lengths are the true set sizes"""
    from test_sparse_sided_model import one_over_the_cap

    regs, _, _ = one_over_the_cap()
    p = 14
    ctx.set_sketches(regs)
    with sided(ctx, 0):
        off = ctx.dist_rows()
    want = model(regs, p, sparse_planes=0, sparse_sided=1)
    assert want[2] > 0 and want[3] > 0
    for lds in (1, 0):
        with sided(ctx, 1, sparse_lds=lds):
            got = ctx.dist_rows()
            assert counters(ctx) == want, lds
            assert got.tobytes() == off.tobytes(), lds


def test_changed_cap(ctx):
    """sparse_cap changed between calls on the same attached matrix.  The thresholds are those of the per-sketch pass, at the
    cap it ran with: at another cap the sided route is off for the call (the two-plane route has its own bound and runs), and
    on again at the first cap.  The second cap is below the longest routed list of the first call."""
    n, p = 257, 14
    regs, _ = sc.collection("mixed_thresholds", n, p)
    ctx.set_sketches(regs)
    with sided(ctx, 0):
        full = ctx.dist_rows()
    c = pcs.census(regs, p, sparse_planes=2, sparse_sided=1)
    longest = 0
    for t in c.tiles:
        for pl, la, _, tr in t["sided"]:
            block, v = regs[c.blocks[t["bj"] if tr else t["bi"]]["cols"]], c.plan["pbase"] + 1 + pl
            longest = max(longest, int(((block < v) if la else (block >= v)).sum(axis=1).max()))
    small = longest // 2 // 8 * 8
    assert 8 <= small < longest <= pcs.SPARSE_CAP
    for cap, on in ((pcs.SPARSE_CAP, True), (small, False), (pcs.SPARSE_CAP, True)):
        with sided(ctx, 1, planes=2, cap=cap):
            got = ctx.dist_rows()
            want = model(regs, p, sparse_planes=2, sparse_cap=cap, sparse_sided=1 if on else 0)
            assert counters(ctx) == want and (want[1] > 0) == on, (cap, counters(ctx), want)
            assert got.tobytes() == full.tobytes(), cap


def test_automatic_rule(ctx):
    from dashing_amd import synth

    n, p = 1400, 14
    regs = synth.survey_sketches(n, p, seed=0x5A1400)[0]
    ctx.set_sketches(regs)
    with sided(ctx, 0):
        off = ctx.dist_rows()
        assert counters(ctx) == (0, 0, 0, 0)
    got = ctx.dist_rows()  # the defaults
    assert ctx.info("sparse_planes") == -1 and ctx.info("sparse_sided") == -1
    assert ctx.info("sparse_sided_items") > 0
    assert got.tobytes() == off.tobytes()
