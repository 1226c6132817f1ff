"""The sparse outer planes on the device (kernels_sparseplane.hip; plan.h, Tuning::sparse_planes): a tile's top one or two
planes counted from position lists instead of by the tile kernel, into the same C(v) slots.

The route is FORCED (sparse_planes = 1, 2) at these sizes, where the automatic rule is off.  Per collection
(tests/sparse_cases.py), size and precision: `sparse_items` is what the model says (tools/path_census.py); the output bytes of
the three estimators and of JI, SIZES and CONTAINMENT_INDEX equal the run with the route off; one estimator's triangle is
within the suite's 1e-6 of the oracle.  Then the call forms that share the plan (a row range, parts, two bands,
fragments beside routed planes), and one collection large enough for the automatic rule to engage by itself."""
import numpy as np
import pytest

import dashing_amd

import sparse_cases as sc
from sparse_cases import pcs

pytestmark = pytest.mark.gpu
RTOL = 1e-6
MEASURES = (dashing_amd.JI, dashing_amd.SIZES, dashing_amd.CONTAINMENT_INDEX)


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all() and (np.isnan(got) == np.isnan(ref)).all(), what
    err = np.abs(got[fin] - ref[fin])
    den = np.maximum(np.abs(ref[fin]), 1e-9)
    assert not (err > RTOL * den).any(), "%s: max rel err %.3g" % (what, (err / den).max())


class routed:
    """the two options set for a block, and put back behind it (the context is the session's)"""

    def __init__(self, ctx, planes, cap=None, **more):
        self.ctx, self.opts = ctx, dict(sparse_planes=planes, sparse_cap=pcs.SPARSE_CAP if cap is None else cap, **more)
        self.defaults = dict(sparse_planes=-1, sparse_cap=pcs.SPARSE_CAP, cum_budget_bytes=8 << 30, overflow_frag_permille=500,
                             range_sort_min_rows=1024, sparse_lds=1)

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, self.defaults[k])


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("p", (13, 14, 15, 16))
@pytest.mark.parametrize("n", (131, 257))
def test_forced_route_bytes_and_oracle(ctx, oracle, kind, n, p):
    regs, cap = sc.collection(kind, n, p)
    if kind == "cap_boundary":  # the host's statement of the two sizes, before the device runs
        g0 = sc.thresholds(regs, p)[4]
        assert sorted(set(g0.tolist())) == [cap, cap + 1] and int((g0 == cap + 1).sum()) == 1
    ctx.set_sketches(regs)
    with routed(ctx, 0):
        off = {(e, m): ctx.dist_rows(estim=e, result_type=m) for e in (0, 1, 2) for m in MEASURES}
        assert ctx.info("sparse_items") == 0
    close(off[(dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI)], oracle.dist_tri(regs, dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI, 31), (kind, n, p, "off"))
    for k in (1, 2):
        c = pcs.census(regs, p, sparse_planes=k, sparse_cap=pcs.SPARSE_CAP if cap is None else cap)
        with routed(ctx, k, cap):
            for (e, m), want in off.items():
                got = ctx.dist_rows(estim=e, result_type=m)
                assert ctx.info("sparse_items") == c.plan["sparse_items"], (kind, n, p, k)
                assert got.tobytes() == want.tobytes(), (kind, n, p, k, e, m)
            # the tile's plane range is what k_finalize and the C(v) scratch still see; the tile kernel has fewer items
            assert ctx.info("avg_tile_planes_x100") == c.plan["avg_tile_planes_x100"] and ctx.info("tiles") == c.plan["tiles"]
            assert ctx.info("items") - ctx.info("frag_items") <= c.plan["dense_planes"] <= ctx.info("items")
        # the other placement of the table (gathered from global memory; at p = 16 it is the only one)
        with routed(ctx, k, cap, sparse_lds=0):
            e, m = dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI
            assert ctx.dist_rows(estim=e, result_type=m).tobytes() == off[(e, m)].tobytes(), (kind, n, p, k, "gathered")
            assert ctx.info("sparse_items") == c.plan["sparse_items"]
        if kind == "constant":
            assert c.plan["sparse_items"] == 0
        elif kind == "cap_boundary":
            assert 0 < c.plan["sparse_items"] < k * c.plan["tiles"]
        else:
            assert c.plan["sparse_items"] > 0


def test_call_forms_share_the_route(ctx):
    """a row range (in the identity layout the route stays off; in the layout made for the range it runs), parts, two
    bands, and fragments beside routed planes: the bytes of the full call with the route off"""
    import torch

    n, p = 257, 14
    regs, _ = sc.collection("mixed_thresholds", n, p)
    ctx.set_sketches(regs)
    with routed(ctx, 0):
        full = ctx.dist_rows()
    rb, re = 37, n - 2
    a, b = dashing_amd.tri_span(n, 0, rb), dashing_amd.tri_span(n, 0, re)
    with routed(ctx, 2):
        assert ctx.dist_rows().tobytes() == full.tobytes() and ctx.info("sparse_items") > 0
        assert ctx.dist_rows(rb, re).tobytes() == full[a:b].tobytes()
    with routed(ctx, 2, range_sort_min_rows=1):
        assert ctx.dist_rows(rb, re).tobytes() == full[a:b].tobytes() and ctx.info("sparse_items") > 0 and ctx.info("sorted") == 1
    dev = torch.device("cuda", 0)
    with routed(ctx, 2):
        for prb, pre, nparts in ((0, n, 2), (rb, re, 3)):
            a0, span = dashing_amd.tri_span(n, 0, prb), dashing_amd.tri_span(n, prb, pre)
            out = torch.full((span,), -3.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            ctx.dist_rows_parts_device_async(out.data_ptr(), prb, pre, nparts)
            ctx.wait()
            assert out.cpu().numpy().tobytes() == full[a0 : a0 + span].tobytes(), (prb, pre, nparts)
            assert ctx.info("sparse_items") > 0
    with routed(ctx, 2, cum_budget_bytes=1 << 20):  # (a tile's C(v) is 32 KiB x planes: three tiles to a band)
        assert ctx.dist_rows().tobytes() == full.tobytes() and ctx.info("bands") >= 2 and ctx.info("sparse_items") > 0
    with routed(ctx, 1, overflow_frag_permille=1000):
        assert ctx.dist_rows().tobytes() == full.tobytes() and ctx.info("frag_items") > 0 and ctx.info("sparse_items") > 0


def test_automatic_rule_engages(ctx):
    from dashing_amd import synth

    n, p = 1400, 14
    ctx.set_sketches(synth.survey_sketches(n, p, seed=0x5A1400)[0])
    with routed(ctx, 0):
        off = ctx.dist_rows()
        assert ctx.info("sparse_items") == 0
        items_off = ctx.info("items")
    got = ctx.dist_rows()  # the defaults
    assert ctx.info("sparse_planes") == -1 and ctx.info("sparse_items") > 0 and ctx.info("items") < items_off
    assert got.tobytes() == off.tobytes()
