"""The compare path's DATA-DEPENDENT branches, held to the oracle in every instance: which arm of finalize_block, join_tails
and k_selfhist_card a collection takes is decided by its register values, so every collection here (tests/path_cases.py)
is first shown ON THE HOST to take the branches it is named for -- with the census model (tools/path_census.py), in both
column orders -- and the model is tied to the device's own plan through dsh_get_info; only then does the device run.
tests/test_path_census.py asserts that these collections fill the matrix instance x condition.

Per collection: the triangle against the oracle (|d| <= 1e-6 * max(|ref|, 1e-9), finite and NaN positions equal) for the
three estimators and the measures JI, SIZES and CONTAINMENT_INDEX, the cardinalities at rtol 1e-12, and every call form
byte for byte against the full call of the same context."""
import numpy as np
import pytest

import dashing_amd

import path_cases as pc
import path_census as pcs
import thr_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-6
MEASURES = (dashing_amd.JI, dashing_amd.SIZES, dashing_amd.CONTAINMENT_INDEX)
IDS = [c.id for c in pc.CASES]


def close(got, ref, what):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all() and (np.isnan(got) == np.isnan(ref)).all(), what
    assert (got[~fin & ~np.isnan(ref)] == ref[~fin & ~np.isnan(ref)]).all(), what  # (infinities of the same sign)
    err = np.abs(got[fin] - ref[fin])
    den = np.maximum(np.abs(ref[fin]), 1e-9)
    bad = err > RTOL * den
    assert not bad.any(), "%s: max rel err %.3g at %d of %d" % (what, (err / den).max(), int(bad.sum()), err.size)


_refs = {}


def reference(oracle, case, estim=dashing_amd.ESTIM_ERTL_MLE, rt=dashing_amd.JI):
    """the oracle's triangle of a case: computed once, never changed"""
    key = (case.id, estim, rt)
    if key not in _refs:
        _refs[key] = oracle.dist_tri(case.regs(), estim, rt, 31)
        _refs[key].setflags(write=False)
    return _refs[key]


def assert_named_conditions(case):
    """host only: the instance, and the conditions the family is named for, in both column orders"""
    for sort in (True, False):
        c = case.census(sort=sort)
        assert c.instance == pc.INSTANCES[case.p], (case.id, c.instance)
        missing = pc.NAMED_FOR[case.family] - c.holds()
        assert not missing, (case.id, "sorted" if sort else "identity", sorted(missing))
        if case.family == "two_valued_and_constant":
            pc.counts_at_the_limit(case, c)


def assert_plan_is_the_models(ctx, c):
    """the device's plan of the last full call against the census of the same column order.  dsh_get_info names no
    per-tile figure, so the tiles' plane counts (behind tile.no_dense_plane and tile.planes_beyond_batch) are tied to the
    device through their SUM only (avg_tile_planes_x100 over the same number of tiles), and the work items through zero or
    not and, for the lockstep kernel, a bound: a free-running item is a run of k-chunks, not a plane.  A tighter tie needs
    new ABI, which this file does not add."""
    got = {k: ctx.info(k) for k in ("planes", "pbase", "kpad", "tiles", "avg_tile_planes_x100", "cum_bytes", "lockstep", "sorted")}
    assert ctx.info("kc") == pcs.PAIR_KC and ctx.info("bands") == 1
    assert got == {k: c.plan[k] for k in got}, (got, c.plan)
    items, frags = ctx.info("items"), ctx.info("frag_items")
    assert (items == 0) == (c.plan["sum_tile_planes"] == 0), (items, c.plan)
    if c.plan["lockstep"]:  # an item is a plane of a tile, or one of f >= 2 fragments of one
        assert items - frags <= c.plan["sum_tile_planes"] <= items, (items, frags, c.plan)


@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_paths_against_the_oracle(ctx, oracle, case):
    assert_named_conditions(case)
    regs = case.regs()
    n = case.n
    try:
        for sort in (1, 0):
            ctx.set_option("sort", sort)
            ctx.set_sketches(regs)
            got = ctx.dist_rows()
            assert ctx.info("sorted") == sort
            assert_plan_is_the_models(ctx, case.census(sort=bool(sort)))
            close(got, reference(oracle, case), (case.id, "sort", sort))
    finally:
        ctx.set_option("sort", -1)
    ctx.set_sketches(regs)
    for estim, rt in [(e, m) for e in (0, 1, 2) for m in MEASURES]:
        close(ctx.dist_rows(estim=estim, result_type=rt), reference(oracle, case, estim, rt), (case.id, estim, rt))
    assert ctx.info("sorted") == 1  # (the default order of a full triangle is the key order)
    for estim in (0, 1, 2):
        got, want = ctx.cardinalities(estim), oracle.cardinalities(regs, estim)
        assert got.shape == (n,) and np.allclose(got, want, rtol=1e-12, atol=0, equal_nan=True), (case.id, estim)


@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_call_forms_agree_byte_for_byte(ctx, case):
    """the other column order, other list caps (other thresholds, lists and planes: the same bytes), a row range, a
    rectangle (GENERAL instance), parts (signalling instance), the nearest neighbours through the square and through the
    bands, and the thresholded output: each against the full call of the same context, which the test above holds to
    the oracle"""
    import torch

    regs = case.regs()
    n = case.n
    ctx.set_sketches(regs)
    full = ctx.dist_rows()
    sq = np.zeros((n, n), np.float32)
    iu = np.triu_indices(n, 1)
    sq[iu] = full
    sq.T[iu] = full
    try:
        for sort in (0, 1):
            ctx.set_option("sort", sort)
            assert ctx.dist_rows().tobytes() == full.tobytes() and ctx.info("sorted") == sort, sort
    finally:
        ctx.set_option("sort", -1)
    try:
        for emax, elow in pc.CAPS[1:]:
            ctx.set_option("emax", emax)
            ctx.set_option("elow", elow)
            assert ctx.dist_rows().tobytes() == full.tobytes(), (emax, elow)
            c = case.census(emax, elow, sort=True)
            assert (ctx.info("emax"), ctx.info("elow")) == (emax, elow)
            assert (ctx.info("planes"), ctx.info("pbase"), ctx.info("avg_tile_planes_x100")) == (c.plan["planes"], c.plan["pbase"], c.plan["avg_tile_planes_x100"])
    finally:
        ctx.set_option("emax", -1)
        ctx.set_option("elow", -1)
    # a row range; the same range in the layout made for it (wanted rows first, key-ordered)
    rb, re = 37, n - 2
    a, b = dashing_amd.tri_span(n, 0, rb), dashing_amd.tri_span(n, 0, re)
    assert ctx.dist_rows(rb, re).tobytes() == full[a:b].tobytes()
    try:
        ctx.set_option("range_sort_min_rows", 1)
        assert ctx.dist_rows(rb, re).tobytes() == full[a:b].tobytes()
    finally:
        ctx.set_option("range_sort_min_rows", 1024)
    # rectangles across the block boundary: above the diagonal, and below it
    assert ctx.dist_rect(3, 125, 126, n).tobytes() == np.ascontiguousarray(sq[3:125, 126:n]).tobytes()
    assert ctx.dist_rect(126, n, 0, 125).tobytes() == np.ascontiguousarray(sq[126:n, 0:125]).tobytes()
    # parts that announce themselves
    dev = torch.device("cuda", 0)
    for prb, pre, nparts in ((0, n, 2), (rb, re, 3)):
        a, span = dashing_amd.tri_span(n, 0, prb), dashing_amd.tri_span(n, prb, pre)
        out = torch.full((span,), -3.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.dist_rows_parts_device_async(out.data_ptr(), prb, pre, nparts)
        ctx.wait()
        assert out.cpu().numpy().tobytes() == full[a : a + span].tobytes(), (prb, pre, nparts)
    # nearest neighbours: the square, then bands of query rows
    for budget in (96 << 30, 0):
        ctx.set_option("knn_square_budget_bytes", budget)
        try:
            gi, gv = ctx.knn(9)
        finally:
            ctx.set_option("knn_square_budget_bytes", 96 << 30)
        assert (gi < n).all() and (gi != np.arange(n)[:, None]).all()
        assert gv.tobytes() == np.ascontiguousarray(sq[np.arange(n)[:, None], gi]).tobytes(), budget
    # the thresholded output (the band walk, also over a collection without planes) at the value whose share of passing
    # pairs is nearest to one half, the smallest value aside (where many pairs are 0 the median would let every pair
    # pass): some pairs pass and some do not -- unless all values are equal (all pass) or none is finite (none passes)
    fin = np.sort(full[np.isfinite(full)])
    u = np.unique(fin)
    if u.size >= 2:
        share = 1.0 - np.searchsorted(fin, u[1:], side="left") / fin.size
        t = float(u[1:][np.argmin(np.abs(share - 0.5))])
    else:
        t = float(u[0]) if u.size else 0.5
    want = thr_ref.tri(full, n, 0, n, t, dashing_amd.JI)
    if u.size >= 2:
        assert 0 < want[1].size < full.size, (want[1].size, full.size, t)
    else:
        assert want[1].size == fin.size  # (every finite pair: all of them, or none)
    assert thr_ref.same(ctx.dist_threshold(t), want)
