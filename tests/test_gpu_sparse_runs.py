"""Runs of items per workgroup in the LDS placement of the sparse counting kernel (kernels_sparseplane.hip,
k_sparse_count_lds; option sparse_run, info sparse_table_fills; plan.h, sparse_table_fills): a workgroup takes `sparse_run`
items of an XCD residue one behind the other, stages the table word only where the table slab changes, and reads the
counters out on all four lanes of a row.

The route is FORCED (sparse_sided = 1).  Per collection (tests/sparse_cases.py) and size -- 3 and 6 blocks, so that a residue
holds several items; p = 15 has one workgroup per CU -- and per run length: the output bytes of three estimators x (JI, SIZES,
CONTAINMENT_INDEX) equal the same context's run with every route off and its run with the table gathered (sparse_lds = 0);
sparse_table_fills is the host function's count on the items the host planner makes for the same keys, which a numpy
restatement (tests/sparse_runs.py) shares; one triangle per size is within the suite's 1e-6 of the oracle.  What the runs of
each case hold is stated on the host first (tests/sparse_runs.py, conditions); test_runs_hold_every_condition asserts what the
file as a whole covers.

Two things the planner cannot make, so that no collection can hold them.  (1) A transposed item followed by a plain one of
the same table slab: order_sparse_items (plan.cpp) sorts the items of a table block and plane by the sum of their tile's two
blocks, a plain item of table block a is tile (c, a) with c <= a, a transposed one is tile (a, b) with b > a, and c + a <
a + b: the plain ones always come first.  The reverse order is covered here; tests/test_sparse_runs_model.py counts both on
hand-made lists.  (2) 32-bit C(v) in this kernel: C(v) is 32 bits wide at p = 16 only (engine.hip), where the table is
gathered; at p = 15 the identical sketches of tests/path_cases.py plan no sparse item at all."""
import pytest

import dashing_amd

import sparse_runs as sr
from sparse_cases import pcs
from test_gpu_sparse_planes import close
from test_gpu_sparse_sided import MEASURES, sided
from test_sparse_sided_model import case, host, plan  # noqa: F401  (host: the fixture of the host library)

pytestmark = pytest.mark.gpu
SIZES = ((257, 13), (257, 14), (641, 14), (257, 15))
KINDS = ("mixed_thresholds", "survey", "near_duplicates")


class runs_of(sided):
    """test_gpu_sparse_sided.sided, forced, at a run length: set for a block, and put back behind it"""

    def __init__(self, ctx, run, **more):
        sided.__init__(self, ctx, 1, sparse_run=run, **more)
        self.defaults["sparse_run"] = 0


def host_items(host, kind, n, p):
    _, keys, gcnt, thr = case(kind, n, p)
    st, _, items, _ = plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, 1)
    assert st["bands"] == 1  # (one launch: the items are its list)
    return items


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,p", SIZES)
def test_runs_bytes_fills_and_oracle(ctx, oracle, host, kind, n, p):
    regs = case(kind, n, p)[0]
    items = host_items(host, kind, n, p)
    assert len(items) > 8  # (a residue of more than one item)
    ctx.set_sketches(regs)
    with sided(ctx, 0):
        off = {(e, m): ctx.dist_rows(estim=e, result_type=m) for e in (0, 1, 2) for m in MEASURES}
        assert ctx.info("sparse_items") == 0 and ctx.info("sparse_table_fills") == 0
    if kind == "mixed_thresholds":
        close(off[(dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI)], oracle.dist_tri(regs, dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI, 31), (kind, n, p, "off"))
    with sided(ctx, 1, sparse_lds=0):
        gathered = {k: ctx.dist_rows(estim=k[0], result_type=k[1]) for k in off}
        assert ctx.info("sparse_items") == len(items) and ctx.info("sparse_table_fills") == 0
    fills = {}
    for run in sr.RUNS:
        want = sr.fills(items, run)
        assert sr.host_fills(host, items, run) == want
        held = sr.conditions(items, run)
        assert (run != 1 or held["single"]) and (run != 64 or held["whole_residue"])
        with runs_of(ctx, run):
            assert ctx.info("sparse_run") == run
            for k, ref in off.items():
                got = ctx.dist_rows(estim=k[0], result_type=k[1])
                assert got.tobytes() == ref.tobytes(), (kind, n, p, run, k, "against the routes off")
                assert got.tobytes() == gathered[k].tobytes(), (kind, n, p, run, k, "against the gathered table")
                assert ctx.info("sparse_items") == len(items)
                assert ctx.info("sparse_table_fills") == want, (kind, n, p, run)
        fills[run] = want
    assert fills[1] == 4 * len(items)
    if n == 641:
        assert fills[8] < fills[1]
    assert ctx.info("sparse_run") >= 1  # (option 0 again: `info` reports the library's default as the run in effect)


def test_runs_hold_every_condition(host):
    """over the cases above: a run whose table slab changes inside it, a plain item followed by a transposed one of the same
    table slab, a ragged run, a run of a single item, and a whole residue in one run"""
    held = dict.fromkeys(("slab_change", "plain_then_transposed", "ragged", "single", "whole_residue"), False)
    same_slab = False
    for n, p in SIZES:
        for kind in KINDS:
            items = host_items(host, kind, n, p)
            for run in sr.RUNS:
                c = sr.conditions(items, run)
                assert not c["transposed_then_plain"]  # (the planner's order, see above)
                for k in held:
                    held[k] |= c[k]
                same_slab |= sr.fills(items, run) < 4 * len(items)
    assert all(held.values()) and same_slab, held


def test_call_forms_at_a_run_of_three(ctx):
    """a row range in the layout made for it, two and three parts, two bands (a band is a launch of its own: its end ends
    every run) and fragments beside routed planes: the bytes of the full call with the route off"""
    import torch

    n, p = 257, 14
    regs = case("mixed_thresholds", n, p)[0]
    ctx.set_sketches(regs)
    with sided(ctx, 0):
        full = ctx.dist_rows()
    rb, re = 37, n - 2
    a, b = dashing_amd.tri_span(n, 0, rb), dashing_amd.tri_span(n, 0, re)
    with runs_of(ctx, 3):
        assert ctx.dist_rows().tobytes() == full.tobytes() and ctx.info("sparse_transposed_items") > 0
    with runs_of(ctx, 3, range_sort_min_rows=1):
        assert ctx.dist_rows(rb, re).tobytes() == full[a:b].tobytes() and ctx.info("sparse_sided_items") > 0 and ctx.info("sorted") == 1
    dev = torch.device("cuda", 0)
    with runs_of(ctx, 3):
        for prb, pre, nparts in ((0, n, 2), (rb, re, 3)):
            a0, span = dashing_amd.tri_span(n, 0, prb), dashing_amd.tri_span(n, prb, pre)
            out = torch.full((span,), -3.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            ctx.dist_rows_parts_device_async(out.data_ptr(), prb, pre, nparts)
            ctx.wait()
            assert out.cpu().numpy().tobytes() == full[a0 : a0 + span].tobytes(), (prb, pre, nparts)
            assert ctx.info("sparse_sided_items") > 0
    with runs_of(ctx, 3, cum_budget_bytes=1 << 20):  # (a tile's C(v) is 32 KiB x planes: three tiles to a band)
        assert ctx.dist_rows().tobytes() == full.tobytes() and ctx.info("bands") >= 2 and ctx.info("sparse_sided_items") > 0
        assert ctx.info("sparse_table_fills") >= 4 * 2  # (every band stages for itself)
    with runs_of(ctx, 3, overflow_frag_permille=1000):
        assert ctx.dist_rows().tobytes() == full.tobytes() and ctx.info("frag_items") > 0 and ctx.info("sparse_sided_items") > 0
