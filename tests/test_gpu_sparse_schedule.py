"""The schedule of the sparse routes on the device (engine.hip, run_pairs): the sparse items of a call are emitted and
ordered BEHIND the first band's tile kernel, their slabs and the items travel then, and every band's counting kernel runs
behind its tile kernel -- both fill the band's C(v), k_finalize reads both.  What can go wrong is the order of things, not a
kernel, so the collections are small and the settings are those that give the schedule something to do: both routes forced
(sparse_planes = 2, sparse_sided = 1) and cum_budget_bytes = 1 MiB, under which the six tiles of three blocks fall into three
or six bands.

Every test asserts from the info keys that the call had several bands and sparse items, that its bytes are those of the same
context with both routes off, and (once per collection) that those are within the suite's 1e-6 of the oracle.  The call forms:
the blocking call, three parts (signalled and with finalize_signal = 0), two calls back to back without a synchronisation
between them, a call after sparse_cap changed, and collections whose first band routes nothing while a later one does and
the reverse -- a condition on the plan, asserted on the host (dshh_plan_sparse_items) before the device runs."""
import functools

import numpy as np
import pytest

import dashing_amd
from dashing_amd import synth

import path_cases
import sparse_cases as sc
import sparse_order_ref as ref
from sparse_cases import pcs
from test_gpu_sparse_planes import close, routed

pytestmark = pytest.mark.gpu
BUDGET = 1 << 20
SIZES = ((257, 14), (300, 14), (257, 13), (257, 16))  # (p = 16: the gathered counting kernel)


@functools.lru_cache(maxsize=None)
def related(n, p):
    r = np.ascontiguousarray(synth.related_sketches(n, p, seed=0x5C4ED + 131 * p + n)[0], np.uint8)
    r.setflags(write=False)
    return r


class scheduled(routed):
    """both routes forced (or both off) under the small C(v) budget, put back behind the block"""

    def __init__(self, ctx, on, cap=None, **more):
        routed.__init__(self, ctx, 2 if on else 0, cap, sparse_sided=1 if on else 0, cum_budget_bytes=BUDGET, **more)
        self.defaults.update(sparse_sided=-1, finalize_signal=-1)


def reference(ctx, oracle, regs, what):
    """the triangle with both routes off (the same bands), held to the oracle"""
    ctx.set_sketches(regs)
    with scheduled(ctx, False):
        off = ctx.dist_rows()
        assert ctx.info("sparse_items") == 0 and ctx.info("bands") >= 2
    close(off, oracle.dist_tri(regs, dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI, 31), what)
    return off


def routed_in_bands(ctx):
    assert ctx.info("bands") >= 2 and ctx.info("sparse_items") > 0 and ctx.info("sparse_sided_items") > 0, (ctx.info("bands"), ctx.info("sparse_items"))


@pytest.mark.parametrize("n,p", SIZES)
def test_blocking_call_and_parts(ctx, oracle, n, p):
    import torch

    regs = related(n, p)
    off = reference(ctx, oracle, regs, (n, p))
    with scheduled(ctx, True):
        assert ctx.dist_rows().tobytes() == off.tobytes(), (n, p)
        routed_in_bands(ctx)
    dev = torch.device("cuda", 0)
    for signal in (-1, 0):
        with scheduled(ctx, True, finalize_signal=signal):
            out = torch.full((len(off),), -3.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            ctx.dist_rows_parts_device_async(out.data_ptr(), 0, n, 3)
            ctx.wait()
            routed_in_bands(ctx)
            if signal == 0:
                assert ctx.info("parts_signalled") == 0
            assert out.cpu().numpy().tobytes() == off.tobytes(), (n, p, signal)


@pytest.mark.parametrize("n,p", ((257, 14), (257, 16)))
def test_two_calls_back_to_back(ctx, oracle, n, p):
    """no synchronisation between them: the second call plans, stages and emits while the first one's kernels run, and
    finds the slabs of the first in place"""
    import torch

    regs = related(n, p)
    off = reference(ctx, oracle, regs, (n, p))
    dev = torch.device("cuda", 0)
    with scheduled(ctx, True):
        outs = [torch.full((len(off),), -3.0, dtype=torch.float32, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        for out in outs:
            ctx.dist_rows_device_async(out.data_ptr())
        ctx.wait()
        routed_in_bands(ctx)
        for out in outs:
            assert out.cpu().numpy().tobytes() == off.tobytes(), (n, p)


def test_call_after_the_cap_changed(ctx, oracle):
    """the slabs in place were built at another cap: they are built again.  (The thresholds of the sided route are the
    per-sketch pass's, so at the second cap the two-plane route plans the items: tests/test_gpu_sparse_sided.py)"""
    n, p = 257, 14
    regs = related(n, p)
    off = reference(ctx, oracle, regs, (n, p))
    for cap in (pcs.SPARSE_CAP, 2040, pcs.SPARSE_CAP):
        with scheduled(ctx, True, cap=cap):
            assert ctx.dist_rows().tobytes() == off.tobytes(), cap
            assert ctx.info("bands") >= 2 and ctx.info("sparse_items") > 0, cap
            assert (ctx.info("sparse_sided_items") > 0) == (cap == pcs.SPARSE_CAP), cap


def band_items(regs, p):
    """the sparse items of every band of the forced plan, from the host planner"""
    keys, gcnt = sc.keys_and_counts(regs, p)
    vU, vA = pcs.sided_thresholds(regs, pcs.SPARSE_CAP)
    pl = ref.plan(ref.load(), keys, gcnt, vU.astype(np.uint32) | (vA.astype(np.uint32) << 8), p, thr_cap=pcs.SPARSE_CAP, budget=BUDGET, sp=2, sd=1)
    return [int(b[3] - b[2]) for b in pl["bands"]]


@pytest.mark.parametrize("family,n,first_routes", (("mixed", 300, False), ("mixed_high", 257, True)))
def test_bands_that_route_nothing(ctx, oracle, family, n, first_routes):
    """mixed: the key order puts the empty sketches first, so the first band's tile has no plane at all and the emission
    (which runs behind that band's tile kernel) serves later bands only.  mixed_high: the first band routes and a later
    one has nothing to count"""
    p = 14
    regs = path_cases.Case(family, p, n).regs()
    per_band = band_items(regs, p)
    if first_routes:
        assert per_band[0] > 0 and 0 in per_band[1:] and sum(per_band[1:]) > 0, per_band
    else:
        assert per_band[0] == 0 and max(per_band[1:]) > 0, per_band
    off = reference(ctx, oracle, regs, (family, n))
    with scheduled(ctx, True):
        assert ctx.dist_rows().tobytes() == off.tobytes(), family
        routed_in_bands(ctx)
        assert ctx.info("bands") == len(per_band) and ctx.info("sparse_items") == sum(per_band), (per_band, ctx.info("bands"), ctx.info("sparse_items"))
