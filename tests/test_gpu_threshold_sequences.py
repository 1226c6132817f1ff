"""GPU: dist_threshold after register mutations of one context (tests/ctx_model.py, read-only; the driver of
tests/test_gpu_ctx_sequences.py applies the mutators and checks the touched rows).  After every mutator the thresholded
triangle is compared with the oracle evaluated on the model under the undecided-pairs rule of tests/test_gpu_threshold.py,
with the dense path of the same context bit for bit, and it is interleaved with dist_rows_async + wait: the buffers of
the two paths do not collide."""
import numpy as np
import pytest

import dashing_amd
import thr_ref
from test_gpu_ctx_sequences import START, Driver
from test_gpu_threshold import compare_with_oracle

pytestmark = pytest.mark.gpu


def check(d, estim, rt, k, t, rb=0, re=None):
    ctx, regs = d.ctx, d.model.regs
    n = regs.shape[0]
    re = n if re is None else re
    span = dashing_amd.tri_span(n, rb, re)
    pin = dashing_amd.PinnedArray(max(span, 1), np.float32)
    ctx.dist_rows_async(pin.array, rb, re, estim=estim, result_type=rt, k=k)  # its copy may still run while ...
    got = ctx.dist_threshold(t, rb, re, estim=estim, result_type=rt, k=k)     # ... the selection computes its band
    ctx.wait()
    dense = pin.array[:span].copy()
    assert thr_ref.same(got, thr_ref.tri(dense, n, rb, re, t, rt))
    want = d.oracle.dist_tri(regs, estim, rt, k)
    lo = dashing_amd.tri_span(n, 0, rb)
    compare_with_oracle(got, want[lo : lo + span], n, rb, re, t, rt)
    ctx.dist_rows_async(pin.array, rb, re, estim=estim, result_type=rt, k=k)
    ctx.wait()
    assert pin.array[:span].tobytes() == dense.tobytes()
    return got


def play(ctx, oracle, steps):
    with Driver(ctx, oracle, "threshold") as d:
        for s in steps:
            if s[0] == "thr":
                check(d, *s[1:])
            elif s[0] == "card":
                got, want = ctx.cardinalities(s[1]), oracle.cardinalities(d.model.regs, s[1])
                fin = np.isfinite(want)
                assert np.allclose(got[fin], want[fin], rtol=1e-12, atol=0)
            else:
                d.done.append(s)
                d.step(s)


@pytest.mark.parametrize("rt,t", [(1, 0.04), (0, 0.12)])
def test_upload_of_one_row(ctx, oracle, rt, t):
    play(ctx, oracle, [START, ("thr", 2, rt, 31, t), ("upload", 77, [("dup", 5)]), ("thr", 2, rt, 31, t),
                       ("upload", 78, [("zero",)]), ("thr", 2, rt, 31, t), ("thr", 2, rt, 31, t, 60, 90)])


@pytest.mark.parametrize("estim", [0, 1, 2])
def test_clear_of_two_rows_and_another_estimator_between(ctx, oracle, estim):
    other = (estim + 1) % 3
    play(ctx, oracle, [START, ("thr", estim, 1, 31, 0.04), ("clear", 30, 2), ("card", other), ("thr", estim, 1, 31, 0.04),
                       ("card", estim), ("thr", other, 0, 21, 0.12)])


@pytest.mark.parametrize("call", ["sketch", "records"])
def test_sketch_into_occupied_slots(ctx, oracle, call):
    lens = [50_000, 20, 900] if call == "records" else [50_000, 3_000, 900]
    play(ctx, oracle, [("set", 120, 12, 77, "law"), ("thr", 2, 1, 31, 0.04), (call, "sync", 40, 321, lens, 31, True),
                       ("thr", 2, 1, 31, 0.04), (call, "async", 41, 322, lens, 21, False), ("thr", 2, 0, 31, 0.12)])
