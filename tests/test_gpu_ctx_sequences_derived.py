"""GPU: the calls that came after tests/test_gpu_ctx_sequences.py -- thresholded hits, pair lists, derived sketches (fold,
union by groups, folded upload), threshold clusters, greedy representatives -- as further call kinds of ONE long-lived
context (the second table of tests/ctx_model.py; the driver is the one of tests/test_gpu_ctx_sequences.py).  What is under
test is what these calls keep between calls and a fresh context never exercises: the band buffer the three threshold
paths share, each under a band rule of its own; label buffers and the union-find array, which only grow; the scratch the
host forms of fold and union share and the partial buffer of a union that cuts a group into chunks (groups hold at most
300 members here, so a union has two levels and uses the first of its two partial buffers); that a folded upload drops the
derived compare state like any other writer; and what the entry points see of an attached tensor and of rows a pending
asynchronous sketch call is still writing.

Registers, hits, pair values and labels have one answer: every comparison of them is exact.  The only tolerances are the
two the suite has between device and oracle VALUES (ctx_model._close, test_gpu_threshold.compare_with_oracle)."""
import os
import time

import numpy as np
import pytest

import dashing_amd
import thr_ref
from ctx_model import (OPTION_DEFAULTS2, OPTION_VALUES2, _oracle_graph, generate2, group_arrays, pair_list, rows)  # (tests/ctx_model.py)
from test_gpu_ctx_sequences import FAR, START, Driver, Qy, play

pytestmark = pytest.mark.gpu

ESTATE = -11
# START under JI (Ertl MLE, k = 31): families of ten sketches.  The oracle's values leave a gap of 0.075 around 0.6346
# (no value within 0.037 of it, 1 % of the pairs above): the components are {0, 1, 5, 6}, {10, 11, 15, 16}, ... and
# the singletons, and slot 0, 10, ... represents its component in the greedy pass as well.
T_JI = 0.6346


def L(kind, frac="1%", form="host", misalign=0, **kw):
    return Qy(kind, frac=frac, form=form, misalign=misalign, **kw)


def big_group(n):
    """150 members: more than a union level takes in one piece (64), so the group is cut and its parts united again"""
    return [(7 * x + 3) % n for x in range(150)]


BIG = big_group(200)


# ---- directed sequences: one cache key each

@pytest.mark.parametrize("new", FAR)
@pytest.mark.parametrize("kind", ["cluster", "greedy"])
def test_upload_of_one_row_between_two_label_queries(ctx, oracle, kind, new):
    """slot 75 sits in {70, 71, 75, 76}; a copy of sketch 5 uploaded there joins {0, 1, 5, 6}, an empty sketch leaves"""
    with Driver(ctx, oracle, "labels around an upload") as d:
        d.run([START, L(kind), L(kind, frac="1/n", form="device", misalign=1)])
        before = getattr(d.Q, kind)(T_JI, 2, 1, 31, "host")[0]
        assert before[75] == 70 and before[5] == 0
        d.run([("upload", 75, [new]), L(kind), L(kind, frac="1/n", form="device", misalign=3)])
        ov = oracle.dist_tri(d.model.regs, 2, 1, 31)
        assert not thr_ref.undecided(ov, T_JI).any()
        after, cnt = getattr(d.Q, kind)(T_JI, 2, 1, 31, "host")
        if new == ("dup", 5):
            assert after[75] == 0 and (after == 0).sum() == 5 and (after == 70).sum() == 3
        else:  # far from everything (the empty and the saturated sketch: no finite value at all)
            assert after[75] == 75 and (after == 75).sum() == 1 and (after == 70).sum() == 3
        assert cnt == int((before == np.arange(200)).sum()) + (0 if new == ("dup", 5) else 1)


@pytest.mark.parametrize("rt", [1, 0])
def test_hits_then_representatives_then_clusters_then_hits(ctx, oracle, rt):
    """the three users of the band buffer one after the other at the same threshold, the middle two with many small
    bands: the hits before and after are the same"""
    with Driver(ctx, oracle, "shared band buffer") as d:
        thr = Qy("thr", rt=rt, rb=0, re=200, frac="1%")
        d.run([START])
        d.done.append(thr)
        first = d.query(thr)
        d.run([("opt", "threshold_band_bytes", 64 << 10), ("opt", "greedy_band_rows", 7), L("greedy", rt=rt), L("cluster", rt=rt),
               ("opt", "threshold_band_bytes", 1 << 30), ("opt", "greedy_band_rows", 4096)])
        d.done.append(thr)
        again = d.query(thr)
        assert first[1].size > 0 and thr_ref.same(again, first)


def test_sizes_go_up_and_down(ctx, oracle):
    """label buffers, the union-find array, the band buffer and the derive scratch only grow: a small matrix after a large
    one runs in oversized buffers, a larger one has them allocated again"""
    ops = []
    for n, p in ((400, 12), (40, 10), (500, 14), (3, 16), (40, 10)):
        ops += [("set", n, p, 100 + n, "related"), L("cluster", frac="1/n"), L("greedy"),  # (host forms: the library's label buffers)
                Qy("fold", new_p=p - 4, first=0, cnt=n, form="host"), Qy("union", groups=[big_group(n), [], [n - 1]], form="device"),
                Qy("fold", new_p=p - 4, first=1, cnt=n - 1, form="device", fresh=False),
                Qy("union", groups=[[0], big_group(n)], form="host", fresh=False)]
    play(ctx, oracle, ops)


def test_derive_scratch_is_reused_across_shapes(ctx, oracle):
    """the host forms of fold and union share one output scratch: a fold in chunks of one row, a union, a fold again, at
    (40, 14) and then at (300, 8)"""
    ops = []
    for n, p in ((40, 14), (300, 8)):
        ops += [("set", n, p, 7 + n, "law"), ("opt", "derive_chunk_bytes", 1), Qy("fold", new_p=p - 3, first=0, cnt=n, form="host"),
                Qy("union", groups=[big_group(n), [1, 2], []], form="host"), Qy("fold", new_p=4, first=2, cnt=n - 3, form="host"),
                ("opt", "derive_chunk_bytes", 1 << 14), Qy("fold", new_p=p, first=0, cnt=n, form="host"),
                Qy("union", groups=[[x] for x in range(n)], form="host", fresh=False)]
    play(ctx, oracle, ops)


_SIX = [("law", 11, 5_000), ("zero",), ("sat",), ("uni", 12), ("law", 13, 200_000_000), ("law", 14, 40)]


@pytest.mark.parametrize("estim", [0, 2])
@pytest.mark.parametrize("form", ["host", "device"])
def test_folded_upload_after_a_key_ordered_range(ctx, oracle, form, estim):
    """a key-ordered range [120, n) leaves a per-sketch pass that covers [120, n) only and a layout of those rows; the
    folded upload (14 -> 10) of slots 5..10 has to drop both like any other writer"""
    play(ctx, oracle, [("set", 300, 10, 6, "law"), Qy("range_sorted", rb=120, re=300, estim=estim), Qy("card", estim=estim),
                       Qy("range_sorted", rb=120, re=300, estim=estim), ("upfold", form, 5, 14, _SIX), Qy("tri", estim=estim),
                       Qy("card", estim=0), Qy("card", estim=1), Qy("card", estim=2), Qy("knn_band", nn=5, estim=estim),
                       Qy("range_sorted", rb=120, re=300, estim=estim), ("upfold", form, 150, 10, _SIX),
                       Qy("range_sorted", rb=120, re=300, estim=estim), Qy("tri", estim=estim, rt=0)])


def test_attached_tensor_then_changed_and_attached_again(ctx, oracle):
    """fold and union read the attached tensor, the label calls compare it; a folded upload writes only into a matrix of
    the library's own and is refused"""
    four = [Qy("fold", new_p=7, first=3, cnt=140, form="device"), Qy("union", groups=[big_group(150), [149, 3]], form="host"),
            L("cluster"), L("greedy", form="device")]
    with Driver(ctx, oracle, "attached") as d:
        d.run([("attach", 150, 11, 8, "related")] + four +
              [("reattach", [(3, FAR[0]), (50, FAR[1]), (51, FAR[2]), (52, FAR[3]), (149, FAR[4])])] + four)
        src = rows([("law", 1, 1000), ("sat",)], 13, None)
        import torch

        dev = torch.from_numpy(src).to("cuda")
        torch.cuda.synchronize()
        for call in (lambda: ctx.upload_folded(src, 13, 3), lambda: ctx.upload_folded_device(dev.data_ptr(), 13, 2, 3),
                     lambda: ctx.upload_folded(src[:, :2048].copy(), 11, 3)):
            with pytest.raises(dashing_amd.DshError) as e:
                call()
            assert e.value.code == ESTATE
        assert d.tensor.cpu().numpy().tobytes() == d.model.regs.tobytes()
        d.check_rows(0, 150)
        d.run(four + [Qy("tri")])


_PENDING = [Qy("fold", new_p=9, first=38, cnt=8, form="host"), Qy("fold", new_p=12, first=0, cnt=120, form="device"),
            Qy("union", groups=[big_group(120)], form="host"), Qy("union", groups=[[40, 41, 42], [43, 0]], form="device"),
            L("cluster"), L("cluster", form="device", misalign=3), L("greedy"), L("greedy", form="device", misalign=1),
            L("cluster", rt=0, frac="1/n"), L("greedy", rt=0, frac="1/n"),
            Qy("thr", rb=0, re=120, frac="1%"), Qy("pairs", seed=3, m=500)]


@pytest.mark.parametrize("x", range(len(_PENDING)))
@pytest.mark.parametrize("call", ["sketch", "records"])
def test_rows_of_a_pending_asynchronous_sketch_call(ctx, oracle, call, x):
    """No host wait and no other call on the context between the asynchronous sketch call and the call under test, which
    must see the sketched rows (same stream).  The driver allocates what a device form needs from torch before the
    sketch call; the label and hit calls run first at a threshold inside a gap of the ORACLE's values of the model (the
    query must find one: asserted), and only then the dense triangle.  The registers are compared after the query."""
    lens = {"sketch": [50_000, 3_000, 900], "records": [50_000, 20, 900]}[call]
    q = _PENDING[x]
    with Driver(ctx, oracle, "pending") as d:
        d.run([("set", 120, 12, 77, "law"), Qy("tri"), (call, "async", 40, 321 + x, lens, (31, 21)[x % 2], bool(x % 3)), q])
        if q[1] in ("cluster", "greedy", "thr"):
            ov = oracle.dist_tri(d.model.regs, q[2]["estim"], q[2]["rt"], q[2]["k"])
            iw = oracle.dist_tri(d.model.regs, q[2]["estim"], 1, q[2]["k"]) if q[2]["rt"] == 0 else None
            assert _oracle_graph(ov, iw, q[2]["frac"], q[2]["rt"], q[2]["k"], 120, [], q[1]) is not None


def test_unions_into_occupied_slots_between_two_triangles(ctx, oracle):
    play(ctx, oracle, [START, Qy("tri"), ("unite", 75, [[5, 75], BIG, [], [78]]), Qy("tri"), L("greedy"),
                       ("unite", 0, [[199], [0, 1]]), L("cluster", frac="1/n"), Qy("tri", rt=0), Qy("card", estim=0)])


def _answers(Q, n):
    gp, mem = group_arrays([BIG, [], [3, 4]], n)
    lhs, rhs = pair_list(5, 1500, n)
    out = list(Q.cluster(T_JI, 2, 1, 31, "host")) + list(Q.greedy(T_JI, 2, 1, 31, "host")) + list(Q.greedy(0.1, 1, 0, 21, "host"))
    hits = Q.thr(T_JI, 0, n, 2, 1, 31)
    out += list(hits) + list(Q.thr(0.1, 60, n, 1, 0, 21)) + list(Q.cluster_of_hits(hits[0], hits[1]))
    out += [Q.fold(7, 10, 150, "host"), Q.union(gp, mem, "host"), Q.pairs(lhs, rhs, 2, 5, 31)]
    return b"".join(np.asarray(x).tobytes() for x in out)


def test_the_new_speed_knobs_move_nothing(ctx, oracle):
    """every value of the four knobs between identical sets of calls on untouched registers: equal bytes; then the knob
    left as it is and one row uploaded: equal to the references"""
    with Driver(ctx, oracle, "knobs") as d:
        d.run([START])
        base = _answers(d.Q, 200)
        for i, (name, values) in enumerate(sorted(OPTION_VALUES2.items())):
            for v in values:
                d.run([("opt", name, v)])
                assert _answers(d.Q, 200) == base, "option %s = %d changed a result" % (name, v)
            d.run([("opt", name, values[0]), ("upload", 75 + 10 * i, [FAR[(i + 4) % len(FAR)]]), L("cluster"), L("greedy", form="device"),
                   Qy("thr", rb=60, re=200, frac="1%"), Qy("fold", new_p=7, first=10, cnt=150, form="host"),
                   Qy("union", groups=[BIG, [75 + 10 * i]], form="host"), Qy("pairs", seed=9, m=1500),
                   ("opt", name, OPTION_DEFAULTS2[name])])
            base = _answers(d.Q, 200)


# ---- random sequences over both tables

@pytest.mark.parametrize("case", range(int(os.environ.get("DSH_SEQ2_FIRST", "0")),
                                       int(os.environ.get("DSH_SEQ2_FIRST", "0")) + int(os.environ.get("DSH_SEQ2_CASES", "30"))))
def test_random_sequence2(ctx, oracle, case):
    t0 = time.time()
    play(ctx, oracle, generate2(case), "random case %d (seed 0x5E2000 + %d)" % (case, case))
    print("case %d: %.1f s" % (case, time.time() - t0))
