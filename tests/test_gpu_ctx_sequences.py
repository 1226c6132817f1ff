"""GPU: one context walked through register mutations and changing call kinds (tests/ctx_model.py).  After every mutator
the touched rows and a neighbour on each side are downloaded and compared with the model bit for bit; every query is
compared with the CPU oracle evaluated on the model, and now and then with the same query on a fresh context that
received the model through set_sketches (equal bytes).  What is under test is what prepare() keeps between calls: the
per-sketch pass per estimator and the rows it covers, the bit-plane layout with its per-column data, the host copy of the
keys, buffers that only grow.

A failure prints the operations so far, one per line, in the form the directed tests below are written in."""
import os

import numpy as np
import pytest

import dashing_amd
from ctx_model import (OPTION_DEFAULTS, OPTION_DEFAULTS2, OPTION_VALUES, CtxQueries, Model, fasta_files, fmt, generate,
                       group_arrays, matrix, row, rows, run_query, sequences)  # (tests/ctx_model.py)

pytestmark = pytest.mark.gpu


def _query_behind_async(ops, x):
    """the query that follows ops[x] directly, if ops[x] is a sketch call in the asynchronous form; else None"""
    op = ops[x]
    if op[0] in ("sketch", "records") and op[1] == "async" and x + 1 < len(ops) and ops[x + 1][0] == "query":
        return ops[x + 1]
    return None


class Driver:
    """applies operations to the context and to the model, and checks one against the other"""

    def __init__(self, ctx, oracle, label=""):
        self.ctx, self.oracle, self.label = ctx, oracle, label
        self.Q = CtxQueries(ctx)
        self.model = Model()
        self.options = dict(OPTION_DEFAULTS, **OPTION_DEFAULTS2)
        self.fresh = None    # the second context (at most one per test)
        self.tensor = None   # the attached torch tensor
        self.pending = None  # (lo, hi, staging) of an asynchronous sketch call whose rows are still to be checked
        self.upcoming = None  # the query right behind the asynchronous sketch call that is about to be made
        self.done = []

    # ---- life cycle
    def close(self):
        try:
            if self.pending:
                self.ctx.wait()
            for name, v in dict(OPTION_DEFAULTS, **OPTION_DEFAULTS2).items():
                self.ctx.set_option(name, v)
            if self.tensor is not None:
                self.ctx.alloc(2, 10)  # the shared context must not keep a pointer into a tensor that is about to go
        finally:
            self.pending = self.tensor = None
            if self.fresh is not None:
                self.fresh.close()
                self.fresh = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self, ops):
        for x, op in enumerate(ops):
            self.done.append(op)
            # the query right behind an asynchronous sketch call follows it with no host wait: what its device form needs
            # from torch is allocated before the call (CtxQueries.reserve)
            self.upcoming = _query_behind_async(ops, x)
            try:
                self.step(op)
            except (AssertionError, dashing_amd.DshError) as e:
                raise AssertionError("%s: operation %d failed: %s: %s\noperations so far:\n%s"
                                     % (self.label, len(self.done), type(e).__name__, e, fmt(self.done))) from e

    # ---- one operation
    def step(self, op):
        if op[0] == "opt":
            self.ctx.set_option(op[1], op[2])
            self.options[op[1]] = op[2]
        elif op[0] == "query":
            self.query(op)
            self.flush()
        else:
            self.flush()
            if self.upcoming is not None:
                self.Q.reserve(self.upcoming)
            self.mutate(op)

    def flush(self):
        """the deferred register check of an asynchronous sketch call (download is in stream order behind it)"""
        if self.pending:
            lo, hi, _ = self.pending
            self.pending = None
            self.check_rows(lo, hi)

    def check_rows(self, lo, hi):
        a, b = max(lo - 1, 0), min(hi + 1, self.model.n)
        got = self.ctx.download(a, b - a)
        want = self.model.regs[a:b]
        assert got.tobytes() == want.tobytes(), "registers of rows %s differ from the model" % (
            (a + np.flatnonzero((got != want).any(axis=1))).tolist(),)

    def mutate(self, op):
        import torch

        ctx, t, p = self.ctx, op[0], self.model.p
        before = self.model.regs
        deferred = None
        if t == "alloc":
            ctx.alloc(op[1], op[2])
            self.tensor = None
        elif t == "set":
            ctx.set_sketches(matrix(op[1], op[2], op[3], op[4]))
            self.tensor = None
        elif t == "upload":
            ctx.upload(rows(op[2], p, before), op[1])
        elif t == "clear":
            ctx.clear(op[1], op[2])
        elif t in ("sketch", "records"):
            _, form, first, seed, lens, k, canon = op
            seq, off = sequences(seed, lens)
            if form == "sync":
                (ctx.sketch_batch if t == "sketch" else ctx.sketch_records)(seq, off, first, k, canon, want_regs=False)
            elif form == "async":  # no host wait: what follows on the context is in stream order behind it
                pin = dashing_amd.PinnedArray(seq.size + 64, np.uint8)
                pin.array[: seq.size] = seq
                (ctx.sketch_batch_async if t == "sketch" else ctx.sketch_records_async)(pin.array, off, first, k, canon)
                deferred = pin
            else:
                d = torch.zeros(seq.size + 256, dtype=torch.uint8, device="cuda")
                d[: seq.size] = torch.from_numpy(seq).to("cuda")
                torch.cuda.synchronize()
                (ctx.sketch_batch_device if t == "sketch" else ctx.sketch_records_device)(d.data_ptr(), off, first, k, canon)
                ctx.synchronize()
        elif t == "fastx":
            _, first, seed, lens_per_genome, width, k, canon = op
            status = ctx.sketch_fastx_batch(fasta_files(seed, lens_per_genome, width), first, k, canon)
            assert not status.any(), "plain FASTA was refused: %s" % (status.tolist(),)
        elif t == "attach":
            self.tensor = torch.from_numpy(matrix(op[1], op[2], op[3], op[4])).to("cuda")
            torch.cuda.synchronize()
            ctx.attach_device(self.tensor.data_ptr(), op[1], op[2])
        elif t == "reattach":
            assert self.tensor is not None
            for r, spec in op[1]:
                self.tensor[r] = torch.from_numpy(row(spec, p, before)).to("cuda")
            torch.cuda.synchronize()
            ctx.attach_device(self.tensor.data_ptr(), self.model.n, p)
        elif t == "upfold":
            _, form, first, src_p, specs = op
            src = rows(specs, src_p, None)
            if form == "host":
                ctx.upload_folded(src, src_p, first)
            else:
                d = torch.from_numpy(src).to("cuda")
                torch.cuda.synchronize()
                ctx.upload_folded_device(d.data_ptr(), src_p, len(specs), first)
        elif t == "unite":  # the unions into a buffer of the caller, and from there into the slots (src_p == p: a copy)
            _, first, groups = op
            gp, mem = group_arrays(groups, self.model.n)
            d = torch.full((len(groups) << p,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.union_groups_device(d.data_ptr(), gp, mem)
            ctx.upload_folded_device(d.data_ptr(), p, len(groups), first)
        else:
            raise AssertionError(op)
        lo, hi = self.model.apply(op, self.oracle)
        if deferred is not None:
            self.pending = (lo, hi, deferred)
        else:
            self.check_rows(lo, hi)

    def fresh_queries(self):
        """a second context holding the model and the options in effect"""
        if self.fresh is None:
            self.fresh = dashing_amd.Context(0)
        self.fresh.set_sketches(self.model.regs)
        for name, v in self.options.items():
            self.fresh.set_option(name, v)
        return CtxQueries(self.fresh)

    def query(self, op):
        kind, q = op[1], op[2]
        n = self.model.n
        if "refused" in q:  # an error return naming the sketch, never a wrong number
            with pytest.raises(dashing_amd.DshError) as e:
                self.Q.rows(0, n, q["estim"], q["rt"], q["k"])
            assert e.value.code == -22 and "sketch %d " % q["refused"] in str(e.value), str(e.value)
            return
        if q.get("may_refuse"):  # nothing is asserted about the outcome but the kind of error
            self.ctx.set_option("range_sort_min_rows", 1)
            try:
                self.Q.rows(q["rb"], q["re"], q["estim"], q["rt"], q["k"])
            except dashing_amd.DshError as e:
                assert e.code == -22
            finally:
                self.ctx.set_option("range_sort_min_rows", self.options["range_sort_min_rows"])
            return
        fresh = _Lazy(self.fresh_queries) if q.get("fresh") else None
        try:
            return run_query(self.Q, self.model.regs, op, self.oracle, self.options, fresh=fresh)
        finally:
            self.Q.release()


class _Lazy:
    """the second context, set up when it is first asked something: behind the first call on the context under test where
    that matters (its upload would otherwise stand between a mutator and that call)"""

    def __init__(self, make):
        self._make, self._q = make, None

    def __getattr__(self, name):
        if self._q is None:
            self._q = self._make()
        return getattr(self._q, name)


def Qy(kind, estim=2, rt=1, k=31, fresh=True, **kw):
    return ("query", kind, dict(estim=estim, rt=rt, k=k, fresh=fresh, **kw))


def play(ctx, oracle, ops, label="directed"):
    with Driver(ctx, oracle, label) as d:
        d.run(ops)


FAR = [("law", 901, 40), ("law", 902, 300_000_000), ("zero",), ("sat",), ("dup", 5)]  # rows far from anything in START
START = ("set", 200, 11, 4242, "related")  # cardinalities of 2e6..8e6


# ---- directed sequences: one cache key each

@pytest.mark.parametrize("new", FAR)
@pytest.mark.parametrize("rt", [1, 0])
def test_upload_of_one_row_between_two_triangles(ctx, oracle, new, rt):
    play(ctx, oracle, [START, Qy("tri", rt=rt), ("upload", 77, [new]), Qy("tri", rt=rt)])


@pytest.mark.parametrize("estim", [0, 1, 2])
def test_clear_of_two_rows_then_cardinalities_then_triangle(ctx, oracle, estim):
    play(ctx, oracle, [START, Qy("tri", estim=estim), ("clear", 30, 2), Qy("card", estim=estim), Qy("tri", estim=estim)])


@pytest.mark.parametrize("form", ["sync", "async", "device"])
@pytest.mark.parametrize("call", ["sketch", "records"])
def test_sketch_into_three_occupied_slots_between_two_triangles(ctx, oracle, call, form):
    """the merge / the overwrite changes three rows of a matrix whose layout and per-sketch pass are cached; with the
    asynchronous forms the triangle follows with no host wait in between (same stream: the kernels execute in order)"""
    lens = [50_000, 20, 900] if call == "records" else [50_000, 3_000, 900]  # (a record shorter than k: a zero row)
    play(ctx, oracle, [("set", 120, 12, 77, "law"), Qy("tri"), (call, form, 40, 321, lens, 31, True), Qy("tri"),
                       (call, form, 41, 322, lens, 21, False), Qy("card"), Qy("tri", rt=0)])


def test_fastx_into_occupied_slots_between_two_triangles(ctx, oracle):
    play(ctx, oracle, [("set", 60, 10, 78, "law"), Qy("tri"), ("fastx", 10, 555, [[4000, 300], [60], [20_000]], 60, 31, True),
                       Qy("tri"), Qy("knn_square", nn=4)])


@pytest.mark.parametrize("A,B", [(a, b) for a in range(3) for b in range(3) if a != b])
def test_cardinalities_and_distances_alternate_estimators(ctx, oracle, A, B):
    play(ctx, oracle, [("set", 150, 10, 5, "law"), Qy("card", estim=A), Qy("tri", estim=B), Qy("card", estim=A),
                       Qy("tri", estim=A), Qy("card", estim=B), ("upload", 9, [FAR[1]]), Qy("card", estim=B), Qy("tri", estim=A)])


_RANGES = [Qy("range_sorted", rb=120, re=300), Qy("card"), Qy("tri"), Qy("range_sorted", rb=40, re=300),
           Qy("rect", q0=0, q1=30, r0=100, r1=300), Qy("knn_band", nn=5), Qy("shard", G=3)]


@pytest.mark.parametrize("estim", [0, 2])
def test_key_ordered_ranges_then_calls_that_need_every_sketch(ctx, oracle, estim):
    """a key-ordered range [rb, n) with rb > 0 leaves a per-sketch pass that covers [rb, n) only: every later call that
    looks at a sketch before rb has to notice"""
    ops = [("set", 300, 12, 6, "law")] + [(o[0], o[1], dict(o[2], estim=estim)) for o in _RANGES]
    play(ctx, oracle, ops)


@pytest.mark.parametrize("estim", [0, 2])
def test_key_ordered_ranges_with_an_upload_before_the_range_between_calls(ctx, oracle, estim):
    ops = [("set", 300, 12, 6, "law")]
    for i, o in enumerate(_RANGES):
        ops += [(o[0], o[1], dict(o[2], estim=estim)), ("upload", 3 + 5 * i, [FAR[i % len(FAR)]])]
    ops += [Qy("range_sorted", rb=120, re=300, estim=estim), ("upload", 8, [("law", 1, 77)]),
            Qy("range_sorted", rb=120, re=300, estim=estim), Qy("range_sorted", rb=2, re=300, estim=estim)]
    play(ctx, oracle, ops)


def test_sizes_go_up_and_down(ctx, oracle):
    """buffers only grow: a small matrix after a large one runs in oversized buffers (the column index changes form at
    p = 12, list entries go from 2 to 4 bytes at p = 16)"""
    ops = []
    for n, p in ((400, 12), (40, 10), (500, 14), (3, 16), (40, 10)):
        ops += [("set", n, p, 100 + n, "law"), Qy("tri", rt=0), Qy("knn_band", nn=2), ("alloc", n, p),
                ("upload", 1, [("law", 5, 10_000), ("sat",)][: n - 1]), Qy("tri", estim=1)]
    play(ctx, oracle, ops)


def _answers(Q, n):
    out = [Q.rows(0, n, 2, 1, 31), Q.rows(60, n, 1, 0, 31), Q.parts(20, 180, 3, 0, 5, 21)]
    out += list(Q.knn(5, 0, n, 0, n, 2, 1, 31))
    return b"".join(x.tobytes() for x in out)


def test_speed_knobs_move_nothing(ctx, oracle):
    """every speed knob between two identical sets of queries with untouched registers: equal bytes; then the knob
    changed and one row uploaded: equal to the oracle and to a fresh context"""
    with Driver(ctx, oracle, "knobs") as d:
        d.run([START])
        base = _answers(d.Q, 200)
        for i, (name, values) in enumerate(sorted(OPTION_VALUES.items())):
            for v in values:
                d.run([("opt", name, v)])
                assert _answers(d.Q, 200) == base, "option %s = %d changed a result" % (name, v)
            d.run([("upload", 11 * i, [FAR[i % len(FAR)]]), Qy("tri", rt=0), Qy("range_sorted", rb=60, re=200), Qy("parts", rb=20, re=180, nparts=3),
                   Qy("knn_band", nn=5), Qy("knn_square", nn=5), ("opt", name, OPTION_DEFAULTS[name])])
            base = _answers(d.Q, 200)


def test_a_register_out_of_range_is_refused_until_repaired(ctx, oracle):
    p = 12
    bad = ("bad", 9, 5_000_000, 1234, 64 - p + 2)
    play(ctx, oracle, [("set", 40, p, 3, "related"), Qy("tri"), ("upload", 17, [bad]), Qy("tri", refused=17),
                       Qy("range_sorted", rb=20, re=40, may_refuse=True), Qy("tri", refused=17), Qy("tri", estim=0, refused=17),
                       ("upload", 17, [("law", 9, 5_000_000)]), Qy("tri"), Qy("tri", estim=0)])


def test_attached_tensor_changed_and_attached_again(ctx, oracle):
    play(ctx, oracle, [("attach", 150, 11, 8, "related"), Qy("tri"), Qy("card", estim=0),
                       ("reattach", [(3, FAR[0]), (50, FAR[1]), (51, FAR[2]), (52, FAR[3]), (149, FAR[4])]),
                       Qy("tri"), Qy("card", estim=0), Qy("knn_square", nn=3), ("set", 150, 11, 9, "law"), Qy("tri")])


# ---- random sequences

@pytest.mark.parametrize("case", range(int(os.environ.get("DSH_SEQ_FIRST", "0")),
                                       int(os.environ.get("DSH_SEQ_FIRST", "0")) + int(os.environ.get("DSH_SEQ_CASES", "40"))))
def test_random_sequence(ctx, oracle, case):
    play(ctx, oracle, generate(case), "random case %d (seed 0x5E0000 + %d)" % (case, case))
