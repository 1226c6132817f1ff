"""CPU: the helper of the sequence tests (tests/ctx_model.py) -- that the model is right, and that the random sequences
of tests/test_gpu_ctx_sequences.py cannot pass by not looking: the conditions below are evaluated on the generator's output
for the seeds the GPU test uses, without a GPU."""
import numpy as np
import pytest

from ctx_model import (INDEX_OF, MUTATOR_KINDS, OPTION_DEFAULTS, QUERY_KINDS, STEPS, Model, fasta_files, fasta_reference,
                       generate, max_n, run_query, sequences, walk)  # (tests/ctx_model.py)
from dashing_amd import synth

CASES = 40  # the default of DSH_SEQ_CASES


@pytest.fixture(scope="module")
def walked():
    return [w for case in range(CASES) for w in walk(generate(case))]


def test_generator_is_deterministic_and_well_formed():
    for case in (0, 7, 39):
        ops = generate(case)
        assert ops == generate(case)
        assert sum(op[0] == "query" for op in ops) == STEPS
        n = p = None
        attached = False
        for op in ops:
            t = op[0]
            if t in ("alloc", "set", "attach"):
                n, p = op[1], op[2]
                assert 2 <= n <= max_n(p)
                attached = t == "attach"
            elif t == "reattach":
                assert attached and all(0 <= r < n for r, _ in op[1])
            elif t in ("upload", "clear", "sketch", "records", "fastx"):
                assert not attached  # the library writes only into a matrix of its own
                first = op[1] if t in ("upload", "clear", "fastx") else op[2]
                cnt = op[2] if t == "clear" else len(op[2] if t == "upload" else (op[3] if t == "fastx" else op[4]))
                assert 0 <= first and first + cnt <= n and 1 <= cnt < n, op  # a strict sub-range
                if t in ("sketch", "records", "fastx"):
                    lens = op[4] if t != "fastx" else [x for g in op[3] for x in g]
                    assert all(x <= 60000 for x in lens) and (t == "records" or all(x >= 50 for x in lens))
            elif t == "query":
                q = op[2]
                for a, b in (("rb", "re"), ("q0", "q1"), ("r0", "r1")):
                    if a in q:
                        assert 0 <= q[a] <= q[b] <= n
                if "nn" in q:
                    assert 1 <= q["nn"] <= n - 1


def test_every_transition_occurs(walked):
    """every ordered pair (previous query kind, next query kind), and every pair (kind of the last register mutator since
    the previous query, next query kind), occurs in the cases the GPU test runs by default"""
    qq = {(prev, kind) for kind, prev, _, _, _ in walked if prev is not None}
    mq = {(mut, kind) for kind, _, mut, _, _ in walked if mut is not None}
    assert not [(a, b) for a in QUERY_KINDS for b in QUERY_KINDS if (a, b) not in qq]
    assert not [(a, b) for a in MUTATOR_KINDS for b in QUERY_KINDS if (a, b) not in mq]


def test_most_queries_have_caches_to_get_wrong(walked):
    """at least half of all queries come after a register mutation that followed an earlier query on the same (n, p)"""
    hot = sum(1 for w in walked if w[3])
    assert len(walked) == CASES * STEPS and 2 * hot >= len(walked), (hot, len(walked))


def test_consecutive_queries_change_the_estimator_about_two_times_in_three():
    diff = tot = 0
    for case in range(CASES):
        e = [w[4] for w in walk(generate(case))]
        diff += sum(a != b for a, b in zip(e, e[1:]))
        tot += len(e) - 1
    assert 0.6 <= diff / tot <= 0.73, diff / tot


def test_every_option_and_every_sketch_form_is_drawn():
    ops = [op for case in range(CASES) for op in generate(case)]
    assert {op[1] for op in ops if op[0] == "opt"} == set(OPTION_DEFAULTS)
    assert {(op[0], op[1]) for op in ops if op[0] in ("sketch", "records")} == {(a, b) for a in ("sketch", "records") for b in ("sync", "async", "device")}
    specs = [s[0] for op in ops if op[0] == "upload" for s in op[2]] + [s[0] for op in ops if op[0] == "reattach" for _, s in op[1]]
    assert {"law", "zero", "sat", "dup"} <= set(specs)
    assert any(x < op[5] for op in ops if op[0] == "records" for x in op[4])  # records shorter than k
    assert any(op[2].get("fresh") for op in ops if op[0] == "query")


class OracleQueries:
    """the query kinds answered by the oracle itself: runs the comparison code of run_query without a GPU"""

    def __init__(self, oracle, model):
        self.o, self.m = oracle, model

    def card(self, estim):
        return self.o.cardinalities(self.m.regs, estim)

    def rows(self, rb, re, estim, rt, k):
        return self.o.dist_rows(self.m.regs, rb, re, estim, rt, k)

    def rect(self, q0, q1, r0, r1, estim, rt, k):
        if q1 == q0 or r1 == r0:
            return np.zeros((q1 - q0, r1 - r0), np.float32)
        return self.o.dist_rect(self.m.regs[q0:q1], self.m.regs[r0:r1], estim, rt, k)

    def knn(self, nn, q0, q1, r0, r1, estim, rt, k):
        return self.o.knn(self.m.regs, nn, q0, q1, r0, r1, estim=estim, result_type=rt, k=k)

    def shard(self, G, estim, rt, k):
        return self.o.dist_tri(self.m.regs, estim, rt, k)

    def parts(self, rb, re, nparts, estim, rt, k):
        return self.o.dist_rows(self.m.regs, rb, re, estim, rt, k)

    def set_option(self, name, value):
        pass


@pytest.mark.parametrize("case", [1, 2])
def test_a_distance_is_never_compared_without_its_full_index(oracle, case):
    """whenever a distance measure is compared under the index-0 rule, the underlying index measure is compared in the
    same step on all pairs with nothing left out"""
    model = Model()
    log = []
    for op in generate(case):
        if op[0] == "query":
            before = len(log)
            run_query(OracleQueries(oracle, model), model.regs, op, oracle, OPTION_DEFAULTS, log)
            step = log[before:]
            kind, q = op[1], op[2]
            if kind == "card" or kind.startswith("knn"):
                assert len(step) == 1 and step[0][0] in ("card", "knn")
            elif q["rt"] in INDEX_OF:
                (a, irt, isize), (b, rt, with_index, size) = step
                assert (a, b) == ("index_full", "close") and irt == INDEX_OF[rt] and rt == q["rt"] and with_index and isize == size
            else:
                assert len(step) == 1 and step[0][:3] == ("close", q["rt"], False)
        else:
            model.apply(op, oracle)
    assert any(e[0] == "index_full" for e in log)


@pytest.mark.parametrize("p", [8, 12, 16])
def test_the_model_is_right(oracle, p):
    """merge = the oracle's sketch of the two inputs joined by an 'N' (k-mers do not span it); overwrite = the oracle's
    sketch of the record alone; a zero row has cardinality 0 under all three estimators"""
    k = 21
    m = Model()
    m.apply(("alloc", 6, p), oracle)
    a = ("sketch", "sync", 1, 160, [30_000, 700, 50], k, True)
    b = ("sketch", "sync", 1, 161, [9_000, 60_000, 5_000], k, True)
    m.apply(a, oracle)
    m.apply(b, oracle)
    sa, oa = sequences(a[3], a[4])
    sb, ob = sequences(b[3], b[4])
    joined = [np.concatenate([sa[int(oa[i]) : int(oa[i + 1])], [ord("N")], sb[int(ob[i]) : int(ob[i + 1])]]).astype(np.uint8) for i in range(3)]
    want = oracle.sketch_batch(*synth.concat_for_device(joined), k, p, True)
    assert (m.regs[1:4] == want).all() and not m.regs[0].any() and not m.regs[4:].any()
    # a FASTA file merges like the sequence kseq hands the encoder
    fx = ("fastx", 2, 162, [[2_000, 80], [500]], 60, k, True)
    before = m.regs.copy()
    m.apply(fx, oracle)
    fs, fo = fasta_reference(fasta_files(fx[2], fx[3], fx[4]))
    assert (m.regs[2:4] == np.maximum(before[2:4], oracle.sketch_batch(fs, fo, k, p, True))).all()
    assert (m.regs[2:4] != before[2:4]).any()
    # overwrite
    r = ("records", "sync", 3, 163, [4_000, k - 1, 100], k, False)
    m.apply(r, oracle)
    sr, orr = sequences(r[3], r[4])
    for i in range(3):
        alone = oracle.sketch_batch(sr[int(orr[i]) : int(orr[i + 1])], np.array([0, r[4][i]], np.uint64), k, p, False)[0]
        assert (m.regs[3 + i] == alone).all()
    assert not m.regs[4].any() and m.regs[3].any() and m.regs[5].any()
    for estim in (0, 1, 2):
        c = oracle.cardinalities(m.regs, estim)
        assert c[0] == 0 and c[4] == 0 and (c[[1, 2, 3, 5]] > 0).all()
    # rows by recipe: assigned in place, neighbours untouched; a duplicate copies the matrix BEFORE the operation
    before = m.regs.copy()
    lo, hi = m.apply(("upload", 2, [("dup", 3), ("sat",), ("zero",)]), oracle)
    assert (lo, hi) == (2, 5) and (m.regs[2] == before[3]).all() and (m.regs[3] == 64 - p + 1).all() and not m.regs[4].any()
    assert (m.regs[[0, 1, 5]] == before[[0, 1, 5]]).all()
    assert m.apply(("clear", 1, 2), oracle) == (1, 3) and not m.regs[1:3].any() and (m.regs[3] == 64 - p + 1).all()
