"""CPU: the helper of the sequence tests (tests/ctx_model.py) -- that the model is right, and that the random sequences
of tests/test_gpu_ctx_sequences.py and tests/test_gpu_ctx_sequences_derived.py cannot pass by not looking: the conditions
below are evaluated on the generators' output for the seeds the GPU tests use, without a GPU."""
import hashlib
import time

import numpy as np
import pytest

import derive_ref
from ctx_model import (FRACS, INDEX_OF, MUTATOR_KINDS, MUTATOR_KINDS2, OPTION_DEFAULTS, OPTION_DEFAULTS2, OPTION_VALUES, OPTION_VALUES2,
                       QUERY_KINDS, QUERY_KINDS2, STEPS, STEPS2, Model, fasta_files, fasta_reference, generate, generate2,
                       group_arrays, max_n, rows, run_query, sequences, walk, walk2)  # (tests/ctx_model.py)
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

    # ---- the kinds of QUERY_KINDS2, from the references themselves
    def fold(self, new_p, first, cnt, form):
        return derive_ref.fold(self.m.regs[first : first + cnt], new_p)

    def union(self, gp, mem, form):
        return derive_ref.union_groups(self.m.regs, gp, mem)

    def thr(self, t, rb, re, estim, rt, k):
        import thr_ref

        return thr_ref.tri(self.rows(rb, re, estim, rt, k), self.m.n, rb, re, t, rt)

    def pairs(self, lhs, rhs, estim, rt, k):
        import pairs_ref

        return pairs_ref.pick_rect(self.rect(0, self.m.n, 0, self.m.n, estim, rt, k), lhs, rhs)

    def _hits(self, t, estim, rt, k):
        import thr_ref

        n = self.m.n
        rp, col, _ = thr_ref.tri(self.rows(0, n, estim, rt, k), n, 0, n, t, rt)
        return n, rp, col

    def cluster(self, t, estim, rt, k, form, misalign=0):
        import cluster_ref

        n, rp, col = self._hits(t, estim, rt, k)
        return cluster_ref.labels_fast(n, *cluster_ref.csr_edges(rp, col))

    def cluster_of_hits(self, row_ptr, col):
        import cluster_ref

        return cluster_ref.labels(self.m.n, *cluster_ref.csr_edges(row_ptr, col))

    def greedy(self, t, estim, rt, k, form, misalign=0):
        import greedy_ref

        return greedy_ref.labels(*self._hits(t, estim, rt, k))

    def overlapped(self, estim, rt, k):
        import contextlib

        return contextlib.nullcontext()

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


# ---- the second generator (generate2: the old kinds and thresholded hits, pair lists, derived sketches, clusters,
# representatives together) -------------------------------------------------------------------------------------------
CASES2 = 30  # the default of DSH_SEQ2_CASES

# sha256(repr(generate(case)))[:16] at the commit before the second table was added: generate() returns what it did
GENERATE_DIGESTS = [
    "b79beadd9a521272", "cc3decd98ca0c19d", "7beb5f11ef20be9d", "c383f4d0635cba8d", "c104c32dd40a6761", "db0e0059f26fa2a4",
    "30b8dcfaa459db84", "ddd43ddd936fbd35", "32c02173bc44820b", "a3ee57f336717a65", "ee6a95702ef84346", "7984dab114c0087e",
    "b289d95e713649bf", "723d8555c2421349", "67c2c1d1f91d638d", "031e5a3abaff4e0e", "7e7997be7fc9220f", "2bf75b116c0a1494",
    "d87478dc76e3cdde", "e9d5b1d80932f43b", "ae00000c7b24e4c3", "eab7a97961e52369", "b06baf784cf277ac", "ec2cda5e2283464e",
    "21485bce138701fc", "346fe5b111649b81", "6dc3144ea3ac831a", "df2934c61c32ff53", "2616029c0327c42f", "adb61262d520da75",
    "61c130cfa2c7d03d", "e1c4bbb79c41b25e", "a0fdfc700b74233f", "58d79f8a4545dd35", "be0e8525b5b5fa62", "8d528198f12d71a1",
    "e102642367c551e4", "5e3998b50f6603ab", "77be3d1dbddf14e0", "25c0d2e85f1cd632",
]


def test_the_first_generator_did_not_move():
    got = [hashlib.sha256(repr(generate(c)).encode()).hexdigest()[:16] for c in range(CASES)]
    assert got == GENERATE_DIGESTS, [c for c in range(CASES) if got[c] != GENERATE_DIGESTS[c]]


def test_second_generator_is_deterministic_and_well_formed():
    for case in range(CASES2):
        ops = generate2(case)
        assert ops == generate2(case) and repr(ops) == repr(generate2(case))
        assert eval(repr(ops)) == ops  # recipes only: a printed sequence can be pasted as it stands
        assert sum(op[0] == "query" for op in ops) == STEPS2
        n = p = None
        attached = False
        for op in ops:
            t = op[0]
            if t in ("alloc", "set", "attach"):
                n, p = op[1], op[2]
                assert 2 <= n <= max_n(p)
                attached = t == "attach"
            elif t == "upfold":
                _, form, first, src_p, specs = op
                assert not attached and form in ("host", "device") and p <= src_p <= min(p + 6, 18)
                assert 0 <= first and first + len(specs) <= n and 1 <= len(specs) < n
                assert all(s[0] in ("law", "uni", "zero", "sat") for s in specs)
            elif t == "unite":
                _, first, groups = op
                assert not attached and 0 <= first and first + len(groups) <= n and 1 <= len(groups) < n
                assert all(0 <= x < n for g in groups for x in g)
            elif t in ("upload", "clear", "sketch", "records", "fastx"):
                assert not attached
            elif t == "opt":
                assert op[2] in dict(OPTION_VALUES, **OPTION_VALUES2)[op[1]]
            elif t == "query" and op[1] in QUERY_KINDS2:
                q = op[2]
                assert q["estim"] in (0, 1, 2) and 0 <= q["rt"] <= 8
                if op[1] == "fold":
                    assert 4 <= q["new_p"] <= p and 0 <= q["first"] and q["cnt"] >= 1 and q["first"] + q["cnt"] <= n
                elif op[1] == "union":
                    assert q["groups"] and all(0 <= x < n for g in q["groups"] for x in g)
                elif op[1] == "thr":
                    assert 0 <= q["rb"] < q["re"] <= n and q["frac"] in FRACS
                elif op[1] == "pairs":
                    assert 1 <= q["m"] <= 2000
                else:
                    assert q["frac"] in FRACS and q["form"] in ("host", "device") and q["misalign"] in (0, 1, 3)


def test_second_generator_reaches_every_new_kind_after_every_mutator_and_every_new_option():
    """over the default cases: every new query kind directly after every mutator kind (the two new ones included), after
    each of the four new options was set to another value -- counted over the queries WITHOUT an overlapped dense call in
    front of them, in which the new call is the first to meet what the mutator left --, in both forms, at every hit fraction, with and without an
    overlapped dense call and a fresh context; and the unions cut groups into chunks, leave groups empty and start
    group_ptr above 0"""
    ops = [op for case in range(CASES2) for op in generate2(case)]
    walked = [w for case in range(CASES2) for w in walk2(generate2(case))]
    mq = {(mut, kind) for kind, mut, _, overlap in walked if not overlap}
    assert not [(a, b) for a in MUTATOR_KINDS + MUTATOR_KINDS2 for b in QUERY_KINDS2 if (a, b) not in mq]
    oq = {(o, kind) for kind, _, opts, overlap in walked if not overlap for o in opts}
    assert not [(a, b) for a in sorted(OPTION_VALUES2) for b in QUERY_KINDS2 if (a, b) not in oq]
    assert {w[0] for w in walked} == set(QUERY_KINDS + QUERY_KINDS2)
    assert {(op[1], op[2]) for op in ops if op[0] == "opt" and op[1] in OPTION_VALUES2} == {(a, v) for a, vs in OPTION_VALUES2.items() for v in vs}
    new = [op for op in ops if op[0] == "query" and op[1] in QUERY_KINDS2]
    for kind in ("fold", "union", "cluster", "greedy"):
        assert {q["form"] for _, k, q in new if k == kind} == {"host", "device"}
    for kind in ("thr", "cluster", "greedy"):
        assert {q["frac"] for _, k, q in new if k == kind} == set(FRACS)
    for kind in QUERY_KINDS2:
        assert {(q["fresh"], q["overlap"]) for _, k, q in new if k == kind} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {q["misalign"] for _, k, q in new if k in ("cluster", "greedy")} == {0, 1, 3}
    assert {(q["estim"], q["rt"]) for _, k, q in new} == {(e, rt) for e in range(3) for rt in range(9)}
    up = [op for op in ops if op[0] == "upfold"]
    assert {op[1] for op in up} == {"host", "device"} and {s[0] for op in up for s in op[4]} == {"law", "uni", "zero", "sat"}
    groups = [g for op in ops if op[0] == "unite" for g in op[2]] + [g for _, k, q in new if k == "union" for g in q["groups"]]
    assert any(len(g) > 64 for g in groups) and any(not g for g in groups) and max(len(g) for g in groups) <= 300
    assert any(len(g) > 64 for op in ops if op[0] == "unite" for g in op[2])
    assert {len(op[2]) % 3 for op in ops if op[0] == "unite"} >= {1, 2}  # (group_arrays: group_ptr[0] = len(groups) % 3)
    print("queries per new kind over %d cases: %s" % (CASES2, {k: sum(1 for w in walked if w[0] == k) for k in QUERY_KINDS2}))


def test_upfold_and_unite_in_the_model(oracle):
    """a folded upload of rows the oracle sketched at src_p is the oracle's sketch of the same sequences at p; a union of
    one-member groups is the identity, of the pair [i, j] the element-wise maximum"""
    k = 21
    seq, off = sequences(170, [30_000, 700, 50, 9_000])
    for p, src_p in ((8, 14), (12, 12), (12, 18), (4, 10)):
        at_src = oracle.sketch_batch(seq, off, k, src_p, True)
        want = oracle.sketch_batch(seq, off, k, p, True)
        assert (derive_ref.fold(at_src, p) == want).all() and want.any()
    # the operation itself, with rows by recipe: assigned in place, neighbours untouched
    m = Model()
    m.apply(("set", 9, 10, 5, "law"), oracle)
    before = m.regs.copy()
    specs = [("law", 3, 50_000), ("sat",), ("zero",), ("uni", 4)]
    assert m.apply(("upfold", "host", 2, 13, specs), oracle) == (2, 6)
    assert (m.regs[2:6] == derive_ref.fold(rows(specs, 13, None), 10)).all() and (m.regs[[0, 1, 6, 7, 8]] == before[[0, 1, 6, 7, 8]]).all()
    assert (m.regs[3] == 64 - 10 + 1).all() and not m.regs[4].any() and m.regs[2].any()
    assert m.apply(("upfold", "device", 0, 10, [("law", 8, 777)]), oracle) == (0, 1)  # src_p == p: a plain copy
    assert (m.regs[0] == rows([("law", 8, 777)], 10, None)[0]).all()
    # unite
    before = m.regs.copy()
    assert m.apply(("unite", 5, [[5], [6], [7], [8]]), oracle) == (5, 9) and (m.regs == before).all()
    m.apply(("unite", 1, [[0, 2], [], [1]]), oracle)  # slot 1 is written by the first group and read by the third:
    assert (m.regs[1] == np.maximum(before[0], before[2])).all() and not m.regs[2].any() and (m.regs[3] == before[1]).all()
    gp, mem = group_arrays([[0, 2], [], [1]], 9)
    assert gp.tolist() == [0, 2, 2, 3] and mem.tolist() == [0, 2, 1]
    gp, mem = group_arrays([[4], [5, 5]], 9)
    assert gp.tolist() == [2, 3, 5] and mem.tolist() == [16, 16, 4, 5, 5]


def test_dry_run_of_the_second_generator(oracle):
    """the default cases against the oracle itself: every reference path of the new kinds runs, and the two shares that
    say the cluster and greedy queries look at something hold -- at most a quarter of them go without the comparison with
    the oracle's graph, at least half of them find neither n singletons nor one cluster.  Both are conditions on the
    GENERATOR: if a change to it trips one, reweight what _query2 draws for `frac` (more of "1/n" and "1%", fewer of
    "none" and "all") or what generate2 draws as matrix kinds -- the bounds stay."""
    log = []
    slowest = (0.0, None)
    for case in range(CASES2):
        model = Model()
        t0 = time.time()
        for op in generate2(case):
            if op[0] == "query":
                run_query(OracleQueries(oracle, model), model.regs, op, oracle, dict(OPTION_DEFAULTS, **OPTION_DEFAULTS2), log)
            else:
                model.apply(op, oracle)
        slowest = max(slowest, (time.time() - t0, case))
    seen = {e[0] for e in log}
    assert {"fold", "union", "thr", "pairs", "cluster", "greedy", "index_full", "close", "card", "knn"} <= seen, seen
    lab = [e for e in log if e[0] in ("cluster", "greedy")]
    skipped = sum(1 for e in lab if not e[5])
    informative = sum(1 for e in lab if e[4])
    thr = [e for e in log if e[0] == "thr"]
    print("cluster and greedy queries: %d; without the oracle's graph: %d (%.1f %%); neither singletons nor one cluster: %d (%.1f %%)"
          % (len(lab), skipped, 100.0 * skipped / len(lab), informative, 100.0 * informative / len(lab)))
    print("of those held to the oracle's graph, %d at a graph that is neither empty nor one cluster" % sum(1 for e in lab if e[6]))
    print("thr queries: %d, %d inside a gap of the oracle's values, %d held to the oracle, %d of those with hits"
          % (len(thr), sum(1 for e in thr if e[4]), sum(1 for e in thr if e[3]), sum(1 for e in thr if e[3] and e[2])))
    print("slowest case on the CPU: case %d, %.1f s" % (slowest[1], slowest[0]))
    assert sum(1 for e in log if e[0] == "skip_oracle" and e[1] != "thr") == skipped > 0  # (the skip path runs, and is logged)
    assert 4 * skipped <= len(lab)
    assert 2 * informative >= len(lab)
    assert 2 * sum(1 for e in lab if e[6]) >= len(lab)
    assert 4 * sum(1 for e in thr if e[3]) >= 3 * len(thr) and 3 * sum(1 for e in thr if e[3] and e[2]) >= len(thr)
    assert any(e[0] == "union" and e[2] > 64 for e in log)
