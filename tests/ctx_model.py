"""Model-based sequence tests of one context (tests/test_gpu_ctx_sequences.py on the device, tests/test_ctx_model.py
for the helper itself): a host-side model of the resident register matrix, the operation table, the seeded generator and
the comparison of every query with the CPU oracle evaluated on the model.  Plain helper module; no fixtures.

An operation is a tuple that holds recipes (seeds, lengths, row specs), never arrays, so a printed sequence can be pasted
into a directed test as it stands:

    ("alloc", n, p)                                        fresh zero matrix
    ("set", n, p, seed, kind)                              set_sketches(matrix(n, p, seed, kind))
    ("upload", first, [rowspec, ...])                      upload of len(rowspecs) rows at `first`
    ("clear", first, cnt)
    ("sketch", form, first, seed, [len, ...], k, canon)    max-merge; form: "sync" | "async" | "device"
    ("records", form, first, seed, [len, ...], k, canon)   overwrite
    ("fastx", first, seed, [[len, ...], ...], width, k, canon)   one in-memory FASTA file per genome, max-merge
    ("attach", n, p, seed, kind)                           a new torch tensor is attached
    ("reattach", [(row, rowspec), ...])                    the attached tensor changed with torch, attached again
    ("opt", name, value)                                   a speed knob: no effect on the model
    ("query", kind, {...})                                 see QUERY_KINDS

A rowspec is ("law", seed, card) | ("uni", seed) | ("zero",) | ("sat",) | ("dup", j) | ("bad", seed, card, pos, value).
"""
import numpy as np

from dashing_amd import synth

from fastx_gen import fasta
from kseq_ref import parse as kseq_parse

QUERY_KINDS = ["card", "tri", "range_id", "range_sorted", "rect", "knn_square", "knn_band", "shard", "parts"]
MUTATOR_KINDS = ["alloc", "set", "upload", "clear", "sketch", "records", "fastx", "attach"]
# the options a sequence may touch, with the value a fresh context has (restored when a test ends)
OPTION_DEFAULTS = {
    "emax": -1, "elow": -1, "kc": 0, "sort": -1, "nsplit": 0, "cum_budget_bytes": 8 << 30, "range_sort_min_rows": 1024,
    "knn_square_budget_bytes": 96 << 30, "part_band_tiles": 2048, "finalize_signal": -1,
}
OPTION_VALUES = {
    "emax": [-1, 0, 3, 17, 255], "elow": [-1, 0, 2, 40, 255], "kc": [0, 16, 32], "sort": [-1, 0, 1], "nsplit": [0, 1, 3, 8],
    "cum_budget_bytes": [1 << 20, 1 << 22, 8 << 30], "range_sort_min_rows": [1, 64, 1024],
    "knn_square_budget_bytes": [0, 96 << 30], "part_band_tiles": [1, 16, 2048], "finalize_signal": [-1, 0, 1],
}
P_CHOICES = [4, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18]
SEED_BASE = 0x5E0000
STEPS = 30


def max_n(p):
    return 400 if p <= 12 else (150 if p <= 14 else 24)


# ---------------------------------------------------------------------------------------------------------------------
# the comparison rule of tests/test_gpu_fuzz.py, verbatim

# distance measure -> the index it is a function of (result_cmp, src/dashing.h:568-592).  The distance
# formulas jump at index == 0 (`ret != 0 ? -log(ret)/k : 1`), so where the index is 0 up to rounding an
# ulp of the device log() in a cardinality (ORIGINAL/IMPROVED small-range terms) may pick the other side.
INDEX_OF = {0: 1, 3: 1, 6: 5, 4: 5, 8: 7}


def _close(got, want, index_got=None, index_want=None):
    """index_*: the same pairs under the underlying index measure; a mismatch is tolerated only where
    both implementations put that index within 1e-9 of zero (the discontinuity of the distance formulas)."""
    if index_got is not None:
        at_jump = (np.abs(index_got) < 1e-9) & (np.abs(index_want) < 1e-9)
        got, want = got[~at_jump], want[~at_jump]
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all()
    err = np.abs(got[fin].astype(np.float64) - want[fin])
    # 1e-6 relative; plus an absolute floor of 1e-12 of the matrix scale: SIZES / containment values are
    # differences of cardinalities, so one ulp of log() (device libm vs glibc, ORIGINAL/IMPROVED estimators)
    # in a cardinality of ~1e2..1e8 can leave ~1e-14 where the CPU gets an exact 0
    scale = float(np.abs(want[fin]).max()) if fin.any() else 1.0
    assert (err <= 1e-6 * np.maximum(np.abs(want[fin]), 1e-9) + 1e-12 * max(scale, 1.0)).all(), err.max()


# ---------------------------------------------------------------------------------------------------------------------
# recipes -> arrays


def row(spec, p, regs):
    """one register row of precision p; ("dup", j) copies row j of `regs` (the matrix before the operation)"""
    m, q = 1 << p, 64 - p
    t = spec[0]
    if t == "law":
        return synth.hll_registers(int(spec[1]), int(spec[2]), p)
    if t == "uni":
        return np.random.default_rng(int(spec[1])).integers(0, q + 2, m).astype(np.uint8)
    if t == "zero":
        return np.zeros(m, np.uint8)
    if t == "sat":
        return np.full(m, q + 1, np.uint8)
    if t == "dup":
        return regs[int(spec[1])].copy()
    if t == "bad":  # a register above 64 - p + 1: no HLL of this precision (the compare entry points refuse it)
        r = synth.hll_registers(int(spec[1]), int(spec[2]), p)
        r[int(spec[3])] = int(spec[4])
        return r
    raise AssertionError(spec)


def rows(specs, p, regs):
    return np.stack([row(s, p, regs) for s in specs])


def matrix(n, p, seed, kind):
    rng = np.random.default_rng(seed)
    m = 1 << p
    if kind == "law":  # cardinalities over many decades: the key order is far from the slot order
        cards = np.exp(rng.uniform(np.log(50 * m / 1024 + 10), np.log(4e8), n))
        regs = np.stack([synth.hll_registers(int(rng.integers(1 << 30)), int(c), p) for c in cards])
    elif kind == "related":
        regs = synth.synthetic_sketches(n, p, seed=int(rng.integers(1 << 30)))
    elif kind == "uniform":
        regs = rng.integers(0, 64 - p + 2, size=(n, m)).astype(np.uint8)
    else:
        raise AssertionError(kind)
    if n > 4 and rng.random() < 0.5:
        regs[int(rng.integers(n))] = 0
        a, b = rng.choice(n, 2, replace=False)
        regs[a] = regs[b]
    return regs


_ACGT = np.frombuffer(b"ACGT", np.uint8)


def sequences(seed, lens):
    """len(lens) sequences back to back (seq uint8, off uint64).  They are mutated copies of one root per seed family
    (seed >> 4), so sketches of different operations overlap; some carry an 'N' run and a lowercase stretch."""
    root = _ACGT[np.random.default_rng(0xD00D + (seed >> 4)).integers(0, 4, 60000)]
    rng = np.random.default_rng(seed)
    out = []
    for L in lens:
        L = int(L)
        a = int(rng.integers(0, root.size - L + 1))
        s = root[a : a + L].copy()
        hit = rng.random(L) < 0.02
        s[hit] = _ACGT[rng.integers(0, 4, int(hit.sum()))]
        if L > 200 and rng.random() < 0.5:
            x = int(rng.integers(0, L - 60))
            s[x : x + int(rng.integers(1, 40))] = ord("N")
            y = int(rng.integers(0, L - 60))
            s[y : y + 50] |= 0x20
        out.append(s)
    return synth.concat_for_device(out)


def fasta_files(seed, lens_per_genome, width):
    """one plain FASTA text per genome (bytes), records of the given lengths"""
    rng = np.random.default_rng(seed)
    files = []
    for g, lens in enumerate(lens_per_genome):
        seq, off = sequences(seed + 16 * (g + 1), lens)
        recs = [(b"g%d_r%d" % (g, i), seq[int(off[i]) : int(off[i + 1])].tobytes()) for i in range(len(lens))]
        files.append(fasta(rng, recs, width))
    return files


def fasta_reference(files):
    """what the encoder sees of every file under kseq: its records, one 'N' between two (seq, off)"""
    seqs = []
    for f in files:
        recs, _ = kseq_parse(f)
        seqs.append(np.frombuffer(b"N".join(q for _, q in recs), np.uint8))
    return synth.concat_for_device(seqs)


# ---------------------------------------------------------------------------------------------------------------------
# the model


class Model:
    """the resident matrix as the operations define it"""

    def __init__(self):
        self.regs = np.zeros((0, 16), np.uint8)
        self.p = 4

    @property
    def n(self):
        return self.regs.shape[0]

    def apply(self, op, oracle):
        """apply a mutator; returns the touched row range (lo, hi), or None for an option"""
        t = op[0]
        if t == "alloc":
            self.p = op[2]
            self.regs = np.zeros((op[1], 1 << op[2]), np.uint8)
            return 0, self.n
        if t in ("set", "attach"):
            self.p = op[2]
            self.regs = matrix(op[1], op[2], op[3], op[4])
            return 0, self.n
        if t == "upload":
            new = rows(op[2], self.p, self.regs)
            self.regs[op[1] : op[1] + len(new)] = new
            return op[1], op[1] + len(new)
        if t == "clear":
            self.regs[op[1] : op[1] + op[2]] = 0
            return op[1], op[1] + op[2]
        if t == "sketch":
            _, _, first, seed, lens, k, canon = op
            seq, off = sequences(seed, lens)
            new = oracle.sketch_batch(seq, off, k, self.p, canon)
            self.regs[first : first + len(lens)] = np.maximum(self.regs[first : first + len(lens)], new)
            return first, first + len(lens)
        if t == "records":
            _, _, first, seed, lens, k, canon = op
            seq, off = sequences(seed, lens)
            self.regs[first : first + len(lens)] = oracle.sketch_batch(seq, off, k, self.p, canon)
            return first, first + len(lens)
        if t == "fastx":
            _, first, seed, lens_per_genome, width, k, canon = op
            seq, off = fasta_reference(fasta_files(seed, lens_per_genome, width))
            new = oracle.sketch_batch(seq, off, k, self.p, canon)
            ng = len(lens_per_genome)
            self.regs[first : first + ng] = np.maximum(self.regs[first : first + ng], new)
            return first, first + ng
        if t == "reattach":
            before = self.regs.copy()
            for r, spec in op[1]:
                self.regs[r] = row(spec, self.p, before)
            rr = [r for r, _ in op[1]]
            return min(rr), max(rr) + 1
        if t == "opt":
            return None
        raise AssertionError(op)


def mutator_kind(op):
    return {"reattach": "attach"}.get(op[0], op[0]) if op[0] not in ("opt", "query") else None


# ---------------------------------------------------------------------------------------------------------------------
# queries: `Q` answers them as numpy arrays (CtxQueries below for a context; the CPU tests have one over the oracle)


class CtxQueries:
    """the query kinds on a dashing_amd.Context, results as numpy arrays"""

    def __init__(self, ctx):
        self.ctx = ctx

    def card(self, estim):
        return self.ctx.cardinalities(estim)

    def rows(self, rb, re, estim, rt, k):
        return self.ctx.dist_rows(rb, re, estim=estim, result_type=rt, k=k)

    def rect(self, q0, q1, r0, r1, estim, rt, k):
        return self.ctx.dist_rect(q0, q1, r0, r1, estim=estim, result_type=rt, k=k)

    def knn(self, nn, q0, q1, r0, r1, estim, rt, k):
        return self.ctx.knn(nn, q0, q1, r0, r1, estim=estim, result_type=rt, k=k)

    def shard(self, G, estim, rt, k):
        import torch

        ctx, n = self.ctx, self.ctx.n
        off = ctx.shard_plan(G, estim)
        total = n * (n - 1) // 2
        assert off[0] == 0 and off[-1] == total and all(off[i] <= off[i + 1] for i in range(G))
        sf = torch.zeros(max(total, 1), dtype=torch.float32, device="cuda")
        for r in range(G):
            span = torch.zeros(max(off[r + 1] - off[r], 1), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()  # the zero fill (torch's stream) must land before the library's stream writes
            ctx.dist_shard_device(span.data_ptr(), r, G, estim, rt, k)
            ctx.synchronize()
            sf[off[r] : off[r + 1]] = span[: off[r + 1] - off[r]]
        torch.cuda.synchronize()
        fin = torch.zeros(max(total, 1), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.unpermute_device(sf.data_ptr(), fin.data_ptr())
        ctx.synchronize()
        return fin.cpu().numpy()[:total]

    def parts(self, rb, re, nparts, estim, rt, k):
        import torch

        import dashing_amd

        span = dashing_amd.tri_span(self.ctx.n, rb, re)
        pd = torch.full((max(span, 1),), -9.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.ctx.dist_rows_parts_device_async(pd.data_ptr(), rb, re, nparts, estim=estim, result_type=rt, k=k)
        self.ctx.wait()
        return pd.cpu().numpy()[:span]

    def set_option(self, name, value):
        self.ctx.set_option(name, value)


def _answer(Q, regs, kind, q, rt, oracle):
    """(got, want) of query q under measure rt; both flat arrays over the same pairs, or None for `want` without oracle"""
    n = regs.shape[0]
    e, k = q["estim"], q["k"]
    if kind == "tri":
        got = Q.rows(0, n, e, rt, k)
        want = oracle.dist_tri(regs, e, rt, k) if oracle else None
    elif kind in ("range_id", "range_sorted"):
        got = Q.rows(q["rb"], q["re"], e, rt, k)
        want = oracle.dist_rows(regs, q["rb"], q["re"], e, rt, k) if oracle else None
    elif kind == "rect":
        got = Q.rect(q["q0"], q["q1"], q["r0"], q["r1"], e, rt, k).ravel()
        want = None
        if oracle:
            want = oracle.dist_rect(regs[q["q0"] : q["q1"]], regs[q["r0"] : q["r1"]], e, rt, k).ravel() if got.size else got.copy()
    elif kind == "shard":
        got = Q.shard(q["G"], e, rt, k)
        want = oracle.dist_tri(regs, e, rt, k) if oracle else None
    elif kind == "parts":
        got = Q.parts(q["rb"], q["re"], q["nparts"], e, rt, k)
        want = oracle.dist_rows(regs, q["rb"], q["re"], e, rt, k) if oracle else None
    else:
        raise AssertionError(kind)
    return got, want


class _Temp:
    """an option at a value for the length of a query, on every context that answers it; then back to `back`"""

    def __init__(self, Qs, name, value, back):
        self.Qs, self.name, self.value, self.back = Qs, name, value, back

    def __enter__(self):
        for Q in self.Qs:
            Q.set_option(self.name, self.value)

    def __exit__(self, *a):
        for Q in self.Qs:
            Q.set_option(self.name, self.back)


class _Null:
    def __enter__(self):
        pass

    def __exit__(self, *a):
        pass


def run_query(Q, regs, op, oracle, options, log=None, fresh=None):
    """Answer op = ("query", kind, q) on Q and compare with the oracle on `regs`; with `fresh` (the same model in a second
    context with the same options) the two results must have equal bytes.  `options`: the option values in effect (the
    kinds that need a knob set it for the query and put the current value back).  `log` collects what was compared."""
    kind, q = op[1], op[2]
    log = [] if log is None else log
    Qs = [Q] + ([fresh] if fresh is not None else [])
    temp = _Null()
    if kind == "range_sorted":  # the range's own key-ordered layout, however short
        temp = _Temp(Qs, "range_sort_min_rows", 1, options["range_sort_min_rows"])
    elif kind == "range_id":
        temp = _Temp(Qs, "range_sort_min_rows", 1 << 30, options["range_sort_min_rows"])
    elif kind == "knn_band":
        temp = _Temp(Qs, "knn_square_budget_bytes", 0, options["knn_square_budget_bytes"])
    elif kind == "knn_square":
        temp = _Temp(Qs, "knn_square_budget_bytes", 96 << 30, options["knn_square_budget_bytes"])
    with temp:
        if kind == "card":
            got = Q.card(q["estim"])
            want = oracle.cardinalities(regs, q["estim"])
            fin = np.isfinite(want)
            assert (np.isfinite(got) == fin).all()
            assert np.allclose(got[fin], want[fin], rtol=1e-12, atol=0)
            log.append(("card", q["estim"], got.size))
            if fresh is not None:
                assert fresh.card(q["estim"]).tobytes() == got.tobytes(), "cardinalities differ from a fresh context"
            return got
        if kind in ("knn_square", "knn_band"):
            n = regs.shape[0]
            a = (q["nn"], q.get("q0", 0), q.get("q1", n), q.get("r0", 0), q.get("r1", n), q["estim"], q["rt"], q["k"])
            gi, gv = Q.knn(*a)
            wi, wv = oracle.knn(regs, a[0], a[1], a[2], a[3], a[4], estim=a[5], result_type=a[6], k=a[7])
            assert (gi == wi).all(), np.argwhere(gi != wi)[:5]
            assert np.allclose(gv, wv, rtol=1e-6, atol=1e-12, equal_nan=True)
            log.append(("knn", q["rt"], gi.size))
            if fresh is not None:
                fi, fv = fresh.knn(*a)
                assert fi.tobytes() == gi.tobytes() and fv.tobytes() == gv.tobytes(), "kNN differs from a fresh context"
            return gi, gv
        rt = q["rt"]
        ig = iw = None
        if rt in INDEX_OF:  # the index on ALL pairs first: the distance may then differ only where that index is 0
            ig, iw = _answer(Q, regs, kind, q, INDEX_OF[rt], oracle)
            _close(ig, iw)
            log.append(("index_full", INDEX_OF[rt], ig.size))
        got, want = _answer(Q, regs, kind, q, rt, oracle)
        assert got.shape == want.shape
        _close(got, want, ig, iw)
        log.append(("close", rt, ig is not None, got.size))
        if fresh is not None:
            assert _answer(fresh, regs, kind, q, rt, None)[0].tobytes() == got.tobytes(), "result differs from a fresh context"
        return got


# ---------------------------------------------------------------------------------------------------------------------
# the generator


def _rowspec(rng, n, p):
    u = rng.random()
    if u < 0.12:
        return ("zero",)
    if u < 0.24:
        return ("sat",)
    if u < 0.36:
        return ("dup", int(rng.integers(n)))
    if u < 0.44:
        return ("uni", int(rng.integers(1 << 30)))
    # cardinalities over eight decades: a replaced row lands, as a rule, far from its old place in the key order
    return ("law", int(rng.integers(1 << 30)), int(10 ** rng.uniform(0.5, 8.6)))


def _lens(rng, cnt, k, short_ok):
    out = []
    for _ in range(cnt):
        if short_ok and rng.random() < 0.2:
            out.append(int(rng.integers(0, k)))  # a record shorter than k: an all-zero row
        else:
            out.append(int(np.exp(rng.uniform(np.log(50), np.log(60000)))))
    return out


def _shape(rng):
    p = int(rng.choice(P_CHOICES))
    return int(rng.integers(2, max_n(p) + 1)), p


def _mutator(rng, kind, n, p, attached):
    """one mutator of `kind` for a resident n x 2^p matrix; returns (ops, n, p, attached)"""
    k = int(rng.choice([15, 21, 31, 32]))
    canon = bool(rng.random() < 0.8)
    pre = []
    if attached and kind in ("upload", "clear", "sketch", "records", "fastx"):
        # an attached matrix is the caller's and the library writes only into its own: back to an owned one first
        pre = [("set", n, p, int(rng.integers(1 << 30)), "law")]
    if kind == "alloc":
        if rng.random() < 0.7:
            n, p = _shape(rng)
        return [("alloc", n, p)], n, p, False
    if kind in ("set", "attach"):
        if kind == "attach" and attached and rng.random() < 0.6:  # the tensor changed under the library
            cnt = int(rng.integers(1, min(n, 5) + 1))
            rr = sorted(int(x) for x in rng.choice(n, cnt, replace=False))
            return [("reattach", [(r, _rowspec(rng, n, p)) for r in rr])], n, p, True
        if rng.random() < 0.4:
            n, p = _shape(rng)
        mk = str(rng.choice(["law", "related", "uniform"]))
        return [(kind, n, p, int(rng.integers(1 << 30)), mk)], n, p, kind == "attach"
    cnt = int(rng.integers(1, min(n - 1, 4) + 1))  # a strict sub-range
    first = int(rng.integers(0, n - cnt + 1))
    if kind == "upload":
        return pre + [("upload", first, [_rowspec(rng, n, p) for _ in range(cnt)])], n, p, False
    if kind == "clear":
        return pre + [("clear", first, cnt)], n, p, False
    seed = int(rng.integers(1 << 20))
    if kind in ("sketch", "records"):
        form = str(rng.choice(["sync", "async", "device"]))
        return pre + [(kind, form, first, seed, _lens(rng, cnt, k, kind == "records"), k, canon)], n, p, False
    if kind == "fastx":
        lens = [_lens(rng, int(rng.integers(1, 4)), k, False) for _ in range(cnt)]
        return pre + [("fastx", first, seed, lens, int(rng.choice([0, 60, 80])), k, canon)], n, p, False
    raise AssertionError(kind)


def _query(rng, kind, n):
    # the estimator changes in about two of three consecutive queries
    estim = int(rng.integers(0, 3))
    rt = int(rng.integers(0, 9))
    q = {"estim": estim, "rt": rt, "k": int(rng.choice([15, 21, 31, 32])), "fresh": bool(rng.random() < 0.25)}
    if kind == "card":
        del q["rt"], q["k"]
    elif kind in ("range_id", "range_sorted"):
        q["rb"] = int(rng.integers(0, n - 1))
        q["re"] = int(rng.integers(q["rb"] + 1, n + 1))
        if kind == "range_sorted" and rng.random() < 0.5:
            q["re"] = n  # [rb, n): with rb > 0 the per-sketch pass is left covering [rb, n) only
    elif kind == "parts":
        q["rb"] = int(rng.integers(0, n - 1))
        q["re"] = int(rng.integers(q["rb"] + 1, n + 1))
        q["nparts"] = int(rng.integers(2, 6))
    elif kind == "rect":
        q["q0"] = int(rng.integers(0, n)); q["q1"] = int(rng.integers(q["q0"], n + 1))
        q["r0"] = int(rng.integers(0, n)); q["r1"] = int(rng.integers(q["r0"], n + 1))
    elif kind in ("knn_square", "knn_band"):
        q["nn"] = int(rng.integers(1, min(n - 1, 8) + 1))
        if n > 3 and rng.random() < 0.4:  # queries vs references
            c = int(rng.integers(1, n))
            q.update(q0=c, q1=n, r0=0, r1=c)
            q["nn"] = min(q["nn"], c)
    elif kind == "shard":
        q["G"] = int(rng.integers(1, 6))
    return ("query", kind, q)


def generate(case, steps=STEPS):
    """the operations of random case `case`: a first matrix, then `steps` steps of [option] [mutators] query"""
    rng = np.random.default_rng(SEED_BASE + case)
    n, p = _shape(rng)
    ops = [("set", n, p, int(rng.integers(1 << 30)), str(rng.choice(["law", "related", "uniform"])))]
    attached = False
    for _ in range(steps):
        if rng.random() < 0.3:
            name = str(rng.choice(sorted(OPTION_VALUES)))
            ops.append(("opt", name, int(rng.choice(OPTION_VALUES[name]))))
        for _ in range(int(rng.choice([0, 1, 2], p=[0.15, 0.6, 0.25]))):
            more, n, p, attached = _mutator(rng, str(rng.choice(MUTATOR_KINDS)), n, p, attached)
            ops += more
        ops.append(_query(rng, str(rng.choice(QUERY_KINDS)), n))
    return ops


def walk(ops):
    """per query of a sequence: (kind, previous query kind or None, kind of the last register mutator since the previous
    query or None, hot, estimator) -- hot: registers changed since the previous query, and that query saw the same (n, p)"""
    out = []
    shape = prev_shape = prev_kind = last_mut = None
    for op in ops:
        if op[0] == "query":
            out.append((op[1], prev_kind, last_mut, last_mut is not None and prev_shape == shape, op[2]["estim"]))
            prev_kind, prev_shape, last_mut = op[1], shape, None
        elif op[0] != "opt":
            if op[0] in ("alloc", "set", "attach"):
                shape = (op[1], op[2])
            last_mut = mutator_kind(op)
    return out


def fmt(ops):
    return "\n".join("    %r," % (op,) for op in ops)
