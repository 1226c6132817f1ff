"""Model-based sequence tests of one context (tests/test_gpu_ctx_sequences.py on the device, tests/test_ctx_model.py
for the helper itself): a host-side model of the resident register matrix, the operation table, the seeded generator and
the comparison of every query with the CPU oracle evaluated on the model.  Plain helper module; no fixtures.

Two tables: the first (QUERY_KINDS, MUTATOR_KINDS, OPTION_*; generate) is the state of the library when the sequence tests
were written and does not move -- tests/test_ctx_model.py pins what generate() returns --, the second (QUERY_KINDS2, ...;
generate2, tests/test_gpu_ctx_sequences_derived.py) adds thresholded hits, pair lists, derived sketches, threshold
clusters and greedy representatives and draws from both.

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
    ("upfold", form, first, src_p, [rowspec, ...])         rows built at src_p >= p, folded into the slots; form: "host" | "device"
    ("unite", first, [[member, ...], ...])                 union_groups_device of the resident rows, copied into the slots
    ("opt", name, value)                                   a speed knob: no effect on the model
    ("query", kind, {...})                                 see QUERY_KINDS and QUERY_KINDS2

A rowspec is ("law", seed, card) | ("uni", seed) | ("zero",) | ("sat",) | ("dup", j) | ("bad", seed, card, pos, value).
"""
import numpy as np

from dashing_amd import synth

import cluster_ref
import derive_ref
import greedy_ref
import pairs_ref
import thr_ref
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
# The second table (generate2): the calls that came after the first one was drawn up.  generate() draws from the tables
# above, so a key added THERE would move every sequence it returns; these are drawn by generate2 alone.
QUERY_KINDS2 = ["fold", "union", "thr", "pairs", "cluster", "greedy"]
MUTATOR_KINDS2 = ["upfold", "unite"]
OPTION_DEFAULTS2 = {"threshold_band_bytes": 1 << 30, "greedy_band_rows": 4096, "cluster_chunk": 1 << 20, "derive_chunk_bytes": 256 << 20}
OPTION_VALUES2 = {
    "threshold_band_bytes": [64 << 10, 1 << 20, 1 << 30], "greedy_band_rows": [1, 7, 129, 4096], "cluster_chunk": [1, 4096, 1 << 20],
    "derive_chunk_bytes": [1, 1 << 14, 256 << 20],
}
FRACS = {"none": 0.0, "1/n": None, "1%": 0.01, "50%": 0.5, "all": 1.0}  # hit fractions of a threshold (None: 1 / n)
SEED_BASE2 = 0x5E2000
STEPS2 = 24
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
        if t == "upfold":
            _, _, first, src_p, specs = op
            assert src_p >= self.p and not any(x[0] in ("dup", "bad") for x in specs)
            new = derive_ref.fold(rows(specs, src_p, None), self.p)
            self.regs[first : first + len(new)] = new
            return first, first + len(new)
        if t == "unite":
            _, first, groups = op
            gp, mem = group_arrays(groups, self.n)
            new = derive_ref.union_groups(self.regs, gp, mem)  # (of the rows BEFORE the operation: the slots may be members)
            self.regs[first : first + len(new)] = new
            return first, first + len(new)
        if t == "opt":
            return None
        raise AssertionError(op)


def group_arrays(groups, n):
    """(group_ptr uint64, members uint32) of a list of member lists.  group_ptr starts at len(groups) % 3, not at 0: the
    members in front of it belong to no group and name no sketch (n + 7), so a library that read them would refuse them"""
    lead = len(groups) % 3
    gp = np.cumsum([lead] + [len(g) for g in groups]).astype(np.uint64)
    mem = np.array([n + 7] * lead + [m for g in groups for m in g], np.uint32)
    return gp, mem


def mutator_kind(op):
    return {"reattach": "attach"}.get(op[0], op[0]) if op[0] not in ("opt", "query") else None


# ---------------------------------------------------------------------------------------------------------------------
# queries: `Q` answers them as numpy arrays (CtxQueries below for a context; the CPU tests have one over the oracle)


class CtxQueries:
    """the query kinds on a dashing_amd.Context, results as numpy arrays"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.reserved = []  # guarded device buffers allocated ahead of a query (reserve)

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

    # ---- the kinds of QUERY_KINDS2
    def _new_guarded(self, items, dtype, misalign=0):
        import torch

        import guard

        return guard.Guarded(items, dtype, front=4096, back=4096, misalign=misalign, device=torch.device("cuda:0"))

    def reserve(self, op):
        """The guarded buffers the device form of query `op` will ask for, allocated NOW.  guard.Guarded fills its buffer
        with torch and then waits for the whole device; a caller that must put no host wait between an asynchronous
        sketch call and the query reserves before that call (n and p as they are now: sketch calls keep them)."""
        kind, q = op[1], op[2]
        if kind not in QUERY_KINDS2 or q.get("form") != "device":
            return
        n, p = self.ctx.n, self.ctx.p
        if kind == "fold":
            want = [(q["cnt"] << q["new_p"], np.uint8, 0)]
        elif kind == "union":
            want = [(len(q["groups"]) << p, np.uint8, 0)]
        else:  # one label buffer per call and threshold: two thresholds, and a greedy query also asks for the components
            want = [(n, np.uint32, q.get("misalign", 0))] * (4 if kind == "greedy" else 2)
        self.reserved += [(w, self._new_guarded(*w)) for w in want]

    def release(self):
        self.reserved = []

    def _guarded(self, items, dtype, misalign=0):
        for x, (w, buf) in enumerate(self.reserved):
            if w == (items, dtype, misalign):
                del self.reserved[x]
                return buf
        return self._new_guarded(items, dtype, misalign)

    def _take(self, buf, what):
        buf.check(what)
        assert buf.unwritten() == 0, "%s left %d elements of the span unwritten" % (what, buf.unwritten())
        return buf.host().copy()

    def fold(self, new_p, first, cnt, form):
        if form == "host":
            return self.ctx.fold(new_p, first, cnt)
        buf = self._guarded(cnt << new_p, np.uint8)
        self.ctx.fold_device(buf.ptr, new_p, first, cnt)
        return self._take(buf, "fold_device").reshape(cnt, 1 << new_p)

    def union(self, gp, mem, form):
        if form == "host":
            return self.ctx.union_groups(gp, mem)
        ng = gp.size - 1
        buf = self._guarded(ng << self.ctx.p, np.uint8)
        self.ctx.union_groups_device(buf.ptr, gp, mem)
        return self._take(buf, "union_groups_device").reshape(ng, 1 << self.ctx.p)

    def thr(self, t, rb, re, estim, rt, k):
        return self.ctx.dist_threshold(t, rb, re, estim=estim, result_type=rt, k=k)

    def pairs(self, lhs, rhs, estim, rt, k):
        return self.ctx.dist_pairs(lhs, rhs, (rt,), estim=estim, k=k)[0]

    def _labels(self, host, device, t, estim, rt, k, form, misalign):
        if form == "host":
            return host(t, estim=estim, result_type=rt, k=k)
        buf = self._guarded(self.ctx.n, np.uint32, misalign)
        cnt = device(buf.ptr, t, estim=estim, result_type=rt, k=k)
        return self._take(buf, device.__name__), cnt

    def cluster(self, t, estim, rt, k, form, misalign=0):
        return self._labels(self.ctx.cluster_threshold, self.ctx.cluster_threshold_device, t, estim, rt, k, form, misalign)

    def greedy(self, t, estim, rt, k, form, misalign=0):
        return self._labels(self.ctx.greedy_threshold, self.ctx.greedy_threshold_device, t, estim, rt, k, form, misalign)

    def cluster_of_hits(self, row_ptr, col):
        return self.ctx.cluster_csr(self.ctx.n, row_ptr, col)

    def overlapped(self, estim, rt, k):
        """a dist_rows_async into pinned memory in front of what the `with` holds, waited for behind it: its bytes are those
        of the synchronous dense rows (the check of tests/test_gpu_threshold_sequences.py)"""
        return _Overlap(self.ctx, estim, rt, k)

    def set_option(self, name, value):
        self.ctx.set_option(name, value)


class _Overlap:
    def __init__(self, ctx, estim, rt, k):
        self.ctx, self.a = ctx, dict(estim=estim, result_type=rt, k=k)

    def __enter__(self):
        import dashing_amd

        n = self.ctx.n
        self.span = dashing_amd.tri_span(n, 0, n)
        self.pin = dashing_amd.PinnedArray(max(self.span, 1), np.float32)
        self.ctx.dist_rows_async(self.pin.array, 0, n, **self.a)

    def __exit__(self, etype, *a):
        self.ctx.wait()
        if etype is None:
            dense = self.ctx.dist_rows(0, self.ctx.n, **self.a)
            assert self.pin.array[: self.span].tobytes() == dense.tobytes(), "the overlapped dense rows differ from the synchronous ones"


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
    if kind in QUERY_KINDS2:
        with Q.overlapped(q["estim"], q["rt"], q["k"]) if q.get("overlap") else _Null():
            return _run_query2(Q, regs, kind, q, oracle, log, fresh)
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
# the kinds of QUERY_KINDS2.  Registers, hits, pair values and labels have ONE answer each: every comparison below is one
# of bytes or integers, except the two the suite already has between device and oracle VALUES (_close above, and
# compare_with_oracle of tests/test_gpu_threshold.py).
#
# Order matters: the threshold held to the oracle's graph is computed from the MODEL alone, so the call under test runs at
# it BEFORE anything else touches the context -- it is the call that meets whatever the mutator left behind.  The dense
# triangle of the same context (the old path) comes after it, and the threshold taken out of that triangle last.

GAP = 2e-6  # the gap of the oracle's values a threshold must sit in (tests/test_gpu_cluster.py, test_against_oracle)


def _oracle_values(regs, q, oracle):
    """(the oracle's values of the triangle under the query's measure, its values of the underlying index or None)"""
    e, rt, k = q["estim"], q["rt"], q["k"]
    iw = oracle.dist_tri(regs, e, INDEX_OF[rt], k) if rt in INDEX_OF else None
    return oracle.dist_tri(regs, e, rt, k), iw


def _dense_checked(Q, regs, q, ov, iw, log):
    """the dense triangle of the same context under the query's measure, compared with the oracle the way a "tri" query
    is (the index on all pairs first)"""
    n, e, rt, k = regs.shape[0], q["estim"], q["rt"], q["k"]
    ig = None
    if iw is not None:
        ig = Q.rows(0, n, e, INDEX_OF[rt], k)
        _close(ig, iw)
        log.append(("index_full", INDEX_OF[rt], ig.size))
    got = Q.rows(0, n, e, rt, k)
    assert got.shape == ov.shape
    _close(got, ov, ig, iw)
    log.append(("close", rt, ig is not None, got.size))
    return got


def own_threshold(dense, frac, rt, n):
    """a value that OCCURS in the dense triangle, at that quantile (quantile_thresholds of tests/test_gpu_cluster.py)"""
    from test_gpu_cluster import quantile_thresholds

    ts = quantile_thresholds(dense, rt, n)
    return ts[["none", "all", "1/n", "1%", "50%"].index(frac)] if len(ts) > 1 else ts[0]


def jump_floor(iw, rt, k):
    """The distance measures of INDEX_OF jump where their index is 0, and there device and oracle may take different sides
    (_close leaves exactly those pairs out).  On either side such a pair lies at a distance of 1 - (4e-9) ** (1 / k) or
    more: its index is below 1e-9 on the oracle, so below 1e-9 + 1e-12 on the device (_close of the index), the argument
    x of the distance formulas is the index or 2 j / (1 + j), below 4e-9 either way, and -log(x) / k >= 1 - x ** (1 / k).
    BELOW that value the pair is no hit for both, and the oracle's graph is the device's; at or above it the oracle's
    graph does not bind the device's.  Returns that value where the oracle sees such a pair, else None."""
    if iw is None or rt in thr_ref.SIMILARITY or not (np.abs(iw) < 1e-9).any():
        return None
    return 1.0 - (4e-9) ** (1.0 / k)


def outside(vals, sim, nothing):
    """a threshold outside the values by a thousandth of their scale, on the side where nothing passes or everything does"""
    d = 1e-3 * max(float(np.abs(vals).max()), 1.0)
    return float(vals.max()) + d if nothing == sim else float(vals.min()) - d  # (similarities pass with v >= t)


def gap_choice(ov, frac, sim, n, below=None):
    """(t, gap): a threshold inside a gap of the oracle's values near the quantile `frac`, and the width of that gap
    (gap_threshold of tests/test_gpu_cluster.py: the widest gap among the 200 values around the quantile).  Where those
    200 hold no gap above GAP the window moves outwards, 200 values at a time, the side towards the nearer end first, and
    stops at the first that does.  `below` (jump_floor, distances only): only the values under it are looked at, so t
    stays under it.  If no window holds a gap the result is (t, 0.0): there is no oracle graph for that fraction --
    except for "none" and "all", which ask for the empty and the full graph and get a threshold outside() all values
    ("all" only without `below`).  No finite value at all: every threshold gives the empty graph.

    Example: JI values 0.9 0.9 0.9 0.2 0.1 (best first), frac "1%" -> the quantile is the first value; its window holds
    the gap 0.9 | 0.2, so (0.55, 0.7).  Five values of 0.9 and frac "50%": no gap anywhere, (0.9, 0.0); frac "none":
    (0.901, 0.002)."""
    from test_gpu_cluster import gap_threshold

    vals = np.asarray(ov, np.float64)
    vals = vals[np.isfinite(vals)]
    if not vals.size:
        return 0.5, float("inf")
    total = vals.size
    if below is not None:
        assert not sim
        vals = vals[vals < below - 1e-3]
    f = 1.0 / n if FRACS[frac] is None else FRACS[frac]
    if vals.size >= 2:
        at = min(f * total / vals.size, 1.0)  # the same number of values from the best end
        step = 200.0 / vals.size
        order = [at] + [g for x in range(1, int(np.ceil(1.0 / step)) + 1)
                        for g in ((at - x * step, at + x * step) if at <= 0.5 else (at + x * step, at - x * step)) if 0.0 <= g <= 1.0]
        for g in order:
            t, gap = gap_threshold(vals, g, sim)
            if gap > GAP:
                return t, gap
    if frac == "none":
        return (outside(vals, sim, True), float("inf")) if vals.size else (below / 2, below)
    if frac == "all" and below is None:
        return outside(vals, sim, False), float("inf")
    return (float(vals[0]) if vals.size else 0.5), 0.0


def _oracle_graph(ov, iw, frac, rt, k, n, log, what):
    """(t, hits of the oracle's values at t) where the oracle's graph binds the device's, else None (logged)"""
    sim = rt in thr_ref.SIMILARITY
    below = jump_floor(iw, rt, k)
    t, gap = gap_choice(ov, frac, sim, n, below)
    if not gap > GAP or thr_ref.undecided(ov, t).any() or (below is not None and t >= below):
        log.append(("skip_oracle", what, frac, gap))
        return None
    with np.errstate(invalid="ignore"):
        hit = (ov.astype(np.float64) >= t) if sim else (ov.astype(np.float64) <= t)
    return t, hit


def pair_list(seed, m, n):
    rng = np.random.default_rng(seed)
    lhs, rhs = rng.integers(0, n, m).astype(np.uint32), rng.integers(0, n, m).astype(np.uint32)
    rep = rng.integers(0, m, m // 4)  # repeats: a quarter of the list says again what another entry says
    lhs[rep], rhs[rep] = lhs[(rep * 7 + 1) % m], rhs[(rep * 7 + 1) % m]
    return lhs, rhs


def _same_as_fresh(fresh, got, again, what):
    if fresh is not None:
        other = again(fresh)
        a = got if isinstance(got, tuple) else (got,)
        b = other if isinstance(other, tuple) else (other,)
        assert len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b)), \
            "%s differs from a fresh context" % what


def _run_query2(Q, regs, kind, q, oracle, log, fresh):
    n = regs.shape[0]
    if kind == "fold":
        a = (q["new_p"], q["first"], q["cnt"], q["form"])
        got = Q.fold(*a)
        want = derive_ref.fold(regs[q["first"] : q["first"] + q["cnt"]], q["new_p"])
        assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes(), "fold differs from the model"
        log.append(("fold", q["form"], got.size))
        _same_as_fresh(fresh, got, lambda F: F.fold(*a), "fold")
        return got
    if kind == "union":
        gp, mem = group_arrays(q["groups"], n)
        got = Q.union(gp, mem, q["form"])
        want = derive_ref.union_groups(regs, gp, mem)
        assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes(), "union differs from the model"
        log.append(("union", q["form"], max(len(g) for g in q["groups"])))
        _same_as_fresh(fresh, got, lambda F: F.union(gp, mem, q["form"]), "union")
        return got
    e, rt, k = q["estim"], q["rt"], q["k"]
    sim = rt in thr_ref.SIMILARITY
    ov, iw = _oracle_values(regs, q, oracle)  # (the CPU alone: the context has not been touched yet)
    if kind == "pairs":
        lhs, rhs = pair_list(q["seed"], q["m"], n)
        got = Q.pairs(lhs, rhs, e, rt, k)  # first; what it is held to follows
        assert got.dtype == np.float32
        dense = _dense_checked(Q, regs, q, ov, iw, log)
        rect = Q.rect(0, n, 0, n, e, rt, k)
        assert pairs_ref.same_bits(got, pairs_ref.pick_rect(rect, lhs, rhs)), "pair values differ from the dense rectangle"
        hi = lhs > rhs
        assert pairs_ref.same_bits(got[hi], pairs_ref.pick_tri(dense, n, lhs[hi], rhs[hi])), "pair values differ from the dense triangle"
        log.append(("pairs", lhs.size, int(hi.sum())))
        _same_as_fresh(fresh, got, lambda F: F.pairs(lhs, rhs, e, rt, k), "pairs")
        return got
    if kind == "thr":
        from test_gpu_threshold import compare_with_oracle

        rb, re = q["rb"], q["re"]
        found = _oracle_graph(ov, iw, q["frac"], rt, k, n, log, "thr")
        below = jump_floor(iw, rt, k)
        fin = ov[np.isfinite(ov)].astype(np.float64)
        if found:
            t = found[0]
        elif fin.size:  # no gap at that fraction: everything for a fraction above a half (never into the jump), else nothing
            t = outside(fin, sim, not (FRACS[q["frac"]] is not None and FRACS[q["frac"]] > 0.5 and below is None))
        else:
            t = 0.5
        held = not thr_ref.undecided(ov, t).any() and (below is None or t < below)
        got = Q.thr(t, rb, re, e, rt, k)  # first
        assert thr_ref.same(got, thr_ref.tri(Q.rows(rb, re, e, rt, k), n, rb, re, t, rt)), "hits differ from the dense rows"
        if held:
            lo, span = int(thr_ref.row_lengths(n, 0, rb).sum()), int(thr_ref.row_lengths(n, rb, re).sum())
            compare_with_oracle(got, ov[lo : lo + span], n, rb, re, t, rt)
        _dense_checked(Q, regs, q, ov, iw, log)
        log.append(("thr", q["frac"], int(got[1].size), held, bool(found)))
        _same_as_fresh(fresh, got, lambda F: F.thr(t, rb, re, e, rt, k), "thr")
        return got
    assert kind in ("cluster", "greedy"), kind
    i, j = np.triu_indices(n, 1)
    form, mis = q["form"], q.get("misalign", 0)
    dense = None

    def labels_at(X, t):
        """(component labels, count) and, for a greedy query, (greedy labels, count) behind them.  The call the query is
        about runs FIRST: for a greedy query the components are wanted only for the references that follow."""
        first = X.greedy(t, e, rt, k, form, mis) if kind == "greedy" else ()
        out = X.cluster(t, e, rt, k, form, mis) + first
        assert all(np.asarray(x).dtype == np.uint32 and np.shape(x) == (n,) for x in out[0::2]), "labels are uint32 [n]"
        return tuple(np.asarray(x, np.uint64 if np.ndim(x) == 0 else np.uint32) for x in out)

    def check(t, hit, by_definition):
        got = labels_at(Q, t)
        comp, nc = got[0], int(got[1])
        want, wc = (cluster_ref.labels if by_definition else cluster_ref.labels_fast)(n, i[hit], j[hit])
        assert np.array_equal(comp, want) and nc == wc, "cluster labels at t = %.9g" % t
        if kind == "cluster" and not by_definition and int(hit.sum()) <= 20000:
            # the graph form over the same hits, in edge chunks of "cluster_chunk" (one edge per launch at its smallest value)
            rp, col, _ = thr_ref.tri(dense, n, 0, n, t, rt)
            via, vc = Q.cluster_of_hits(rp, col)
            assert np.array_equal(via, want) and vc == wc, "cluster_csr over the hits at t = %.9g" % t
        if kind == "greedy":
            lab, nr = got[2], int(got[3])
            if by_definition:
                h = np.zeros((n, n), bool)
                h[i, j] = hit
                want, wr = greedy_ref.labels_from_definition(n, h)
            else:
                rp, col, _ = thr_ref.tri(dense, n, 0, n, t, rt)
                want, wr = greedy_ref.labels(n, rp, col)
            assert np.array_equal(lab, want) and nr == wr, "greedy labels at t = %.9g" % t
            assert np.array_equal(comp[lab], comp), "a greedy cluster leaves its component at t = %.9g" % t
        _same_as_fresh(fresh, got, lambda F: labels_at(F, t), kind)
        return int(got[-1])

    found = _oracle_graph(ov, iw, q["frac"], rt, k, n, log, kind)
    gcnt = check(found[0], found[1], True) if found else None  # first: the label call itself meets what the mutator left
    dense = _dense_checked(Q, regs, q, ov, iw, log)
    t_own = own_threshold(dense, q["frac"], rt, n)
    cnt = check(t_own, thr_ref.passes(dense, t_own, rt), False)
    log.append((kind, q["frac"], form, cnt, 1 < cnt < n, bool(found), gcnt is not None and 1 < gcnt < n))
    return cnt


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


# ---------------------------------------------------------------------------------------------------------------------
# the second generator: the old and the new kinds together.  It has its own seed base and draws nothing through generate().


def _rowspec2(rng):
    """a row built at a precision of its own: nothing that refers to the resident matrix ("dup") or that is refused ("bad")"""
    u = rng.random()
    if u < 0.15:
        return ("zero",)
    if u < 0.3:
        return ("sat",)
    if u < 0.45:
        return ("uni", int(rng.integers(1 << 30)))
    return ("law", int(rng.integers(1 << 30)), int(10 ** rng.uniform(0.5, 8.6)))


def _groups(rng, n, ng):
    """member lists: about one in four holds 65..300 members (more than a union level takes in one piece: the group is cut
    into chunks whose partial unions are united again), repeated as needed at small n; about one in seven is empty"""
    out = []
    for _ in range(ng):
        u = rng.random()
        size = int(rng.integers(65, 301)) if u < 0.25 else (0 if u < 0.4 else int(rng.integers(1, 7)))
        out.append([int(x) for x in rng.integers(0, n, size)])
    return out


def _mutator2(rng, kind, n, p, attached):
    if kind in MUTATOR_KINDS:
        return _mutator(rng, kind, n, p, attached)
    pre = [("set", n, p, int(rng.integers(1 << 30)), "law")] if attached else []  # (the library writes only into its own)
    cnt = int(rng.integers(1, min(n - 1, 4) + 1))
    first = int(rng.integers(0, n - cnt + 1))
    if kind == "upfold":
        src_p = int(rng.integers(p, min(p + 6, 18) + 1))
        form = str(rng.choice(["host", "device"]))
        return pre + [("upfold", form, first, src_p, [_rowspec2(rng) for _ in range(cnt)])], n, p, False
    if kind == "unite":
        return pre + [("unite", first, _groups(rng, n, cnt))], n, p, False
    raise AssertionError(kind)


def _query2(rng, kind, n, p):
    if kind in QUERY_KINDS:
        return _query(rng, kind, n)
    q = {"estim": int(rng.integers(0, 3)), "rt": int(rng.integers(0, 9)), "k": int(rng.choice([15, 21, 31, 32])),
         "fresh": bool(rng.random() < 0.25), "overlap": bool(rng.random() < 0.25)}
    form = str(rng.choice(["host", "device"]))
    if kind == "fold":
        first = int(rng.integers(0, n))
        q.update(new_p=int(rng.integers(4, p + 1)), first=first, cnt=int(rng.integers(1, n - first + 1)), form=form)
    elif kind == "union":
        q.update(groups=_groups(rng, n, int(rng.integers(1, 6))), form=form)
    elif kind == "thr":
        q["rb"] = int(rng.integers(0, n - 1))
        q["re"] = n if rng.random() < 0.5 else int(rng.integers(q["rb"] + 1, n + 1))
        q["frac"] = str(rng.choice(sorted(FRACS)))
    elif kind == "pairs":
        q.update(seed=int(rng.integers(1 << 30)), m=int(rng.integers(1, 2001)))
    else:  # cluster, greedy: mostly the thresholds at which the graph is neither empty nor whole
        q.update(frac=str(rng.choice(["none", "1/n", "1%", "50%", "all"], p=[0.1, 0.3, 0.3, 0.2, 0.1])), form=form,
                 misalign=int(rng.choice([0, 1, 3])))
    return ("query", kind, q)


def generate2(case, steps=STEPS2):
    """as generate(), over both tables: a first matrix, then `steps` steps of [option] [mutators] query"""
    rng = np.random.default_rng(SEED_BASE2 + case)
    n, p = _shape(rng)
    ops = [("set", n, p, int(rng.integers(1 << 30)), str(rng.choice(["law", "related", "uniform"])))]
    attached = False
    for _ in range(steps):
        if rng.random() < 0.5:
            values = OPTION_VALUES2 if rng.random() < 0.7 else OPTION_VALUES
            name = str(rng.choice(sorted(values)))
            ops.append(("opt", name, int(rng.choice(values[name]))))
        for _ in range(int(rng.choice([0, 1, 2], p=[0.15, 0.6, 0.25]))):
            kind = str(rng.choice(MUTATOR_KINDS2 if rng.random() < 0.3 else MUTATOR_KINDS))
            more, n, p, attached = _mutator2(rng, kind, n, p, attached)
            ops += more
        ops.append(_query2(rng, str(rng.choice(QUERY_KINDS2 if rng.random() < 0.75 else QUERY_KINDS)), n, p))
    return ops


def walk2(ops):
    """per query of a sequence: (kind, kind of the last register mutator since the previous query or None, names of the
    options that were set to ANOTHER value since the previous query, whether a dense call is enqueued in front of it)"""
    out, last_mut, opts = [], None, set()
    cur = dict(OPTION_DEFAULTS, **OPTION_DEFAULTS2)
    for op in ops:
        if op[0] == "query":
            out.append((op[1], last_mut, frozenset(opts), bool(op[2].get("overlap"))))
            last_mut, opts = None, set()
        elif op[0] == "opt":
            if cur[op[1]] != op[2]:
                opts.add(op[1])
            cur[op[1]] = op[2]
        else:
            last_mut = mutator_kind(op)
    return out
