"""Every register value at every precision, by made k-mers (tests/kmer_cases.py): k_sketch, k_sketch_records, the device
FASTA decode and the fold, held to the registers that follow from the CONSTRUCTION of the hash -- one_hot, or the
byte-wise maximum of several -- and to the oracle.  Random genomes never raise a register above about 20, but the kernels
branch above that: the FAST instances (p <= 15) repair a zero high word of t = (h << p) | guard behind the sub-chunk, the
packed-byte (p = 16, 17) and GLOBAL (p >= 18) instances take min(zh, zl + 32) with a hand-written shift-or, the guard bit
alone tells q = 64 - p from q + 1, and the byte registers are raised by a CAS on the containing word.  Everything here
is compared for equality; every input is a legal sequence."""
import functools

import numpy as np
import pytest

import kmer_cases as kc
import oracle.oracle_py as opy
from dashing_amd import synth
from hashinv import revcomp

pytestmark = pytest.mark.gpu
PS = range(4, 25)
KCS = [(31, True), (31, False), (32, True), (32, False)]
NN = ord("N")
SUB = 8192  # bases of a sub-chunk of the work list; a step of k_sketch's loop is 1, 2 or 4 of them


def ns(n):
    return np.full(n, NN, np.uint8)


def acgt(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]


@functools.lru_cache(maxsize=None)
def made(p, k, canon):
    """one k-mer per value of V(p), the walk over the indices started somewhere else for each: [(x, index, value)]"""
    out = []
    for v in kc.V(p):
        x, idx = kc.make(p, v, k, canon, start=kc.spread(p, v, k, canon))
        out.append((x, idx, v))
    return out


def isolated(p, k, canon):
    """genomes that hold one made k-mer and no other valid k-mer: the bare k-mer for every value of V(p), and for 32, 33 and
    q + 1 also the k-mer behind 1, 31, 32 and 33 bytes of N with an N after it (other lanes, other offsets in the lane's
    words, the zero-word repair loop at j != 0): [(text, index, value)]"""
    out = []
    for x, idx, v in made(p, k, canon):
        t = kc.text(x, k)
        out.append((t, idx, v))
        if v in (32, 33, 64 - p + 1):
            out += [(np.concatenate([ns(lead), t, ns(1)]), idx, v) for lead in (1, 31, 32, 33)]
    return out


def assert_rows(got, want_hot, oracle_rows, what):
    """both references, exactly: the construction's rows (list of arrays) and the oracle's"""
    assert got.shape == oracle_rows.shape
    for g, hot in enumerate(want_hot):
        assert np.array_equal(oracle_rows[g], hot), ("the ORACLE differs from the construction", what, g)
        if not np.array_equal(got[g], hot):
            at = np.flatnonzero(got[g] != hot)[:4]
            raise AssertionError("%s: row %d differs from the construction at %s: got %s, want %s"
                                 % (what, g, at.tolist(), got[g][at].tolist(), hot[at].tolist()))


# ---- a. isolated k-mers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,canon", KCS)
@pytest.mark.parametrize("p", PS)
def test_isolated_kmers_of_every_value(ctx, oracle, p, k, canon):
    """p <= 13: FAST with 256 lanes, p = 14: 512, p = 15: 1 024 (k = 31: the specialised window; k = 32: the general one);
    p = 16, 17: packed bytes with 512 and 1 024 lanes; p >= 18: GLOBAL."""
    cases = isolated(p, k, canon)
    seq, off = synth.concat_for_device([t for t, _, _ in cases])
    ctx.alloc(len(cases), p)
    got = ctx.sketch_batch(seq, off, 0, k, canon)
    assert_rows(got, [kc.one_hot(p, idx, v) for _, idx, v in cases], oracle.sketch_batch(seq, off, k, p, canon), (p, k, canon))


# ---- b. strands ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS)
def test_reverse_complement_texts(ctx, oracle, p):
    """canonical: the same row; not canonical: the row of the reverse complement's own hash, another one"""
    for k, canon in KCS:
        ms = made(p, k, canon)
        seq, off = synth.concat_for_device([kc.rc_text(x, k) for x, _, _ in ms])
        want = []
        for x, idx, v in ms:
            ridx, rv = (idx, v) if canon else kc.rule(opy.wang(revcomp(x, k)), p)
            assert canon or (ridx, rv) != (idx, v)
            want.append(kc.one_hot(p, ridx, rv))
        ctx.alloc(len(ms), p)
        got = ctx.sketch_batch(seq, off, 0, k, canon)
        assert_rows(got, want, oracle.sketch_batch(seq, off, k, p, canon), (p, k, canon))


# ---- c. one word, several bytes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [10, 15, 16, 17, 18, 24])
def test_several_registers_of_one_word_raised_together(ctx, oracle, p):
    """Four k-mers for the four registers 4j ... 4j + 3 of one 32-bit word of the row, four different values, and for two of
    the registers a second k-mer, one smaller and one larger: in one genome, N-separated, so that their start positions
    lie in neighbouring lanes of one wave (k + 1 apart); in reverse order; in two calls on the same slot; and in two work
    items of one genome (two workgroups merging into the row).  The row is the byte-wise maximum every time, on top of
    what the row held: the registers beside the word, and a larger value inside it, keep theirs.  (A call takes genome g
    to slot first_slot + g, so two GENOMES of one slot in one call cannot be said: two work items of one genome are what
    one call can make of it.)"""
    q = 64 - p
    rng = np.random.default_rng(p)
    for k, canon in [(31, True), (32, False)]:
        base = 4 * (1 + kc.spread(p - 3, p, k))
        vals = [5, min(34, q - 8), 20, 11]
        picks = [(base + i, vals[i], 0) for i in range(4)] + [(base, 2, 0), (base + 2, 27, 0)]
        texts, hot = [], np.zeros(1 << p, np.uint8)
        for idx, v, skip in picks:
            x, got_idx = kc.make(p, v, k, canon, index=idx, skip=skip)
            assert got_idx == idx and kc.rule(opy.wang(x), p) == (idx, v)
            texts.append(kc.text(x, k))
            hot = np.maximum(hot, kc.one_hot(p, idx, v))
        assert hot[base:base + 4].tolist() == [5, vals[1], 27, 11]

        def joined(ts):
            return np.concatenate([np.concatenate([t, ns(1)]) for t in ts])

        before = np.zeros((3, 1 << p), np.uint8)
        before[0] = rng.integers(0, q + 2, 1 << p)
        before[2] = rng.integers(0, q + 2, 1 << p)
        before[1, base - 1], before[1, base + 4], before[1, base + 3] = 7, 9, 40   # (40 > 11: stays)
        want = np.maximum(before[1], hot)
        assert want[base - 1:base + 5].tolist() == [7, 5, vals[1], 27, 40, 9]
        calls = {
            "forward": [joined(texts)],
            "reverse": [joined(texts[::-1])],
            "two calls": [joined(texts[:3]), joined(texts[3:])],
            "two work items": [np.concatenate([joined(texts[:3]), ns(16 * SUB), joined(texts[3:])])],
        }
        ctx.alloc(3, p)
        for name, genomes in calls.items():
            ctx.upload(before)
            orow = before[1].copy()
            for g in genomes:
                seq, off = synth.concat_for_device([g])
                ctx.sketch_batch(seq, off, 1, k, canon, want_regs=False)
                orow = np.maximum(orow, oracle.sketch_batch(seq, off, k, p, canon)[0])
            whole = ctx.download()
            assert np.array_equal(orow, want), ("the ORACLE differs from the construction", p, k, name)
            assert np.array_equal(whole[1], want), (p, k, name, whole[1][base - 1:base + 5].tolist(), want[base - 1:base + 5].tolist())
            assert np.array_equal(whole[0], before[0]) and np.array_equal(whole[2], before[2]), (p, k, name)


# ---- d. steps of 16 384 and 32 768 bases -----------------------------------------------------------------------------
@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("k", [31, 32])
@pytest.mark.parametrize("p", [14, 15, 16, 17])
def test_planted_in_genomes_of_several_steps(ctx, oracle, p, k, canon):
    """p = 14 and 16 walk 16 384 bases per step, p = 15 and 17 walk 32 768.  Random ACGT with made k-mers of value >= 33
    and of value exactly 32 on both step grids (counted from the 32-aligned base in front of the genome): s - k, s,
    s - k + 1, s + 31, s - 5; the first start position of the item's last step and the last k bases of the genome; right
    behind an N; one that straddles the end of a work item of 16 sub-chunks and one right behind that end, whose lanes
    belong to the next item.  Genome 0 starts at offset 13 and is three of the larger steps and a ragged tail, genome 1
    ends one sub-chunk into its second step, genome 2 is two work items."""
    q = 64 - p
    step = 16384 if p in (14, 16) else 32768
    rng = np.random.default_rng(100 * p + 2 * k + canon)
    lead = 13
    lens = [3 * 32768 + 1234 - lead, 0, 0]
    starts = [lead]                                              # absolute offsets of the genomes
    c0 = [lead & ~31]
    starts.append(starts[0] + lens[0])
    c0.append(starts[1] & ~31)
    lens[1] = c0[1] + step + SUB - 57 - starts[1]
    starts.append(starts[1] + lens[1])
    c0.append(starts[2] & ~31)
    lens[2] = c0[2] + 17 * SUB + 777 - starts[2]
    seq = acgt(rng, lead + sum(lens)).copy()
    off = np.array([starts[0], starts[1], starts[2], starts[2] + lens[2]], np.uint64)

    spots = []  # (genome, absolute start)
    for s, (m0, m1, m2) in ((16384, (1, 3, 5)), (32768, (1, 2, 3))):   # genome 0: both grids, three boundaries of each
        spots += [(0, c0[0] + m0 * s - k), (0, c0[0] + m0 * s), (0, c0[0] + m1 * s - k + 1), (0, c0[0] + m1 * s + 31), (0, c0[0] + m2 * s - 5)]
    spots += [(1, c0[1] + step), (1, starts[1] + lens[1] - k), (1, starts[1] + 5000), (1, starts[1])]
    item_end = c0[2] + 16 * SUB
    spots += [(2, item_end - 5), (2, item_end + 64), (2, item_end - 2 * k - 1), (2, starts[2] + lens[2] - k)]
    values = [33, 32, 34, 32, q + 1, 32, q, 33, q - 1, 32]
    planted, used = [], set()
    for n, (g, at) in enumerate(spots):
        v = values[n % len(values)]
        x, idx = kc.make(p, v, k, canon, start=kc.spread(p, n, k, canon))
        while idx in used:  # (every planted k-mer a register of its own)
            x, idx = kc.make(p, v, k, canon, start=idx + 1)
        used.add(idx)
        assert starts[g] <= at and at + k <= starts[g] + lens[g]
        assert not any(g == g2 and abs(at - at2) < k for g2, at2, _, _ in planted), "two planted k-mers overlap"
        seq[at:at + k] = kc.text(x, k)
        planted.append((g, at, idx, v))
    seq[starts[1] + 5000 - 1] = NN

    ctx.alloc(3, p)
    got = ctx.sketch_batch(seq, off, 0, k, canon)
    want = oracle.sketch_batch(seq, off, k, p, canon)
    for g, at, idx, v in planted:
        assert want[g][idx] == v, ("the oracle does not show a planted k-mer", g, at, idx, v, int(want[g][idx]))
        assert got[g][idx] == v, ("planted k-mer", g, at - c0[g], idx, v, int(got[g][idx]))
    assert (got == want).all(), "registers differ in %d places" % int((got != want).sum())


# ---- e. records ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 10, 13, 15, 17, 18])
def test_isolated_kmers_as_records(ctx, oracle, p):
    """k_sketch_records (p <= 17: the exact 64-bit rule per start position) and the GLOBAL k_sketch behind a row clear
    (p = 18); empty records and records shorter than k in between give zero rows; the rows on both sides survive"""
    rng = np.random.default_rng(p)
    for k, canon in KCS:
        recs, want = [], []
        for n, (t, idx, v) in enumerate(isolated(p, k, canon)):
            recs.append(t)
            want.append(kc.one_hot(p, idx, v))
            if n % 3 == 0:
                recs.append(acgt(rng, 0))
            if n % 3 == 1:
                recs.append(acgt(rng, [5, k - 1][n % 2]))
            if n % 3 != 2:
                want.append(np.zeros(1 << p, np.uint8))
        seq, off = synth.concat_for_device(recs)
        pad, n = 2, len(recs)
        before = rng.integers(0, 64 - p + 2, (n + 2 * pad, 1 << p)).astype(np.uint8)
        ctx.alloc(n + 2 * pad, p)
        ctx.upload(before)
        got = ctx.sketch_records(seq, off, pad, k, canon)
        assert_rows(got, want, oracle.sketch_batch(seq, off, k, p, canon), (p, k, canon))
        whole = ctx.download()
        assert (whole[:pad] == before[:pad]).all() and (whole[pad + n:] == before[pad + n:]).all(), "a neighbouring slot changed"
        assert (whole[pad:pad + n] == got).all()


# ---- f. device FASTA decode ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [10, 15, 18])
def test_isolated_kmers_as_fasta_files(ctx, oracle, p):
    """a header, the sequence on one line; for two of the files split over two lines"""
    for k, canon in KCS:
        cases = isolated(p, k, canon)
        files = []
        for n, (t, _, _) in enumerate(cases):
            s = t.tobytes()
            body = s[:17] + b"\n" + s[17:] if n in (1, 3) else s
            files.append(b">made %d\n" % n + body + b"\n")
        ctx.alloc(len(files), p)
        status = ctx.sketch_fastx_batch(files, 0, k, canon)
        assert not status.any(), status.tolist()
        seq, off = synth.concat_for_device([t for t, _, _ in cases])
        assert_rows(ctx.download(), [kc.one_hot(p, idx, v) for _, idx, v in cases], oracle.sketch_batch(seq, off, k, p, canon), (p, k, canon))


# ---- g. fold against sketching ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,new_p", [(5, 4), (14, 10), (15, 4), (17, 7), (24, 4), (24, 14)])
def test_fold_is_what_sketching_at_the_lower_precision_gives(ctx, oracle, p, new_p):
    """k-mers made for new_p, sketched at p and folded: values <= d = p - new_p come from the dropped index bits
    (d - msb(low)), larger ones from v0 + d, up to the cap q' + 1 of the all-zero tail.  One k-mer per row, and all of them
    in the last row."""
    d, nq = p - new_p, 64 - new_p
    values = sorted(v for v in {1, d, d + 1, d + 2, 33, nq, nq + 1} if 1 <= v <= nq + 1)
    for k, canon in [(31, True), (32, False)]:
        texts, want = [], []
        for v in values:
            x, idx = kc.make(new_p, v, k, canon, start=kc.spread(new_p, v, k, p))
            texts.append(kc.text(x, k))
            want.append(kc.one_hot(new_p, idx, v))
        texts.append(np.concatenate([np.concatenate([t, ns(1)]) for t in texts]))
        want.append(np.maximum.reduce(want))
        seq, off = synth.concat_for_device(texts)
        ctx.alloc(len(texts), p)
        at_p = ctx.sketch_batch(seq, off, 0, k, canon)
        assert (at_p == oracle.sketch_batch(seq, off, k, p, canon)).all()
        folded = ctx.fold(new_p)
        ctx.alloc(len(texts), new_p)
        direct = ctx.sketch_batch(seq, off, 0, k, canon)
        orows = oracle.sketch_batch(seq, off, k, new_p, canon)
        assert_rows(direct, want, orows, ("sketched at", new_p, k, canon))
        assert_rows(folded, want, orows, ("folded from", p, new_p, k, canon))
