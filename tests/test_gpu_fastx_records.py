"""GPU parity of per-record sketches from raw file bytes (dsh_sketch_fastx_records: the decoder of kernels_fastx.hip with
its record index, then the records kernels).  The expectation is always built the same way: tests/kseq_ref.py::parse gives
the file's records, and the oracle's registers of each record's sequence ALONE give its row; counts, names and rows are
compared by equality.  A refused file (status != 0) writes nothing and counts 0; rows outside the call's span survive."""
import ctypes as C
import os

import numpy as np
import pytest

import dashing_amd
from dashing_amd import api, synth
from fastx_gen import damage, fasta, fastq  # (tests/fastx_gen.py)
from guard import Guarded
from kseq_ref import parse as kseq_parse  # (tests/kseq_ref.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384  # kFastxChunk: the raw bytes of one workgroup of the decoder
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def dna(rng, n):
    return LETTERS[rng.integers(0, 4, n)].tobytes()


def genomes(n, L, seed, decorate=True):
    return [bytes(g) for g in synth.synthetic_genomes(n, L, seed=seed, decorate=decorate)]


def expected(oracle, data, k, p, canon):
    """(names, rows) of one file: kseq's records, the oracle's registers of every record's sequence alone"""
    recs, _ = kseq_parse(data)
    seq, off = synth.concat_for_device([np.frombuffer(q, np.uint8) for _, q in recs])
    rows = oracle.sketch_batch(seq, off, k, p, canon) if recs else np.zeros((0, 1 << p), np.uint8)
    return [n for n, _ in recs], rows


def garbage(rng, n, p):
    return rng.integers(0, 64 - p + 2, (n, 1 << p)).astype(np.uint8)


def check(ctx, oracle, files, k=31, p=10, canon=True, refused=(), pad=2, seed=0, count_first=True):
    """files into the slots [pad, pad + total), every file's span as long as kseq's record count (for a refused file that
    is what its host parse would need); the matrix holds random registers before.  Returns the per-file expectations."""
    rng = np.random.default_rng(seed)
    want = [expected(oracle, f, k, p, canon) for f in files]
    counts = [len(names) for names, _ in want]
    if count_first:
        st, n_rec = ctx.count_fastx_records(files)
        for f in range(len(files)):
            if not st[f]:  # (count-only knows the early refusals alone)
                assert f in refused or int(n_rec[f]) == counts[f], "file %d: counted %d records, kseq reads %d" % (f, n_rec[f], counts[f])
            else:
                assert f in refused and n_rec[f] == 0, "file %d refused in the count" % f
    slot_ptr = np.zeros(len(files) + 1, np.uint64)
    slot_ptr[0] = pad
    slot_ptr[1:] = pad + np.cumsum(counts, dtype=np.uint64)
    total = int(slot_ptr[-1]) - pad
    ctx.alloc(total + 2 * pad, p)
    before = garbage(rng, total + 2 * pad, p)
    ctx.upload(before)
    status, n_rec, names = ctx.sketch_fastx_records(files, slot_ptr, k, canon)
    whole = ctx.download()
    assert (whole[:pad] == before[:pad]).all() and (whole[pad + total:] == before[pad + total:]).all(), "a row outside the span changed"
    for f, (wn, wr) in enumerate(want):
        a, b = int(slot_ptr[f]), int(slot_ptr[f + 1])
        if f in refused:
            assert status[f] != 0, "file %d: expected a refusal" % f
        if status[f]:
            assert f in refused, "file %d: refused (status %d)" % (f, status[f])
            assert n_rec[f] == 0 and (whole[a:b] == before[a:b]).all(), "file %d: refused, yet it reports or writes" % f
            assert all(x == b"" for x in names[a - pad:b - pad])
            continue
        assert int(n_rec[f]) == len(wn), "file %d: %d records, kseq reads %d" % (f, n_rec[f], len(wn))
        assert names[a - pad:b - pad] == wn, "file %d: names differ from kseq's" % f
        bad = np.flatnonzero((whole[a:b] != wr).any(axis=1))
        assert bad.size == 0, "file %d: rows of records %s differ (k=%d p=%d canon=%d)" % (f, bad[:8].tolist(), k, p, canon)
    return want


# ---- FASTA shapes -----------------------------------------------------------------------------------------------------------
def test_fasta_line_widths_and_line_ends(ctx, oracle):
    rng = np.random.default_rng(1)
    g = genomes(1, 60_000, 3)[0]
    recs = lambda tag, a, n, L: [(b"%s_%d text" % (tag, i), g[a + i * L: a + (i + 1) * L]) for i in range(n)]
    files = [
        fasta(rng, recs(b"w1", 0, 3, 1500), 1),
        fasta(rng, recs(b"w60", 100, 4, 4000), 60),
        fasta(rng, recs(b"w63", 200, 4, 4000), 63),
        fasta(rng, recs(b"w64", 300, 4, 4000), 64),
        fasta(rng, recs(b"w65", 400, 4, 4000), 65),
        fasta(rng, recs(b"one", 500, 3, 9000), 0),
        fasta(rng, recs(b"crlf", 600, 4, 4000), 70, eol=b"\r\n"),
        fasta(rng, recs(b"noeol", 700, 3, 4000), 60, final_eol=False),
        fasta(rng, recs(b"blank", 800, 3, 4000), 50, blank_every=3),
    ]
    check(ctx, oracle, files)


def test_fasta_record_shapes_headers_and_names(ctx, oracle):
    rng = np.random.default_rng(2)
    g = genomes(1, 50_000, 5)[0]
    long_name = bytes(rng.integers(33, 126, 40000, dtype=np.uint8))
    files = [
        fasta(rng, [(b"short", b"ACGT"), (b"empty", b""), (b"real", g[:9000]), (b"tail", b"ACGTACGTAC"), (b"e2", b""), (b"e3", b"")], 80),
        b">a\n>b\n",
        fasta(rng, [(b"", g[:3000]), (b"x", g[3000:6000])], 80),                     # headers of one byte / one name byte
        fasta(rng, [(long_name, g[:5000]), (b"after", g[5000:8000])], 80),          # a header longer than two chunks
        b">  x y\n" + g[:200] + b"\n>b\rq\n" + g[200:500] + b"\n>a\tc\n" + g[500:900] + b"\n",  # an empty name, '\r' and tab end a name
        b">a\n" + g[:5000] + b"\n@b also a header\n" + g[5000:9000] + b"\n",          # '@' heads a record of a FASTA file too
        b">",
        b">a\nACGT\n>",
        b">a\nACGT\n>\n",
        b">no sequence, no newline",
        b"",
        fasta(rng, [(b"h", g[:4000])], 60) + b">",                                   # a header character as the last byte
    ]
    want = check(ctx, oracle, files, k=3)
    assert [len(w[0]) for w in want][6:11] == [0, 1, 2, 1, 0]
    assert want[8][0] == [b"a", b""] and want[9][0] == [b"no"] and want[4][0] == [b"", b"b", b"a"]
    check(ctx, oracle, files, k=21, count_first=False)


def test_a_header_start_on_every_byte_of_a_lane_and_on_chunk_edges(ctx, oracle):
    """the second record's header character at raw offset x: the in-lane rank (x mod 64), the wave and workgroup prefix
    (which lane), the chunk base (16383, 16384, 16385, 32768) -- placed by the length of the sequence line in front"""
    rng = np.random.default_rng(3)
    g = dna(rng, 40_000)
    files = []
    for x in [64 * 67 + o for o in range(64)] + [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK]:
        t = b">a\n" + g[: x - 4] + b"\n>b second\n" + g[x: x + 700] + b"\n>c\n" + g[100:160] + b"\n"
        assert t[x: x + 2] == b">b"
        files.append(t)
    check(ctx, oracle, files, k=21)


def test_more_records_than_a_run_holds_and_a_long_record_between_tiny_ones(ctx, oracle):
    """5 000 records of 1 to 3 bases in one file -- more than kRecRunRecs and kRecRunSegs within one run's reach -- and a
    record longer than kRecRunSpan between tiny ones, in one call"""
    rng = np.random.default_rng(4)
    g = dna(rng, 30_000)
    tiny = [(b"t%d" % i, g[i: i + 1 + i % 3]) for i in range(5000)]
    mixed = [(b"a", b"AC"), (b"b", b"G"), (b"long", g[:9000]), (b"c", b"T"), (b"d", b"ACG")]
    check(ctx, oracle, [fasta(rng, tiny, 60), fasta(rng, mixed, 60)], k=1, p=8)


def test_a_file_of_many_chunks(ctx, oracle):
    """more than 256 chunks: k_fastx_offsets walks several chunks per lane, the chunk's first record number is a prefix sum"""
    rng = np.random.default_rng(5)
    g = dna(rng, 100_000)
    recs = [(b"r%05d" % i, g[(i * 37) % 90_000: (i * 37) % 90_000 + 205]) for i in range(20_000)]
    data = fasta(rng, recs, 0)
    assert len(data) >= 257 * CHUNK
    check(ctx, oracle, [data], k=21, p=8)


# ---- FASTQ ------------------------------------------------------------------------------------------------------------------
def test_fastq_shapes(ctx, oracle):
    """reads of 1 to 400 bases, of 16383 / 16384 / 20000, CRLF, no final newline, quality lines that begin with '@' '+' '>',
    and the ways a text can end.  kseq_ref gives ONE record (name b"only", no sequence) for b"@only a header" -- a name was
    read before the end of the file --, and none for b"@": the expectation is kseq's, so the device must count that
    header-without-newline although no marker byte stands for it."""
    rng = np.random.default_rng(7)
    g = genomes(1, 120_000, 13)[0]

    def reads(lens):
        out, at = [], 0
        for L in lens:
            out.append(g[at: at + L])
            at = (at + L) % (len(g) - 30000)
        return out

    nasty = lambda i, L: (b"@+>@"[i % 4: i % 4 + 1] + bytes(rng.integers(33, 75, max(L - 1, 0), dtype=np.uint8)))[:L]
    good = fastq(rng, reads([150] * 40))
    files = [
        fastq(rng, reads([int(x) for x in rng.integers(1, 400, 150)]), qual=nasty),
        fastq(rng, reads([16383, 16384, 20000, 17, 63, 64, 65])),
        fastq(rng, reads([100] * 60), eol=b"\r\n"),
        fastq(rng, reads([250] * 30), final_eol=False),
        b"@only a header",
        b"@r\n",
        good + b"@s\n",
        good + b"@s",      # ends inside a header line: kseq reads one more, empty record
        good + b"@",       # ... kseq's ordinary end of file
        b"@x",
    ]
    want = check(ctx, oracle, files, k=21)
    assert [len(w[0]) for w in want][4:10] == [1, 1, 41, 41, 40, 1]


# ---- parameters -------------------------------------------------------------------------------------------------------------
def _mixed(seed):
    rng = np.random.default_rng(seed)
    g = genomes(1, 40_000, 21 + seed)[0]
    lens = [0, 1, 20, 21, 30, 31, 32, 33, 150, 9000, 3, 700]
    recs, at = [], 0
    for i, L in enumerate(lens):
        recs.append((b"r%d" % i, g[at: at + L]))
        at += L
    return [fasta(rng, recs, 61), fastq(rng, [g[i * 300: i * 300 + 1 + 11 * i] for i in range(40)]), fasta(rng, recs[::-1], 0, eol=b"\r\n")]


@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("k", [1, 21, 31, 32])
def test_k_and_canon(ctx, oracle, k, canon):
    check(ctx, oracle, _mixed(1), k=k, p=10, canon=canon, count_first=False)


@pytest.mark.parametrize("p", [8, 10, 14, 17, 18])
def test_precisions(ctx, oracle, p):
    """p = 18 is above the records kernel: every record goes through k_sketch's genome route, its row cleared first"""
    check(ctx, oracle, _mixed(2), k=31, p=p, count_first=False)


# ---- several files, refusals, the caller's buffers ------------------------------------------------------------------------
def _refused_pair(rng, g):
    rd = [g[i * 200: (i + 1) * 200] for i in range(50)]
    late = fastq(rng, rd[:20]) + b"@x\n" + rd[20] + b"\n+\n" + b"I" * 150 + b"\n" + fastq(rng, rd[21:])  # (the length fingerprint)
    plus = fasta(rng, [(b"plus line", g[:6000])], 80) + b"+\nIIII\n"                                      # (early: a '+' line in FASTA)
    return late, plus


def test_accepted_and_refused_files_interleaved_write_their_spans_only(ctx, oracle):
    rng = np.random.default_rng(8)
    g = genomes(1, 60_000, 17, decorate=False)[0]
    late, plus = _refused_pair(rng, g)
    fa = fasta(rng, [(b"c%d x" % i, g[i * 3000: i * 3000 + 2500]) for i in range(6)], 70)
    fq = fastq(rng, [g[i * 150: (i + 1) * 150] for i in range(30)])
    files = [fa, late, fq, plus, fa[: len(fa) // 2], b"", fq]
    refused = {1, 3}
    k, p, pad = 21, 10, 3
    want = [expected(oracle, f, k, p, True) for f in files]
    counts = [len(w[0]) for w in want]
    slot_ptr = np.zeros(len(files) + 1, np.uint64)
    slot_ptr[0] = pad
    slot_ptr[1:] = pad + np.cumsum(counts, dtype=np.uint64)
    total = int(slot_ptr[-1]) - pad
    n = total + 2 * pad
    # every row pre-filled by an earlier sketch call
    ctx.alloc(n, p)
    fill = [np.frombuffer(dna(rng, 400), np.uint8) for _ in range(n)]
    seq, off = synth.concat_for_device(fill)
    before = ctx.sketch_batch(seq, off, 0, k, True)
    assert before.any(axis=1).all()
    raw, roff, lens = ctx._fastx_regions(files)
    status = Guarded(len(files), np.uint32)
    n_rec = Guarded(len(files), np.uint64)
    hdr = Guarded(total, np.uint64)
    ctx._ck(ctx._lib.dsh_sketch_fastx_records(ctx._h, raw.ctypes.data, roff.ctypes.data, lens.ctypes.data, len(files), slot_ptr.ctypes.data,
                                              k, 1, status.ptr, n_rec.ptr, hdr.ptr))
    for gd, what in ((status, "status_out"), (n_rec, "n_rec_out"), (hdr, "hdr_off_out")):
        gd.check(what)
    assert status.unwritten() == 0 and n_rec.unwritten() == 0
    st, nr, ho = status.host(), n_rec.host(), hdr.host()
    whole = ctx.download()
    assert (whole[:pad] == before[:pad]).all() and (whole[pad + total:] == before[pad + total:]).all()
    buf = raw.tobytes()
    for f, (wn, wr) in enumerate(want):
        a, b = int(slot_ptr[f]), int(slot_ptr[f + 1])
        assert bool(st[f]) == (f in refused), "file %d: status %d" % (f, st[f])
        if st[f]:
            assert nr[f] == 0 and (whole[a:b] == before[a:b]).all()
            assert (ho[a - pad:b - pad] == np.uint64(hdr.scan)).all(), "a refused file wrote a header offset"
            continue
        assert int(nr[f]) == len(wn) and (whole[a:b] == wr).all()
        for r, name in enumerate(wn):
            h = int(ho[a - pad + r])
            assert int(roff[f]) <= h < int(roff[f]) + len(files[f]) and buf[h: h + 1] in (b">", b"@")
            assert buf[h + 1: h + 1 + len(name)] == name


def test_count_only_needs_no_matrix(oracle):
    rng = np.random.default_rng(9)
    g = genomes(1, 30_000, 19)[0]
    late, plus = _refused_pair(rng, g)
    files = [fasta(rng, [(b"r%d" % i, g[i * 100: i * 100 + 90]) for i in range(200)], 60), fastq(rng, [g[i * 50: i * 50 + 50] for i in range(77)]),
             plus, b"", b">", b"@x", late]
    with dashing_amd.Context(0) as fresh:  # before dsh_sketches_alloc
        st, nr = fresh.count_fastx_records(files)
        assert [int(x) for x in nr[:6]] == [200, 77, 0, 0, 0, 1] and [bool(x) for x in st[:6]] == [False, False, True, False, False, False]
        assert not st[6]  # (a late refusal is not known to the count)
        with pytest.raises(dashing_amd.DshError) as e:
            fresh.sketch_fastx_records(files, np.arange(len(files) + 1))
        assert e.value.code == -11  # DSH_ESTATE: the full call needs the matrix
    assert [len(kseq_parse(f)[0]) for f in files[:6]] == [int(x) for x in nr[:6]]


@pytest.mark.parametrize("delta", [-1, 1])
def test_a_span_of_the_wrong_size_is_reported_and_nothing_written(ctx, oracle, delta):
    rng = np.random.default_rng(10)
    g = genomes(1, 30_000, 23)[0]
    files = [fasta(rng, [(b"a%d" % i, g[i * 500: i * 500 + 400]) for i in range(5)], 60),
             fastq(rng, [g[i * 90: i * 90 + 80] for i in range(9)]),
             fasta(rng, [(b"c%d" % i, g[i * 300: i * 300 + 300]) for i in range(7)], 0)]
    spans = [5, 9 + delta, 7]
    slot_ptr = np.concatenate([[1], 1 + np.cumsum(spans)]).astype(np.uint64)
    ctx.alloc(int(slot_ptr[-1]) + 1, 10)
    before = garbage(rng, ctx.n, 10)
    ctx.upload(before)
    with pytest.raises(dashing_amd.DshError) as e:
        ctx.sketch_fastx_records(files, slot_ptr, 21)
    assert e.value.code == api.ERANGE and "file 1" in str(e.value) and "9 records" in str(e.value)
    assert e.value.n_rec.tolist() == [5, 9, 7] and not e.value.status.any()
    assert (ctx.download() == before).all(), "a row changed although the call reported DSH_ERANGE"


def test_equals_sketch_records_on_the_host_parsers_records(ctx, oracle, tmp_path):
    host = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    host.dshh_append_fastx_records.restype = C.c_long
    host.dshh_append_fastx_records.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    for i, data in enumerate(_mixed(3)):
        pth = tmp_path / ("f%d" % i)
        pth.write_bytes(data)
        buf, starts, names, n = np.zeros(len(data) + 64, np.uint8), np.zeros(4096, np.uint64), C.create_string_buffer(1 << 16), C.c_size_t(0)
        nrec = host.dshh_append_fastx_records(str(pth).encode(), buf.ctypes.data, buf.size, C.byref(n), starts.ctypes.data, starts.size, names, len(names))
        assert nrec > 0
        off = np.concatenate([starts[:nrec], [n.value]]).astype(np.uint64)
        ctx.alloc(nrec, 10)
        via_host = ctx.sketch_records(buf[: n.value], off, 0, 21)
        ctx.upload(garbage(np.random.default_rng(i), nrec, 10))
        st, nr, got_names = ctx.sketch_fastx_records([data], [0, nrec], 21)
        assert not st[0] and int(nr[0]) == nrec
        assert (ctx.download() == via_host).all()
        assert b"\n".join(got_names) == names.value.rstrip(b"\n")


def test_argument_errors_launch_nothing(ctx):
    rng = np.random.default_rng(11)
    data = fasta(rng, [(b"a", dna(rng, 500)), (b"b", dna(rng, 500))], 60)
    ctx.alloc(6, 10)
    before = garbage(rng, 6, 10)
    ctx.upload(before)
    raw = np.full(4096, 0x4E, np.uint8)
    raw[: len(data)] = np.frombuffer(data, np.uint8)
    raw[2048: 2048 + len(data)] = np.frombuffer(data, np.uint8)
    st, nr, hdr = np.zeros(2, np.uint32), np.zeros(2, np.uint64), np.zeros(8, np.uint64)
    u64 = lambda *v: np.array(v, np.uint64)

    def call(off, lens, slots, k=21):
        return ctx._lib.dsh_sketch_fastx_records(ctx._h, raw.ctypes.data, off.ctypes.data, lens.ctypes.data, 2, slots.ctypes.data if slots is not None else None,
                                                 k, 1, st.ctypes.data, nr.ctypes.data, hdr.ctypes.data)

    good_off, good_len, good_slots = u64(0, 2048, 4096), u64(len(data), len(data)), u64(1, 3, 5)
    EINVAL = -22
    assert call(u64(0, 2040, 4096), good_len, good_slots) == EINVAL       # a region not on a multiple of 32
    assert call(good_off, u64(len(data), 2049), good_slots) == EINVAL      # raw_len beyond the region
    assert call(good_off, good_len, u64(1, 4, 3)) == EINVAL                # slot_ptr decreases
    assert call(good_off, good_len, u64(3, 5, 7)) == EINVAL                # slots out of range
    assert call(good_off, good_len, good_slots, k=0) == EINVAL
    assert call(good_off, good_len, good_slots, k=33) == EINVAL
    assert call(good_off, good_len, None, k=33) == EINVAL                  # count-only checks the same
    assert call(u64(0, 2040, 4096), good_len, None) == EINVAL
    assert (ctx.download() == before).all() and not st.any() and not nr.any() and not hdr.any()
    assert call(good_off, good_len, good_slots) == 0 and nr.tolist() == [2, 2]


# ---- fuzz ---------------------------------------------------------------------------------------------------------------------
FUZZ_SEED, FUZZ_CASES, FUZZ_FILES = 0xF0A5, 40, 6


def fuzz_case(case):
    """the case's texts, built like test_gpu_fastx.py's fuzz (shorter sequences): (files, undamaged flags, p, k)"""
    rng = np.random.default_rng(FUZZ_SEED + case)
    g = genomes(1, 20_000, 2000 + case, decorate=bool(case & 1))[0]
    files, undamaged = [], []
    for f in range(FUZZ_FILES):
        eol = b"\r\n" if rng.random() < 0.2 else b"\n"
        if rng.random() < 0.5:  # FASTA
            nrec = int(rng.integers(1, 6))
            cuts = sorted(set([0, len(g)] + [int(x) for x in rng.integers(0, len(g), nrec - 1)]))
            recs = [(bytes(rng.integers(33, 126, int(rng.integers(0, 90)), dtype=np.uint8)), g[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
            data = fasta(rng, recs, int(rng.choice([0, 1, 7, 60, 63, 64, 65, 80, 200, 5000])), eol=eol, final_eol=bool(rng.random() < 0.7),
                         blank_every=int(rng.choice([0, 0, 3, 11])))
        else:  # FASTQ
            lens = [int(x) for x in rng.integers(1, int(rng.choice([50, 300, 3000])), int(rng.integers(1, 60)))]
            at, rds = 0, []
            for L in lens:
                rds.append(g[at: at + L])
                at = (at + L) % (len(g) - 3000)
            data = fastq(rng, rds, eol=eol, final_eol=bool(rng.random() < 0.7))
        ok = True
        if rng.random() < 0.5:
            data = damage(rng, data, eol)
            ok = False
        files.append(data)
        undamaged.append(ok)
    return files, undamaged, int(rng.choice([8, 10, 12])), int(rng.choice([5, 21, 31, 32]))


@pytest.mark.parametrize("case", range(FUZZ_CASES))
def test_fuzz_accepted_means_kseqs_records(ctx, oracle, case):
    """well-formed and damaged texts: whatever the device ACCEPTS gives kseq's count, names and every row; what is
    undamaged must be accepted; what is refused changes nothing"""
    files, undamaged, p, k = fuzz_case(case)
    rng = np.random.default_rng(case)
    want = [expected(oracle, f, k, p, True) for f in files]
    st0, nr0 = ctx.count_fastx_records(files)
    # spans as a caller would lay them out: the device's count where it accepts, kseq's (the host parse) where it refuses
    counts = [int(nr0[f]) if not st0[f] else len(want[f][0]) for f in range(len(files))]
    slot_ptr = np.concatenate([[1], 1 + np.cumsum(counts)]).astype(np.uint64)
    ctx.alloc(int(slot_ptr[-1]) + 1, p)
    before = garbage(rng, ctx.n, p)
    ctx.upload(before)
    try:
        status, n_rec, names = ctx.sketch_fastx_records(files, slot_ptr, k)
    except dashing_amd.DshError as e:  # only a LATE refusal may move a count between the two calls
        assert e.code == api.ERANGE
        raise AssertionError("case %d: the count-only call and the full call disagree: %s" % (case, e))
    whole = ctx.download()
    assert (whole[0] == before[0]).all() and (whole[-1] == before[-1]).all()
    for f, (wn, wr) in enumerate(want):
        a, b = int(slot_ptr[f]), int(slot_ptr[f + 1])
        if undamaged[f]:
            assert status[f] == 0, "case %d file %d: a well-formed file was refused" % (case, f)
        if status[f]:
            assert n_rec[f] == 0 and (whole[a:b] == before[a:b]).all(), "case %d file %d: refused, yet it reports or writes" % (case, f)
            continue
        assert int(n_rec[f]) == len(wn), "case %d file %d: %d records, kseq reads %d" % (case, f, n_rec[f], len(wn))
        assert names[a - 1:b - 1] == wn, "case %d file %d: names" % (case, f)
        assert (whole[a:b] == wr).all(), "case %d file %d: accepted, but rows differ from kseq's" % (case, f)


def test_fuzz_does_not_pass_empty(ctx):
    """what keeps the 40 cases from passing empty: at least 30 % of their files are undamaged by construction (one half is
    expected), and the device accepts at least one DAMAGED file -- damage() can leave a well-formed text, for example a
    doubled blank line in FASTA (a FASTA file has no late refusal: the count-only call's verdict is the full call's)"""
    built = [fuzz_case(case) for case in range(FUZZ_CASES)]
    n_files = sum(len(files) for files, _, _, _ in built)
    n_undamaged = sum(sum(undamaged) for _, undamaged, _, _ in built)
    assert n_undamaged >= 0.3 * n_files, (n_undamaged, n_files)
    damaged = [f for files, undamaged, _, _ in built for f, ok in zip(files, undamaged) if not ok and f[:1] == b">"]
    status, _ = ctx.count_fastx_records(damaged)
    assert (status == 0).any(), "no damaged file among %d was accepted" % len(damaged)
