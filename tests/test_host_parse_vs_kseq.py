"""The host reader (host/host.cpp FastxParser through libdashing_host.so) against the kseq port tests/kseq_ref.py, on hand
cases, on every compression the reader opens, on a seeded fuzz of damaged files and where structure straddles the reader's
1 MiB read block.  Both modes: dshh_append_fastx (records joined by one 'N') and dshh_append_fastx_records (record starts
and names).  The reader is a port of kseq_read, so the records agree byte for byte; their ACGT runs -- all the encoder
sees -- are compared as well."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from fastx_gen import damage, random_text  # (tests/fastx_gen.py)
from kseq_ref import all_runs, parse, runs  # (tests/kseq_ref.py)
from test_kseq_ref import CASES as KSEQ_CASES  # the hand cases, with their expectations written out by hand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 1 << 20  # host.cpp kFastxReadBlock


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.environ.get("DSH_HOST_LIB", os.path.join(ROOT, "dashing_amd", "libdashing_host.so")))
    cp, vp, sz = C.c_char_p, C.c_void_p, C.c_size_t
    lib.dshh_append_fastx.restype = C.c_long
    lib.dshh_append_fastx.argtypes = [cp, vp, sz, C.POINTER(sz)]
    lib.dshh_append_fastx_records.restype = C.c_long
    lib.dshh_append_fastx_records.argtypes = [cp, vp, sz, C.POINTER(sz), vp, sz, vp, sz]
    return lib


def stream(host, path, cap):
    out = np.zeros(cap, np.uint8)
    n = C.c_size_t(0)
    r = host.dshh_append_fastx(path.encode(), out.ctypes.data, cap, C.byref(n))
    assert r >= 0, r
    return r, out[: n.value].tobytes()


def records(host, path, cap, nmax):
    out = np.zeros(cap, np.uint8)
    n = C.c_size_t(0)
    starts = np.zeros(nmax + 1, np.uint64)
    names = C.create_string_buffer(cap + nmax + 16)
    r = host.dshh_append_fastx_records(path.encode(), out.ctypes.data, cap, C.byref(n), starts.ctypes.data, starts.size,
                                       names, len(names))
    assert r >= 0, r
    seq = out[: n.value].tobytes()
    st = starts[:r].astype(int).tolist() + [n.value]
    return [seq[st[i] : st[i + 1]] for i in range(r)], names.raw  # (names: '\n'-joined, NUL behind; a name may hold a NUL)


def check(host, path, data):
    want, _ = parse(data)
    cap = len(data) + 64
    r, s = stream(host, path, cap)
    assert r == len(want), (data[:200], r, len(want))
    assert s == b"N".join(q for _, q in want)
    assert runs(s) == all_runs(want)
    got, names = records(host, path, cap, data.count(b">") + data.count(b"@") + 1)
    packed = b"".join(n + b"\n" for n, _ in want)
    assert names[: len(packed) + 1] == packed + b"\0"
    assert got == [q for _, q in want]
    assert [runs(q) for q in got] == [runs(q) for _, q in want]


def _zstd_compress(data, level=3):
    try:
        z = C.CDLL("libzstd.so.1")
    except OSError:
        return None
    z.ZSTD_compressBound.restype = C.c_size_t
    z.ZSTD_compressBound.argtypes = [C.c_size_t]
    z.ZSTD_compress.restype = C.c_size_t
    z.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    cap = z.ZSTD_compressBound(len(data))
    dst = C.create_string_buffer(cap)
    n = z.ZSTD_compress(dst, cap, data, len(data), level)
    return dst.raw[:n]


@pytest.mark.parametrize("comp", ["plain", "gz", "zst"])
@pytest.mark.parametrize("i", range(len(KSEQ_CASES)))
def test_hand_cases(host, tmp_path, i, comp):
    data = KSEQ_CASES[i][0]
    path = tmp_path / "x.fa"
    if comp == "plain":
        path.write_bytes(data)
    elif comp == "gz":
        path = tmp_path / "x.fa.gz"
        path.write_bytes(gzip.compress(data))
    else:
        frame = _zstd_compress(data)
        if frame is None:
            pytest.skip("no libzstd.so.1 on this host")
        path = tmp_path / "x.fa.zst"
        path.write_bytes(frame)
    check(host, str(path), data)


def _genome(rng, L):
    g = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), L).tobytes())
    for _ in range(int(rng.integers(0, 4))):  # lowercase and N runs
        a = int(rng.integers(0, L))
        g[a : a + int(rng.integers(1, 40))] = bytes(g[a : a + 40]).lower() if rng.random() < 0.5 else b"N" * len(g[a : a + 40])
    return bytes(g[:L])


FUZZ_CASES = int(os.environ.get("DSH_HOST_FUZZ_CASES", "3000"))


def test_fuzz_against_kseq(host, tmp_path):
    """3 000 seeded texts, well-formed or damaged (tests/fastx_gen.py::damage: '\\r' and '\\r\\r\\n' anywhere, text before
    and between records, empty reads, cuts on a '+' line, quality of the wrong length, ...): the reader equals kseq"""
    path = str(tmp_path / "z.fx")
    for case in range(FUZZ_CASES):
        rng = np.random.default_rng(0x5EC0 + case)
        g = _genome(rng, int(rng.integers(1, 3000)))
        data, eol = random_text(rng, g)
        if rng.random() < 0.8:
            data = damage(rng, data, eol)
        with open(path, "wb") as f:
            f.write(data)
        try:
            check(host, path, data)
        except AssertionError as e:
            raise AssertionError("case %d: %r" % (case, data[:300])) from e


@pytest.mark.parametrize("what", ["crlf", "cr_cr_lf", "lone_cr", "header", "name", "plus", "qual_cr"])
@pytest.mark.parametrize("shift", [-2, -1, 0, 1])
def test_structure_across_the_read_block(host, tmp_path, what, shift):
    """a '\\r\\n', a '\\r\\r\\n', a lone '\\r', a header, a name, a '+' line, a quality line's '\\r\\r\\n' on the 1 MiB read
    block's edge: the thing's first byte at BLOCK - 2 ... BLOCK + 1"""
    rng = np.random.default_rng(11)
    line = lambda n: rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()
    at = BLOCK + shift
    if what in ("crlf", "cr_cr_lf", "lone_cr"):
        mid = {"crlf": b"\r\n", "cr_cr_lf": b"\r\r\n", "lone_cr": b"\r"}[what]
        data = b">a\n" + line(at - 3) + mid + line(50) + b"\r\n" + line(30) + b"\n"
        assert data[at : at + len(mid)] == mid
    elif what == "header":
        data = b">a\n" + line(at - 4) + b"\n>b x\n" + line(40) + b"\n"
        assert data[at : at + 1] == b">"
    elif what == "name":
        data = b">a\n" + line(at - 9) + b"\n>name_across_the_block\tcomment\n" + line(40) + b"\n"
    else:  # FASTQ records of 100 bases, then one whose '+' (or whose quality's '\\r\\r\\n') starts at `at`
        recs, n = [], 0
        while n < at - 1000:
            recs.append(b"@r\n" + line(100) + b"\n+\n" + b"I" * 100 + b"\n")
            n += len(recs[-1])
        data = b"".join(recs)
        plus = at if what == "plus" else at - 51
        data += b"@" + b"p" * (plus - len(data) - 53) + b"\n" + line(50) + b"\n"
        assert len(data) == plus
        data += b"+\n" + b"I" * 49 + b"\r\r\n@t\nAC\n+\nII\n"  # 49 + the '\\r' kseq keeps = 50
        assert data[at : at + 1] == (b"+" if what == "plus" else b"\r")
    path = tmp_path / "b.fa"
    path.write_bytes(data)
    check(host, str(path), data)


@pytest.mark.parametrize("d", range(-3, 3))
def test_crlf_at_every_offset_around_the_read_block(host, tmp_path, d):
    """the '\\r' of a CRLF on every byte from 3 before to 2 behind the read block's end: a FASTA sequence line, a FASTQ
    sequence line, a FASTQ quality line"""
    rng = np.random.default_rng(12)
    r = rng.choice(np.frombuffer(b"ACGT", np.uint8), BLOCK + 200).tobytes()
    at = BLOCK + d
    fa = b">a\n" + r[: at - 3] + b"\r\n" + r[:100] + b"\r\n"
    L = at - 4
    fq_seq = b"@q\r\n" + r[:L] + b"\r\n+\r\n" + b"I" * L + b"\r\n"
    h, L = at - 2008, 1000
    fq_qual = b"@" + b"x" * h + b"\r\n" + r[:L] + b"\r\n+\r\n" + b"I" * L + b"\r\n"
    for data, where in ((fa, 3 + at - 3), (fq_seq, 4 + at - 4), (fq_qual, h + 8 + 2 * L)):
        assert where == at and data[at : at + 2] == b"\r\n"
        path = tmp_path / "c.fa"
        path.write_bytes(data)
        check(host, str(path), data)
