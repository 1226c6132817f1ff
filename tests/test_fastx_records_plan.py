"""CPU: the host arithmetic between the decoder's record index and the records planner (csrc/sketch_plan.h:
fastx_tail_records, fastx_line_start, fastx_record_offsets) and the name rule (host.h: fastx_name_len), through
libdashing_host.so against a few lines of Python and, for the tail rule, against kseq itself (tests/kseq_ref.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from kseq_ref import parse as kseq_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACE = b" \t\n\v\f\r"


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    lib.dshh_fastx_tail_records.restype = C.c_int
    lib.dshh_fastx_tail_records.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.dshh_fastx_line_start.restype = C.c_uint64
    lib.dshh_fastx_line_start.argtypes = [C.c_char_p, C.c_uint64]
    lib.dshh_fastx_record_offsets.restype = None
    lib.dshh_fastx_record_offsets.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.dshh_fastx_name_len.restype = C.c_size_t
    lib.dshh_fastx_name_len.argtypes = [C.c_char_p, C.c_size_t]
    return lib


def test_name_ends_at_the_first_isspace_byte_or_the_end(host):
    for text in [b"", b"abc", b"abc def", b" x", b"a\tb", b"a\rb", b"a\nb", b"a\vb", b"a\fb", b"a\x00b c", b"\xffz\x1f\x0e\x08 q", b"a" * 300]:
        want = next((i for i, c in enumerate(text) if c in SPACE), len(text))
        assert host.dshh_fastx_name_len(text, len(text)) == want, text
        assert host.dshh_fastx_name_len(text, min(2, len(text))) == min(want, 2, len(text))


def test_line_start(host):
    text = b"@a b\nACGT\n+\nIIII\n@second\nAC"
    for pos in range(len(text)):
        assert host.dshh_fastx_line_start(text, pos) == text.rfind(b"\n", 0, pos) + 1, pos


def strict_fastq(data):
    """the decoder's view of an accepted FASTQ text: (markers, the index of the line it ends on)"""
    nl = data.count(b"\n")
    lines = data.split(b"\n")
    return sum(1 for i in range(0, nl, 4)), nl & 3, lines


GOOD = b"@r1 x\nACGT\n+\nIIII\n@r2\nAC\n+\nII\n"


@pytest.mark.parametrize("data", [
    GOOD, GOOD[:-1], GOOD + b"@s\n", GOOD + b"@s", GOOD + b"@", GOOD + b"@\r", GOOD + b"@s tail text", b"@only a header", b"@x", b"@",
    b"@r\n", b"@r\nAC", b"@r\nAC\n", b"@r\n\n+", b"@r\n\n+\n", b"@r\n\n+\r", b"@r\n\n+\n\n", GOOD + b"@e\n\n+", GOOD + b"@e\n\n+\n"])
def test_tail_rule_gives_kseqs_count(host, data):
    """markers + the tail rule = the records kseq returns, for four-line texts the decoder accepts (equal sequence and
    quality lengths per record)"""
    markers, end_line, _ = strict_fastq(data)
    got = markers + host.dshh_fastx_tail_records(data, len(data), 1, end_line)
    assert got == len(kseq_parse(data)[0]), data
    assert host.dshh_fastx_tail_records(data, len(data), 0, end_line) == 0  # (FASTA: the decoder leaves the last byte out itself)
    assert host.dshh_fastx_tail_records(data, 0, 1, 0) == 0


def test_record_offsets(host):
    dpos = np.array([32, 40, 41, 100], np.uint64)
    for markers, n, end in [(4, 4, 130), (4, 3, 130), (3, 4, 130), (0, 1, 64), (0, 0, 64), (1, 1, 33)]:
        off = np.zeros(n + 1, np.uint64)
        host.dshh_fastx_record_offsets(dpos.ctypes.data, markers, n, end, off.ctypes.data)
        want = [int(dpos[r]) if r < markers else end for r in range(n)] + [end]
        assert off.tolist() == want
        assert (np.diff(off.astype(np.int64)) >= 0).all()
