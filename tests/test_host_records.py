"""The host reader's records mode (dshh_append_fastx_records, sketch_by_seq / dist_by_seq): record starts and kseq names
equal the kseq port tests/kseq_ref.py, and the records back to back equal what dshh_append_fastx gives with its 'N'
separators taken out."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from kseq_ref import parse as kseq_parse  # (tests/kseq_ref.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    cp, vp, sz = C.c_char_p, C.c_void_p, C.c_size_t
    lib.dshh_append_fastx.restype = C.c_long
    lib.dshh_append_fastx.argtypes = [cp, vp, sz, C.POINTER(sz)]
    lib.dshh_append_fastx_records.restype = C.c_long
    lib.dshh_append_fastx_records.argtypes = [cp, vp, sz, C.POINTER(sz), vp, sz, vp, sz]
    return lib


def records(host, path, cap=1 << 20):
    out = np.zeros(cap, np.uint8)
    n = C.c_size_t(0)
    starts = np.zeros(4096, np.uint64)
    names = C.create_string_buffer(1 << 16)
    r = host.dshh_append_fastx_records(path.encode(), out.ctypes.data, cap, C.byref(n), starts.ctypes.data, starts.size,
                                       names, len(names))
    assert r >= 0, r
    nm = names.value.decode().split("\n")[:r]
    return out[: n.value].tobytes(), starts[:r].astype(int).tolist(), nm


def _zstd_compress(data, level=3):
    """a zstd frame made with the host's libzstd (the runtime library the reader binds); None if absent"""
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


def genome(host, path, cap=1 << 20):
    out = np.zeros(cap, np.uint8)
    n = C.c_size_t(0)
    assert host.dshh_append_fastx(path.encode(), out.ctypes.data, cap, C.byref(n)) >= 0
    return out[: n.value].tobytes()


def reference(text):
    """kseq's view (tests/kseq_ref.py, a port of klib's kseq_read): the records read before the first error, with their
    names (header up to the first white space) and sequences"""
    recs, _ = kseq_parse(text.encode("latin-1"))
    return [(n.decode("latin-1"), s.decode("latin-1")) for n, s in recs]


CASES = {
    "crlf.fa": ">r1 desc\r\nACGT\r\nGGCC\r\n>r2\r\nTTTT\r\n",
    "empty_lines.fa": ">a\n\nACGTACGT\n\n>b x\nAC\n\n\nGT\n>c\n>d\nNNNN\n",
    "bare_header.fa": ">\nACGT\n>\n\n>z\nCC\n",
    "tabs.fa": ">id1\tsome\tthing\nACGTTT\n>id2 \tx\nGG\n>id3\tq r\nA\n",
    "quals.fq": "@q1 x\nACGTA\n+\n@@+@@\n@q2\nGGT\n+q2\n+@+\n@q3\nACGTACGT\nAC\n+\n@@@@\n@@@@@@\n",
    "mixed_case.fa": ">m1\nacgtNNacgt\nACGT\n>m2 desc\nggg\n",
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("comp", ["plain", "gz", "zst"])
def test_records_equal_reference(host, tmp_path, name, comp):
    text = CASES[name]
    path = str(tmp_path / name)
    with open(path, "w", newline="") as f:
        f.write(text)
    if comp == "gz":
        with open(path, "rb") as f, gzip.open(path + ".gz", "wb") as g:
            g.write(f.read())
        path += ".gz"
    elif comp == "zst":
        with open(path, "rb") as f:
            frame = _zstd_compress(f.read())
        if frame is None:
            pytest.skip("no libzstd.so.1 on this host")
        with open(path + ".zst", "wb") as g:
            g.write(frame)
        path += ".zst"
    seq, starts, names = records(host, path)
    ref = reference(text)
    assert names == [n for n, _ in ref]
    want_starts, o = [], 0
    for _, s in ref:
        want_starts.append(o)
        o += len(s)
    assert starts == want_starts
    assert seq == "".join(s for _, s in ref).encode()
    # genome mode: the same records with one 'N' between them
    assert genome(host, path) == b"N".join(s.encode() for _, s in ref)


def test_records_append_behind_existing_bytes(host, tmp_path):
    path = str(tmp_path / "x.fa")
    with open(path, "w") as f:
        f.write(">a\nACGT\n>b\nGG\n")
    out = np.zeros(64, np.uint8)
    n = C.c_size_t(10)
    starts = np.zeros(8, np.uint64)
    names = C.create_string_buffer(64)
    assert host.dshh_append_fastx_records(path.encode(), out.ctypes.data, 64, C.byref(n), starts.ctypes.data, 8, names, 64) == 2
    assert n.value == 16 and starts[:2].tolist() == [10, 14] and out[10:16].tobytes() == b"ACGTGG"
    assert host.dshh_append_fastx_records(b"/nonexistent/file.fa", out.ctypes.data, 64, C.byref(n), starts.ctypes.data, 8,
                                          names, 64) == -1
