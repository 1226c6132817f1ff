"""The band rule of dsh_greedy_threshold* (plan::greedy_band_end, through dshh_greedy_bands of csrc/host/plan_capi.cpp):
dsh_dist_threshold's rule -- whole rows, at most band_bytes of float32 (one row at least) -- with one more cap on the rows of
a band, which is what bounds the LDS of k_greedy_diag."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_CAPS = (1, 7, 129, 4096, 8192)


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    lib.dshh_greedy_bands.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.dshh_greedy_bands.restype = C.c_int64
    return lib


def bands(host, n, band_bytes, row_cap):
    out = np.zeros(max(n, 1) + 1, np.uint64)
    nb = host.dshh_greedy_bands(n, band_bytes, row_cap, out.ctypes.data, out.size)
    assert nb >= 0
    return out[: nb + 1].astype(np.int64)


def check(host, n, band_bytes, row_cap):
    b = bands(host, n, band_bytes, row_cap)
    what = (n, band_bytes, row_cap)
    if n < 2:
        assert b.size == 1, what
        return 0
    # rows [0, n - 1) exactly once, in ascending order (the last band may take the empty row n - 1 along)
    assert b[0] == 0 and (np.diff(b) > 0).all() and n - 1 <= b[-1] <= n, what
    rows = np.diff(b)
    assert rows.max() <= min(row_cap, 1 << 20), what
    cum = np.concatenate([[0], np.cumsum(n - 1 - np.arange(n, dtype=np.int64))])  # values in front of row i
    span = cum[b[1:]] - cum[b[:-1]]
    floats = max(band_bytes // 4, 1)
    assert ((span <= floats) | (rows == 1)).all(), what
    # greedy: a band stops only where the next row would break a rule (or the triangle ends)
    more = b[1:-1]
    nxt = span[:-1] + (n - 1 - more)
    assert ((rows[:-1] == min(row_cap, 1 << 20)) | (nxt > floats)).all(), what
    return rows.size


def test_bands_cover_the_rows_once_within_both_caps(host):
    rng = np.random.default_rng(0x6EED)
    ns = [0, 1, 2, 3, 129, 4097, 8193, 50_000] + rng.integers(2, 50_001, 12).tolist()
    for n in ns:
        sizes = [4, 8, 1000, 64 << 10, 1 << 20, 1 << 30] + (4 * rng.integers(1, max(n, 2) * 40, 3)).tolist()
        for band_bytes in sizes:
            for cap in ROW_CAPS:
                check(host, int(n), int(band_bytes), cap)


def test_the_row_cap_alone_cuts_a_small_triangle(host):
    # 700 rows fit one band of 1 GiB: the cap decides
    assert bands(host, 700, 1 << 30, 8192).tolist() == [0, 700]
    assert bands(host, 700, 1 << 30, 129).tolist() == [0, 129, 258, 387, 516, 645, 700]
    assert check(host, 700, 1 << 30, 1) == 699
    assert check(host, 700, 1 << 30, 7) == 100
    # and the byte budget alone: 4 bytes = one value per band, so every row is a band of its own until the rows are empty
    assert check(host, 50, 4, 4096) == 49
