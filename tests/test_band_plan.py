"""The band rule every consumer of dense bands shares (plan::tri_band_end and plan::rect_band_rows, through
dshh_threshold_bands of csrc/host/plan_capi.cpp, which walks them as for_each_band of csrc/bands.h does), against a numpy
model written from the rule:
  triangle   a band of whole rows [b0, b1), b1 <= re: at most band_bytes / 4 values (one row at least) and at most
             min(max(row_cap, 1), 2^20) rows; as many rows as that allows
  rectangle  min(max((band_bytes / 4) / ncols, 1), 2^20) rows per band, the last band what is left."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ROWS = 1 << 20
NS = (0, 1, 2, 3, 129, 4097, 50_000)
BAND_BYTES = (4, 1000, 64 << 10, 1 << 30)
ROW_CAPS = (1, 7, 1 << 20)


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    lib.dshh_threshold_bands.argtypes = [C.c_uint64] * 6 + [C.c_void_p, C.c_uint64]
    lib.dshh_threshold_bands.restype = C.c_int64
    lib.dshh_greedy_bands.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.dshh_greedy_bands.restype = C.c_int64
    return lib


def bands(host, n, rb, re, ncols, band_bytes, row_cap):
    out = np.zeros(max(re - rb, 0) + 2, np.uint64)
    nb = host.dshh_threshold_bands(n, rb, re, ncols, band_bytes, row_cap, out.ctypes.data, out.size)
    assert nb >= 0
    return out[: nb + 1].astype(np.int64)


def row_ranges(n):
    return [(0, n), (3, n // 2), (n - 2, n), (n // 3, n // 3)]  # whole, inner, the last two rows, empty


def model_triangle(n, rb, re, floats, row_cap):
    """Boundaries of the bands of rows [rb, re) of the triangle of n sketches (row i holds n - 1 - i values)."""
    if rb >= re:
        return np.array([rb], np.int64)
    max_rows = min(max(row_cap, 1), MAX_ROWS)
    cum = np.concatenate([[0], np.cumsum(n - 1 - np.arange(n, dtype=np.int64))])  # values in front of row i
    b0 = np.arange(rb, re, dtype=np.int64)
    fit = np.searchsorted(cum, cum[b0] + floats, side="right") - 1  # the last boundary the budget reaches from b0
    end = np.minimum(np.minimum(np.maximum(fit, b0 + 1), b0 + max_rows), re).tolist()  # the end of a band that starts at b0
    out = [rb]
    while out[-1] < re:
        out.append(end[out[-1] - rb])
    return np.array(out, np.int64)


def check_triangle(host, n, rb, re, band_bytes, row_cap):
    what = (n, rb, re, band_bytes, row_cap)
    b = bands(host, n, rb, re, 0, band_bytes, row_cap)
    floats = max(band_bytes // 4, 1)
    if rb >= re:
        assert b.tolist() == [rb], what
        return b
    # the rows exactly once, in ascending order, nothing behind re
    assert b[0] == rb and b[-1] == re and (np.diff(b) > 0).all(), what
    rows = np.diff(b)
    max_rows = min(max(row_cap, 1), MAX_ROWS)
    cum = np.concatenate([[0], np.cumsum(n - 1 - np.arange(n, dtype=np.int64))])
    span = cum[b[1:]] - cum[b[:-1]]
    # within both caps, or a single row
    assert rows.max() <= max_rows, what
    assert ((span <= floats) | (rows == 1)).all(), what
    # a band ends only where the next row would break a cap (or the range ends)
    more = b[1:-1]
    assert ((rows[:-1] == max_rows) | (span[:-1] + (n - 1 - more) > floats)).all(), what
    assert b.tolist() == model_triangle(n, rb, re, floats, row_cap).tolist(), what
    return b


def test_triangle_bands_match_the_model(host):
    for n in NS:
        for rb, re in row_ranges(n):
            if rb < 0 or re > n:
                continue  # (n < 2: no "last two rows")
            for band_bytes in BAND_BYTES:
                for cap in ROW_CAPS:
                    check_triangle(host, n, rb, re, band_bytes, cap)


def test_row_end_beyond_n_is_cut_to_n(host):
    assert bands(host, 129, 100, 10_000, 0, 1000, 7).tolist() == bands(host, 129, 100, 129, 0, 1000, 7).tolist()


def test_greedy_bands_are_the_triangle_rule_up_to_row_n(host):
    """dshh_greedy_bands = tri_band_end(n, b0, n, floats, cap) from row 0 on, without a band of the empty last row alone."""
    for n in NS:
        for band_bytes in BAND_BYTES:
            for cap in ROW_CAPS:
                want = bands(host, n, 0, n, 0, band_bytes, cap).tolist()
                if len(want) > 1 and want[-2] == n - 1:
                    want.pop()  # [n - 1, n): no values, greedy.hip never asks for it
                out = np.zeros(n + 2, np.uint64)
                nb = host.dshh_greedy_bands(n, band_bytes, cap, out.ctypes.data, out.size)
                assert nb >= 0 and out[: nb + 1].tolist() == want, (n, band_bytes, cap)


def test_rectangle_bands_match_the_model(host):
    for ncols in (1, 5, 4097):
        for band_bytes in BAND_BYTES:
            per = min(max(max(band_bytes // 4, 1) // ncols, 1), MAX_ROWS)
            for rb, re in ((0, 50_000), (3, 2_000), (7, 8), (5, 5), (0, (1 << 20) + 3)):
                if (re - rb) // per > 200_000:
                    continue  # (a row a band over a million rows: the same arithmetic as over 50 000)
                want = list(range(rb, re, per)) + [re] if re > rb else [rb]
                got = bands(host, 0, rb, re, ncols, band_bytes, 1)  # (n and row_cap play no part)
                assert got.tolist() == want, (ncols, band_bytes, rb, re)
                if re > rb:
                    rows = np.diff(got)
                    assert rows.max() <= MAX_ROWS and ((rows * ncols <= max(band_bytes // 4, 1)) | (rows == 1)).all()
                    assert (rows[:-1] == per).all() and got[-1] == re


def test_the_bounds_must_fit(host):
    out = np.zeros(4, np.uint64)
    assert host.dshh_threshold_bands(50, 0, 50, 0, 4, 1, out.ctypes.data, out.size) == -1
