"""GPU: the five consumers of dense bands (csrc/bands.h on the host, csrc/thr_walk.h on the device) give the same bytes
however the bands fall, at the smallest shapes where the shared walk can go wrong:
  n = 4200  row 0 has 4199 values: two chunks, the second of 103 values; the rows start at every alignment mod 4
  n = 131   every row is shorter than one float4 step of a wave (256 values): every load takes the edge path
Each with one band (1 GiB), bands of 64 KiB and bands of 4 bytes (every row its own band).  The one-band hits are pinned to
numpy.nonzero on the dense values; what each call computes is pinned to its reference model by the tests of its own file."""
import time

import numpy as np
import pytest

import dashing_amd
from dashing_amd import synth

pytestmark = pytest.mark.gpu

D = dashing_amd
BAND_BYTES, BAND_ROWS = 1 << 30, 4096  # the defaults, restored afterwards
KW = dict(estim=2, result_type=D.JI, k=31)


def outputs(ctx, n, t, seed):
    """every output of every consumer as bytes, by name"""
    out = {}

    def put(name, arrays, count=None):
        out[name] = tuple(np.ascontiguousarray(a).tobytes() for a in arrays) + (count,)

    put("threshold [0, n)", ctx.dist_threshold(t, **KW))
    put("threshold [3, n / 2)", ctx.dist_threshold(t, 3, n // 2, **KW))
    put("rect [0, 40) x [40, n)", ctx.dist_rect_threshold(t, 0, 40, 40, n, **KW))
    lab, nc = ctx.cluster_threshold(t, **KW)
    put("cluster", [lab], nc)
    for rows in (4096, 7):
        ctx.set_option("greedy_band_rows", rows)
        g, nr = ctx.greedy_threshold(t, **KW)
        put("greedy, %d rows" % rows, [g], nr)
        for mode in ("first", "best"):
            e, ne = ctx.greedy_extend(t, n // 2, seed, mode, **KW)
            put("greedy_extend %s, %d rows" % (mode, rows), [e], ne)
    ctx.set_option("greedy_band_rows", BAND_ROWS)
    st = ctx.group_stats(lab, route="dense", **KW)  # (stats_route = 0 for the call)
    put("group_stats", [st.medoid, st.cnt, st.sum, st.worst])
    return out


@pytest.mark.parametrize("n", [4200, 131])
def test_no_output_depends_on_how_the_bands_fall(ctx, n):
    regs = synth.synthetic_sketches(n, 10, seed=0xBA2D + n)
    try:
        ctx.set_sketches(regs)
        dense = ctx.dist_rows(**KW)
        # a threshold that between 1 % and 20 % of the pairs pass (JI: v >= t): the walk is neither empty nor saturated
        t = np.float32(np.quantile(dense, 0.95))
        share = float((dense >= t).mean())
        print("n=%d t=%.9g: %.2f %% of %d pairs pass" % (n, t, 100 * share, dense.size))
        assert 0.01 <= share <= 0.20
        # the seed of the extension: the greedy labels of the first half alone
        ctx.set_sketches(regs[: n // 2])
        seed, _ = ctx.greedy_threshold(float(t), **KW)
        ctx.set_sketches(regs)
        t0 = time.time()
        one = outputs(ctx, n, float(t), seed)
        print("one band: %.2f s" % (time.time() - t0))
        # the one-band hits are the dense values that pass, in row-major order
        rp, col, val = ctx.dist_threshold(float(t), **KW)
        idx = np.nonzero(dense >= t)[0]
        first = np.concatenate([[0], np.cumsum(n - 1 - np.arange(n, dtype=np.int64))])  # dense index of (i, i + 1)
        row = np.searchsorted(first, idx, side="right") - 1
        assert np.array_equal(col, (idx - first[row] + row + 1).astype(np.uint32))
        assert val.tobytes() == dense[idx].tobytes()
        assert np.array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.uint64))
        for band_bytes in (64 << 10, 4):
            ctx.set_option("threshold_band_bytes", band_bytes)
            t0 = time.time()
            got = outputs(ctx, n, float(t), seed)
            print("bands of %d bytes: %.2f s" % (band_bytes, time.time() - t0))
            assert got.keys() == one.keys()
            for name in one:
                assert got[name] == one[name], (n, band_bytes, name)
    finally:
        ctx.set_option("threshold_band_bytes", BAND_BYTES)
        ctx.set_option("greedy_band_rows", BAND_ROWS)
        ctx.set_option("stats_route", -1)
