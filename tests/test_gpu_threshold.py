"""GPU: the thresholded output (dsh_dist_threshold*, dsh_dist_rect_threshold) against the dense path it
is built on (bit for bit, no exclusions), across band sizes, against the CPU oracle (with the undecided pairs of
tests/thr_ref.py), at the edge of the caller's capacity, and at 100 000 sketches."""
import numpy as np
import pytest

import dashing_amd
import thr_ref
from dashing_amd import synth
from test_gpu_compare import close  # (the 1e-6 relative rule between GPU and oracle values)

pytestmark = pytest.mark.gpu

D = dashing_amd
RESULT_TYPES = (D.MASH_DIST, D.JI, D.SIZES, D.CONTAINMENT_INDEX, D.CONTAINMENT_DIST, D.SYMMETRIC_CONTAINMENT_INDEX)


def thresholds_for(dense, rt):
    """several thresholds per case: the exact ties, below and above every value, and values taken from the data"""
    ts = [0.0, 1.0, -1.0, 2.0]
    fin = dense[np.isfinite(dense)]
    if fin.size:
        ts += [float(fin.min()), float(fin.max()), float(np.nextafter(fin.max(), np.float32(np.inf))),
               float(np.nextafter(fin.min(), np.float32(-np.inf))), float(np.median(fin)), float(fin[fin.size // 3])]
    if rt == D.SIZES:
        ts.append(float(np.float32(3.0e6)))
    return ts


def check_tri(ctx, n, estim, rt, k, rb=0, re=None, ts=None):
    re = n if re is None else re
    dense = ctx.dist_rows(rb, re, estim=estim, result_type=rt, k=k)
    for t in (thresholds_for(dense, rt) if ts is None else ts):
        got = ctx.dist_threshold(t, rb, re, estim=estim, result_type=rt, k=k)
        want = thr_ref.tri(dense, n, rb, re, t, rt)
        assert thr_ref.same(got, want), (n, estim, rt, t, rb, re, got[0][-1], want[0][-1])
        cnt = ctx.dist_threshold_count(t, rb, re, estim=estim, result_type=rt, k=k)
        assert np.array_equal(cnt, want[0])
    return dense


@pytest.mark.parametrize("p,n", [(10, 1), (10, 2), (10, 127), (10, 128), (10, 129), (10, 300), (14, 130), (12, 97), (4, 33),
                                 (16, 140), (19, 131)])
@pytest.mark.parametrize("estim", [0, 1, 2])
def test_equal_to_dense_path(ctx, p, n, estim):
    """shapes of test_tri_vs_oracle: every estimator, six result types, ties at t = 1.0 (JI of duplicated sketches;
    Mash of an empty sketch: about half of the values in its row and column) and t = 0.0 (Mash of duplicates)"""
    regs = synth.synthetic_sketches(n, p, seed=0x1234 + p * 131 + n)
    if n > 3:
        regs[n // 2] = regs[0]
        regs[n - 1] = 0
    if n > 100:
        regs[1::4] = 0  # every fourth sketch empty: 44 % of all pairs have one, and sit exactly on Mash 1.0 / JI 0.0
        regs[3] = regs[2]
    ctx.set_sketches(regs)
    for rt in RESULT_TYPES:
        dense = check_tri(ctx, n, estim, rt, 31)
        if n > 100 and rt == D.MASH_DIST:
            assert 0.4 < float((dense == 1.0).mean()) < 0.99 and (dense == 0.0).any()
        if n > 3 and rt == D.JI:
            assert (dense == 1.0).any()


def test_row_sub_ranges_and_rectangle(ctx):
    n, p = 300, 10
    regs = synth.synthetic_sketches(n, p, seed=77)
    regs[7] = regs[8] = regs[9]
    regs[20] = 0
    ctx.set_sketches(regs)
    for rt in (D.JI, D.MASH_DIST, D.CONTAINMENT_INDEX):
        for rb, re in [(0, n), (1, 70), (70, 71), (71, 299), (n - 1, n), (n - 2, n), (5, 5), (9, 3), (250, 10 ** 6), (n, n)]:
            check_tri(ctx, n, 2, rt, 21, rb, re, ts=(0.03, 0.3, 1.0, 0.0, -1.0))
        for q0, q1, r0, r1 in [(0, n, 0, n), (3, 40, 100, 297), (7, 10, 5, 12), (50, 51, 0, n), (10, 10, 0, n), (0, 20, 33, 33),
                               (0, 5, 299, 300)]:
            dense = ctx.dist_rect(q0, q1, r0, r1, estim=2, result_type=rt, k=21)
            for t in (0.03, 0.3, 1.0, 0.0, -1.0, 2.0):
                got = ctx.dist_rect_threshold(t, q0, q1, r0, r1, estim=2, result_type=rt, k=21)
                assert thr_ref.same(got, thr_ref.rect(dense, r0, t, rt)), (rt, q0, q1, r0, r1, t)


def test_long_rows_cross_chunks(ctx):
    """rows longer than one chunk of the selection kernels (4096 values), starting at every alignment"""
    n, p = 9000, 8
    regs = synth.synthetic_sketches(n, p, seed=5)
    regs[4100] = regs[3]
    ctx.set_sketches(regs)
    check_tri(ctx, n, 2, D.JI, 31, 0, 9, ts=(0.05, 0.2, 1.0, -1.0))
    check_tri(ctx, n, 2, D.MASH_DIST, 31, 4890, 4911, ts=(0.05, 0.0, 2.0))
    dense = ctx.dist_rect(3, 8, 1, n, estim=2, result_type=D.JI, k=31)
    for t in (0.05, 1.0, -1.0):
        assert thr_ref.same(ctx.dist_rect_threshold(t, 3, 8, 1, n), thr_ref.rect(dense, 1, t, D.JI))


def test_band_independence(ctx):
    n, p = 10_000, 14
    regs = synth.survey_sketches(n, p, seed=0x5EED0000)[0]
    regs[5] = regs[6] = regs[7]
    regs[9000] = regs[123]
    ctx.set_sketches(regs)
    for rt, t in ((D.JI, 0.05), (D.MASH_DIST, 0.08), (D.JI, 1.0)):
        one = ctx.dist_threshold(t, result_type=rt, k=31)
        assert one[1].size > 0
        try:
            ctx.set_option("threshold_band_bytes", 48 << 20)  # the triangle is 200 MB: at least four bands
            many = ctx.dist_threshold(t, result_type=rt, k=31)
            sub1 = ctx.dist_threshold(t, 3000, 5000, result_type=rt, k=31)
            ctx.set_option("threshold_band_bytes", 12 << 20)  # bands of about 500 rows: below range_sort_min_rows
            sub2 = ctx.dist_threshold(t, 3000, 5000, result_type=rt, k=31)
        finally:
            ctx.set_option("threshold_band_bytes", 1 << 30)
        assert thr_ref.same(one, many)
        assert thr_ref.same(sub1, sub2)
        lo, hi = int(one[0][3000]), int(one[0][5000])
        assert np.array_equal(sub1[0], one[0][3000:5001] - one[0][3000])
        assert np.array_equal(sub1[1], one[1][lo:hi]) and np.array_equal(sub1[2].view(np.uint32), one[2][lo:hi].view(np.uint32))
        again = ctx.dist_threshold(t, result_type=rt, k=31)
        assert thr_ref.same(one, again)
    dense = ctx.dist_rows(result_type=D.JI, k=31)
    assert thr_ref.same(ctx.dist_threshold(0.05, result_type=D.JI, k=31), thr_ref.tri(dense, n, 0, n, 0.05, D.JI))


def compare_with_oracle(got, oracle_vals, n, rb, re, t, rt):
    """the rule of item 3: a pair outside the undecided band is a hit exactly when the oracle says so; common hits are
    close().  Returns the number of undecided pairs."""
    und = thr_ref.undecided(oracle_vals, t)
    assert und.sum() <= thr_ref.UNDECIDED_CAP * max(oracle_vals.size, 1), int(und.sum())
    lens = thr_ref.row_lengths(n, rb, re)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rp, col, val = got
    rows = np.repeat(np.arange(lens.size), np.diff(rp.astype(np.int64)))
    pos = starts[rows] + (col.astype(np.int64) - (rb + rows + 1))
    assert (np.diff(pos) > 0).all()  # rows ascending, columns ascending
    ghit = np.zeros(oracle_vals.size, bool)
    ghit[pos] = True
    ohit = thr_ref.passes(oracle_vals, t, rt)
    assert (ghit == ohit)[~und].all(), int(((ghit != ohit) & ~und).sum())
    both = ghit & ohit
    gv = np.zeros(oracle_vals.size, np.float32)
    gv[pos] = val
    close(gv[both], oracle_vals[both])
    return int(und.sum())


@pytest.mark.parametrize("case", range(len(thr_ref.oracle_cases())))
def test_against_oracle(ctx, oracle, case):
    name, make, rt, k, ts = thr_ref.oracle_cases()[case]
    regs = make()
    n = regs.shape[0]
    want = oracle.dist_tri(regs, 2, rt, k)
    ctx.set_sketches(regs)
    for t in ts:
        got = ctx.dist_threshold(t, estim=2, result_type=rt, k=k)
        und = compare_with_oracle(got, want, n, 0, n, t, rt)
        print("%s rt=%d t=%g: %d hits, %d undecided" % (name, rt, t, got[1].size, und))
        assert 0 < got[1].size < want.size


def test_capacity(ctx):
    import torch

    n, p = 700, 12
    regs = synth.related_sketches(n, p, seed=91)[0]
    ctx.set_sketches(regs)
    full = ctx.dist_threshold(0.03, estim=2, result_type=D.JI, k=31)
    hits = full[1].size
    assert hits > 100
    dev = torch.device("cuda:0")
    GUARD, CAN_U, CAN_F = 64, 0xDEADBEEF, -12345.5
    for cap, mis in ((hits, 0), (hits - 1, 0), (0, 0), (hits, 1), (hits - 1, 2), (0, 3)):
        # mis: row_ptr, col and val start that many items behind the tensor's (aligned) start, with canaries in front
        rp = torch.full((mis + n + 1,), -1, dtype=torch.int64, device=dev)
        col = torch.full((mis + cap + GUARD,), CAN_U - (1 << 32), dtype=torch.int32, device=dev)  # (bit pattern 0xDEADBEEF)
        val = torch.full((mis + cap + GUARD,), CAN_F, dtype=torch.float32, device=dev)
        rp_all, col_all, val_all = rp, col, val
        rp, col, val = rp[mis:], col[mis:], val[mis:]
        assert col.data_ptr() == col_all.data_ptr() + 4 * mis and rp.data_ptr() == rp_all.data_ptr() + 8 * mis
        torch.cuda.synchronize()
        if cap == hits:
            assert ctx.dist_threshold_device(rp.data_ptr(), col.data_ptr(), val.data_ptr(), cap, 0.03, estim=2, result_type=D.JI, k=31) == hits
        else:
            with pytest.raises(dashing_amd.DshError) as e:
                ctx.dist_threshold_device(rp.data_ptr(), col.data_ptr(), val.data_ptr(), cap, 0.03, estim=2, result_type=D.JI, k=31)
            assert e.value.code == dashing_amd.ERANGE == -34 and e.value.n_hits == hits
            assert str(hits) in str(e.value)
        assert np.array_equal(rp.cpu().numpy().view(np.uint64), full[0])
        c = col.cpu().numpy().view(np.uint32)
        v = val.cpu().numpy()
        assert np.array_equal(c[:cap], full[1][:cap]) and np.array_equal(v[:cap].view(np.uint32), full[2][:cap].view(np.uint32))
        assert (c[cap:] == CAN_U).all() and (v[cap:] == np.float32(CAN_F)).all()
        assert (rp_all[:mis] == -1).all() and (col_all[:mis] == CAN_U - (1 << 32)).all() and (val_all[:mis] == CAN_F).all()
        # counts only on the device: NULL col/val
        rp2 = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        assert ctx.dist_threshold_device(rp2.data_ptr(), 0, 0, 0, 0.03, estim=2, result_type=D.JI, k=31) == hits
        assert np.array_equal(rp2.cpu().numpy().view(np.uint64), full[0])
        dense = ctx.dist_rows(estim=2, result_type=D.JI, k=31)  # the context answers a plain call afterwards
        assert thr_ref.same(full, thr_ref.tri(dense, n, 0, n, 0.03, D.JI))


def _checksum(torch, x):
    """64-bit wrapping sum of position-weighted words"""
    x = x.to(torch.int64)
    w = torch.arange(1, x.numel() + 1, device=x.device, dtype=torch.int64)
    return int((x * (2 * w + 1)).sum().item())


def test_at_size_100k_p10(ctx):
    import torch

    from test_gpu_configs import derived_collection

    dev = torch.device("cuda:0")
    n, p = 100_000, 10
    regs_d = derived_collection(torch, dev, n, p, 4_000, seed=0x5EED1000)
    ctx.attach_device(regs_d.data_ptr(), n, p)
    try:
        span = dashing_amd.tri_span(n, 0, n)
        dense = torch.empty(span, dtype=torch.float32, device=dev)
        ctx.dist_rows_device(dense.data_ptr(), result_type=D.MASH_DIST, k=31)
        t = 0.02
        tt = torch.tensor(t, dtype=torch.float32, device=dev)
        parts = [torch.nonzero(dense[s : s + (1 << 30)] <= tt).flatten() + s for s in range(0, span, 1 << 30)]
        pos = torch.cat(parts)
        hits = pos.numel()
        print("100000 x p=10, Mash <= %g: %d hits of %d (%.4f %%)" % (t, hits, span, 100.0 * hits / span))
        assert 0 < hits < span // 100
        lens = torch.arange(n - 1, -1, -1, device=dev, dtype=torch.int64)
        starts = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
        row = torch.searchsorted(starts, pos, right=True) - 1
        want_col = (row + 1 + pos - starts[row]).to(torch.int64)
        want_val = dense[pos]
        want_rp = torch.searchsorted(pos, starts)  # hits before the start of every row; entry n = all
        rp = torch.empty(n + 1, dtype=torch.int64, device=dev)
        col = torch.empty(hits, dtype=torch.int32, device=dev)
        val = torch.empty(hits, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        got = ctx.dist_threshold_device(rp.data_ptr(), col.data_ptr(), val.data_ptr(), hits, t, result_type=D.MASH_DIST, k=31)
        assert got == hits
        colu = col.to(torch.int64) & 0xFFFFFFFF
        assert torch.equal(rp, want_rp)
        for r in (0, 1, 17, 3999, 4000, 50_000, 99_990, n - 2, n - 1):
            lo, hi = int(want_rp[r]), int(want_rp[r + 1])
            assert torch.equal(colu[lo:hi], want_col[lo:hi]) and torch.equal(val[lo:hi].view(torch.int32), want_val[lo:hi].view(torch.int32))
        assert _checksum(torch, rp) == _checksum(torch, want_rp)
        assert _checksum(torch, colu) == _checksum(torch, want_col)
        assert _checksum(torch, val.view(torch.int32)) == _checksum(torch, want_val.view(torch.int32))
    finally:
        ctx.alloc(2, 10)  # the shared context must not keep a pointer into a tensor that is about to go
