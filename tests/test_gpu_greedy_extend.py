"""GPU: dsh_greedy_extend*  -- the greedy representatives continued behind a labelling of the first slots,
covered slots given to the first or to the best representative.  The result has ONE answer, so every comparison here is an
exact comparison of uint32 arrays with the sequential reference (tests/greedy_extend_ref.py) over the hits AND VALUES that
Context.dist_threshold returns for the same context (the same float32: no tolerance anywhere).  No test here tries to
provoke a device fault."""
import ctypes

import numpy as np
import pytest

import dashing_amd
import greedy_extend_ref as X
import guard
import thr_ref
from dashing_amd import synth
from test_gpu_cluster import quantile_thresholds, tri_shapes

pytestmark = pytest.mark.gpu

D = dashing_amd
EINVAL, ESTATE = -22, -11
BAND_BYTES, BAND_ROWS = 1 << 30, 4096  # the defaults, restored after every change
MODES = (("first", X.FIRST), ("best", X.BEST))
KW = dict(estim=2)


def restore(ctx):
    ctx.set_option("threshold_band_bytes", BAND_BYTES)
    ctx.set_option("greedy_band_rows", BAND_ROWS)


def first_news(n):
    return sorted({min(m, n) for m in (0, 1, 77, 128, n - 1, n) if m >= 0})


def arbitrary_labelling(m, which):
    """valid, and no full call's prefix: every old slot its own representative / only slot 0 one"""
    return np.arange(m, dtype=np.uint32) if which == 0 else np.zeros(m, np.uint32)


def assert_labels(got, want, what):
    lab, nr = got
    assert lab.dtype == np.uint32 and lab.shape == want[0].shape, what
    assert np.array_equal(lab, want[0]) and nr == want[1], what


# ---- against the hits of the same context ----------------------------------------------------------------------------
@pytest.mark.parametrize("rt", [D.JI, D.MASH_DIST, D.CONTAINMENT_INDEX])
@pytest.mark.parametrize("shape", range(len(tri_shapes())))
def test_equals_the_sequential_pass_over_the_hits(ctx, shape, rt):
    name, make, k = tri_shapes()[shape]
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    sim = rt in thr_ref.SIMILARITY
    dense = ctx.dist_rows(estim=2, result_type=rt, k=k)
    ts = quantile_thresholds(dense, rt, n)
    ms = first_news(n)
    caps = (1, 7, 129)
    turn = 0
    try:
        for x, t in enumerate(ts + [float("nan")]):
            rp, col, val = ctx.dist_threshold(t, estim=2, result_type=rt, k=k)
            for mname, mode in MODES:
                full = X.labels_fast(n, rp, col, val, 0, None, mode, sim)
                cases = []
                for m in ms:
                    cases.append((m, full[0][:m] if m else None, "prefix"))
                    if m:
                        cases.append((m, arbitrary_labelling(m, (m + x) % 2), "arbitrary"))
                for m, li, kind in cases:
                    want = full if kind == "prefix" else X.labels_fast(n, rp, col, val, m, li, mode, sim)
                    got = ctx.greedy_extend(t, m, li, mname, result_type=rt, k=k, **KW)
                    assert_labels(got, want, (name, rt, t, mname, m, kind))
                    if t != t:  # NaN: every new slot represents itself, the old ones stay
                        assert np.array_equal(got[0][m:], np.arange(m, n, dtype=np.uint32))
                print("%s rt=%d t=%.9g %s: %d hits of %d, %d representatives" % (name, rt, t, mname, col.size, dense.size, full[1]))
                # many bands, rows cut across bands, diagonal blocks of one row: the same labels.  Small collections take
                # every cap with every case; the largest takes the caps and the cases in turn
                ctx.set_option("threshold_band_bytes", 64 << 10)
                for cap in caps if n <= 700 else (caps[turn % 3],):
                    ctx.set_option("greedy_band_rows", cap)
                    for q, (m, li, kind) in enumerate(cases):
                        if n > 700 and q != turn % len(cases):
                            continue
                        want = full if kind == "prefix" else X.labels_fast(n, rp, col, val, m, li, mode, sim)
                        assert_labels(ctx.greedy_extend(t, m, li, mname, result_type=rt, k=k, **KW), want, (name, rt, t, mname, m, kind, cap))
                turn += 1
                restore(ctx)
    finally:
        restore(ctx)


# ---- equivalences ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", range(len(tri_shapes())))
def test_first_from_scratch_is_greedy_threshold(ctx, shape):
    name, make, k = tri_shapes()[shape]
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    for rt in (D.JI, D.MASH_DIST):
        dense = ctx.dist_rows(estim=2, result_type=rt, k=k)
        for t in quantile_thresholds(dense, rt, n) + [float("nan")]:
            want, wr = ctx.greedy_threshold(t, estim=2, result_type=rt, k=k)
            got, gr = ctx.greedy_extend(t, 0, None, "first", estim=2, result_type=rt, k=k)
            assert got.tobytes() == want.tobytes() and gr == wr, (name, rt, t)


def test_extending_the_prefix_of_a_full_call_gives_the_full_call(ctx):
    name, make, rt, k, _ = thr_ref.oracle_cases()[6]
    assert name == "survey3000p12" and rt == D.JI
    regs = make()
    n, m = regs.shape[0], 1000
    ctx.set_sketches(regs)
    dense = ctx.dist_rows(estim=2, result_type=rt, k=k)
    informative = 0  # thresholds at which some new slots are covered and some are representatives
    for t in quantile_thresholds(dense, rt, n)[2:5]:
        for mname, _ in MODES:
            full, nr = ctx.greedy_extend(t, 0, None, mname, estim=2, result_type=rt, k=k)
            ext, er = ctx.greedy_extend(t, m, full[:m], mname, estim=2, result_type=rt, k=k)
            covered = int((full[m:] != np.arange(m, n)).sum())
            print("t=%.9g %s: %d representatives, %d covered new slots" % (t, mname, nr, covered))
            assert np.array_equal(ext, full) and er == nr, (t, mname)
            informative += 0 < covered < n - m
    assert informative >= 2


# ---- BEST differs from FIRST -----------------------------------------------------------------------------------------
def test_best_differs_from_first_on_related700(ctx):
    """related700p12, JI, t = 0.0312421937 -- inside a gap of 3.5e-5 of the oracle's values (test_gpu_cluster's
    test_against_oracle): 2 393 hits, 198 representatives, and on the CPU oracle 24 of the 502 covered slots get another
    label under BEST.  A test that cannot tell the modes apart fails here."""
    name, make, rt, k, _ = thr_ref.oracle_cases()[2]
    assert name == "related700p12" and rt == D.JI
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    t = 0.0312421937
    first, fr = ctx.greedy_extend(t, 0, None, "first", estim=2, result_type=rt, k=k)
    best, br = ctx.greedy_extend(t, 0, None, "best", estim=2, result_type=rt, k=k)
    ndiff = int((first != best).sum())
    print("t = %.9g: %d representatives, %d labels differ between FIRST and BEST" % (t, fr, ndiff))
    x = np.arange(n)
    assert np.array_equal(first == x, best == x) and fr == br == 198
    assert ndiff >= 1
    # every covered slot passes against its label, and no other representative before it has a strictly better value
    rp, col, val = ctx.dist_threshold(t, estim=2, result_type=rt, k=k)
    dv = X.dense_of_csr(n, rp, col, val, -1.0)
    X.check_consequences(n, dv, t, 0, None, best, X.BEST, True, "best")
    X.check_consequences(n, dv, t, 0, None, first, X.FIRST, True, "first")


# ---- the tie rule ----------------------------------------------------------------------------------------------------
def tie_sketches(p=10, seed=0x71E):
    """slots [c, a, b, x]: a is non-zero only in the first half of the registers, b is a rolled by half (the same histogram,
    a disjoint support), x = max(a, b); c holds 3/16 of the registers of a and of b.  The estimator is a function of
    histograms, so v(a, x) and v(b, x) are the same float; c hits x with a worse value and hits neither a nor b."""
    rng = np.random.default_rng(seed)
    R = 1 << p
    a = np.zeros(R, np.uint8)
    a[: R // 2] = np.minimum(rng.geometric(0.5, R // 2) + 2, 64 - p + 1)
    b = np.roll(a, R // 2)
    x = np.maximum(a, b)
    c = np.zeros(R, np.uint8)
    q = 3 * R // 16
    c[:q] = a[:q]
    c[R // 2 : R // 2 + q] = b[R // 2 : R // 2 + q]
    return np.stack([c, a, b, x])


@pytest.mark.parametrize("rt,t", [(D.JI, 0.03), (D.MASH_DIST, 0.08)])
def test_ties_go_to_the_smaller_slot(ctx, oracle, rt, t):
    regs = tie_sketches()
    sim = rt in thr_ref.SIMILARITY
    # on the CPU, with the oracle: pairs in triangle order (c,a) (c,b) (c,x) (a,b) (a,x) (b,x)
    ov = np.asarray(oracle.dist_tri(regs, 2, rt, 31), np.float32)
    hit = (ov >= np.float32(t)) if sim else (ov <= np.float32(t))
    print("oracle values", ov.tolist())
    assert ov[4].view(np.uint32) == ov[5].view(np.uint32)  # v(a, x) and v(b, x) are bit-equal
    assert hit.tolist() == [False, False, True, False, True, True]  # c hits x only; a and b do not hit each other
    assert (ov[2] < ov[4]) if sim else (ov[2] > ov[4])  # c's value is the worse one
    # and the device's own values say the same
    ctx.set_sketches(regs)
    rp, col, val = ctx.dist_threshold(t, estim=2, result_type=rt, k=31)
    assert rp.tolist() == [0, 1, 2, 3, 3] and col.tolist() == [3, 3, 3] and val[1].view(np.uint32) == val[2].view(np.uint32)
    try:
        for m in (0, 1, 2, 3):  # x is reached by the triangle's rows, or by the rectangle of the old rows
            li = np.arange(m, dtype=np.uint32) if m else None
            for cap in (BAND_ROWS, 1):
                ctx.set_option("greedy_band_rows", cap)
                best, nr = ctx.greedy_extend(t, m, li, "best", estim=2, result_type=rt, k=31)
                assert best.tolist() == [0, 1, 2, 1] and nr == 3, (m, cap)  # a: not b (the tie), not c (that is FIRST)
                first, nr = ctx.greedy_extend(t, m, li, "first", estim=2, result_type=rt, k=31)
                assert first.tolist() == [0, 1, 2, 0] and nr == 3, (m, cap)
    finally:
        restore(ctx)


# ---- rectangle rows that cross chunks at every alignment -------------------------------------------------------------
def test_rectangle_rows_cross_chunks_at_every_alignment(ctx):
    """the sketches of test_long_rows_cross_chunks; first_new = 300 .. 303, so the rectangle's rows hold 8700 .. 8697 values:
    every residue mod 4, and three 4096-value chunks.  Duplicates of slot 3 sit a chunk and two chunks further on."""
    n, p = 9000, 8
    regs = synth.synthetic_sketches(n, p, seed=5)
    regs[4100] = regs[3]
    regs[7777] = regs[3]
    regs[8999] = regs[3]
    ctx.set_sketches(regs)
    dense = ctx.dist_rows(estim=2, result_type=D.JI, k=31)
    for t in [quantile_thresholds(dense, D.JI, n)[3], 1.0]:
        rp, col, val = ctx.dist_threshold(t, estim=2, result_type=D.JI, k=31)
        for mname, mode in MODES:
            full = X.labels_fast(n, rp, col, val, 0, None, mode, True)
            for m in (300, 301, 302, 303):
                assert (n - m) % 4 == (300 - m) % 4
                got = ctx.greedy_extend(t, m, full[0][:m], mname, estim=2, result_type=D.JI, k=31)
                assert_labels(got, full, (t, mname, m, "prefix"))
                li = arbitrary_labelling(m, 0)
                got = ctx.greedy_extend(t, m, li, mname, estim=2, result_type=D.JI, k=31)
                assert_labels(got, X.labels_fast(n, rp, col, val, m, li, mode, True), (t, mname, m, "arbitrary"))
                if t == 1.0:
                    assert got[0][3] == 3 and got[0][4100] == 3 and got[0][7777] == 3 and got[0][8999] == 3


# ---- the device form writes n labels and nothing else ----------------------------------------------------------------
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_device_form_between_guard_bands(ctx, misalign):
    import torch

    n, p, m = 700, 12, 77
    regs = synth.related_sketches(n, p, seed=91)[0]
    ctx.set_sketches(regs)
    for t in (0.03, 0.6, 2.0):
        for mname, _ in MODES:
            full, _ = ctx.greedy_extend(t, 0, None, mname, estim=2, result_type=D.JI, k=31)
            for first_new, li in ((0, None), (m, full[:m]), (n, full)):
                want, wr = ctx.greedy_extend(t, first_new, li, mname, estim=2, result_type=D.JI, k=31)
                buf = guard.Guarded(n, np.uint32, front=4096, back=4096, misalign=misalign, device=torch.device("cuda:0"))
                nr = ctx.greedy_extend_device(buf.ptr, t, first_new, li, mname, estim=2, result_type=D.JI, k=31)
                buf.check("greedy_extend_device t=%g %s m=%d" % (t, mname, first_new))
                assert buf.unwritten() == 0
                assert np.array_equal(buf.host(), want) and nr == wr
                assert np.array_equal(want, full)


# ---- the context afterwards ------------------------------------------------------------------------------------------
def test_dense_and_threshold_calls_around_an_extend_call(ctx):
    n, p, m = 3000, 12, 1000
    regs = synth.survey_sketches(n, p, seed=0x5EED0000)[0]
    ctx.set_sketches(regs)
    for rt, t in ((D.JI, 0.03), (D.MASH_DIST, 0.1)):
        sim = rt in thr_ref.SIMILARITY
        sub = ctx.dist_rows(100, 900, estim=2, result_type=rt, k=31)
        before = ctx.dist_rows(estim=2, result_type=rt, k=31)
        rect = ctx.dist_rect(0, m, m, n, estim=2, result_type=rt, k=31)
        csr = ctx.dist_threshold(t, estim=2, result_type=rt, k=31)
        for mname, mode in MODES:
            li = arbitrary_labelling(m, 0)
            lab, nr = ctx.greedy_extend(t, m, li, mname, estim=2, result_type=rt, k=31)
            after = ctx.dist_rows(estim=2, result_type=rt, k=31)
            assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
            assert np.array_equal(rect.view(np.uint32), ctx.dist_rect(0, m, m, n, estim=2, result_type=rt, k=31).view(np.uint32))
            assert thr_ref.same(ctx.dist_threshold(t, estim=2, result_type=rt, k=31), csr)
            assert_labels((lab, nr), X.labels_fast(n, *csr, m, li, mode, sim), (rt, t, mname))
            again, nr2 = ctx.greedy_extend(t, m, li, mname, estim=2, result_type=rt, k=31)
            assert np.array_equal(again, lab) and nr2 == nr
            assert np.array_equal(sub.view(np.uint32), ctx.dist_rows(100, 900, estim=2, result_type=rt, k=31).view(np.uint32))


# ---- error codes -----------------------------------------------------------------------------------------------------
def test_error_codes(ctx):
    def err(fn, *a, **kw):
        with pytest.raises(D.DshError) as e:
            fn(*a, **kw)
        return e.value

    fresh = D.Context(0)
    try:
        assert err(fresh.greedy_extend, 0.5).code == ESTATE
        assert err(fresh.greedy_extend_device, 0, 0.5).code == ESTATE
    finally:
        fresh.close()
    n = 129
    regs = synth.synthetic_sketches(n, 10, seed=0x77 + n)
    ctx.set_sketches(regs)
    lib = D.api.load_library()
    nr = ctypes.c_uint64()
    out = np.zeros(n, np.uint32)
    ok = np.zeros(n + 1, np.uint32)

    def raw(mode, first_new, li, outp, device=False):
        fn = lib.dsh_greedy_extend_device if device else lib.dsh_greedy_extend
        return fn(ctx._h, 2, 1, 31, 0.5, mode, first_new, None if li is None else li.ctypes.data, outp, ctypes.byref(nr))

    for device in (False, True):
        outp = None if device else out.ctypes.data  # (every refusal comes before the output is looked at, or is about it)
        if device:
            import torch

            dbuf = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            outp = dbuf.data_ptr()
        assert raw(0, n + 1, ok, outp, device) == EINVAL  # first_new > n
        assert raw(2, 0, None, outp, device) == EINVAL and raw(-1, 0, None, outp, device) == EINVAL  # assign_mode
        assert raw(0, 5, None, outp, device) == EINVAL  # labels_in NULL with first_new > 0
        assert raw(0, 0, ok, outp, device) == EINVAL  # ... and NULL if and only if
        assert raw(1, 0, None, None, device) == EINVAL  # a NULL output with n > 0
    # labels_in violations name the slot
    bad = np.zeros(50, np.uint32)
    bad[17] = 18  # behind its slot
    e = err(ctx.greedy_extend, 0.5, 50, bad)
    assert e.code == EINVAL and "labels_in[17]" in str(e)
    bad = np.zeros(50, np.uint32)
    bad[31] = 10  # 10 is covered by 0, so it is no representative, and 31 points at it
    e = err(ctx.greedy_extend, 0.5, 50, bad, "best")
    assert e.code == EINVAL and "labels_in[31]" in str(e)
    import torch

    e = err(ctx.greedy_extend_device, torch.zeros(n, dtype=torch.int32, device="cuda:0").data_ptr(), 0.5, 50, bad)
    assert e.code == EINVAL and "labels_in[31]" in str(e)
    # after the refusals the context still answers; n == first_new copies and counts
    li = np.zeros(n, np.uint32)
    li[100:] = 100
    lab, n_reps = ctx.greedy_extend(2.0, n, li, "best")
    assert np.array_equal(lab, li) and n_reps == 2
    lab, n_reps = ctx.greedy_extend(2.0)
    assert np.array_equal(lab, np.arange(n, dtype=np.uint32)) and n_reps == n


def test_empty_and_tiny_collections(ctx):
    for n in (1, 2):
        ctx.set_sketches(synth.synthetic_sketches(n, 10, seed=0x77 + n))
        for mname, _ in MODES:
            for m in range(n + 1):
                li = np.arange(m, dtype=np.uint32) if m else None
                lab, nr = ctx.greedy_extend(2.0 if mname == "first" else float("nan"), m, li, mname, result_type=D.JI)
                assert lab.tolist() == list(range(n)) and nr == n
