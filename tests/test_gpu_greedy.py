"""GPU: the greedy representatives (dsh_greedy_threshold*).  The result has ONE answer -- the
lexicographically first maximal independent set of the hit graph in slot order, every other slot labelled with its
smallest representative -- so every comparison here is an exact comparison of uint32 arrays with the sequential reference
(tests/greedy_ref.py): over the hits Context.dist_threshold returns for the same context (the same float32 values: no
tolerance), and over the graph of the CPU oracle at thresholds chosen inside a gap of the oracle's values.  The feature
has no give-up path, and no test here tries to provoke a device fault."""
import numpy as np
import pytest

import dashing_amd
import greedy_ref
import guard
import thr_ref
from dashing_amd import synth
from test_gpu_cluster import gap_threshold, quantile_thresholds, tri_shapes

pytestmark = pytest.mark.gpu

D = dashing_amd
EINVAL, ESTATE = -22, -11
BAND_BYTES, BAND_ROWS = 1 << 30, 4096  # the defaults, restored after every change


def restore(ctx):
    ctx.set_option("threshold_band_bytes", BAND_BYTES)
    ctx.set_option("greedy_band_rows", BAND_ROWS)


def reference(ctx, n, t, rt, k):
    rp, col, _ = ctx.dist_threshold(t, estim=2, result_type=rt, k=k)
    return greedy_ref.labels(n, rp, col) + (col.size,)


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
    dense = ctx.dist_rows(estim=2, result_type=rt, k=k)
    ts = quantile_thresholds(dense, rt, n)
    try:
        for x, t in enumerate(ts + [float("nan")]):
            want = reference(ctx, n, t, rt, k)
            nhits = want[2]
            got = ctx.greedy_threshold(t, estim=2, result_type=rt, k=k)
            print("%s rt=%d t=%.9g: %d hits of %d, %d representatives" % (name, rt, t, nhits, dense.size, want[1]))
            assert_labels(got, want, (name, rt, t))
            if x == 0 or t != t:  # nothing passes; NaN: every slot represents itself
                assert nhits == 0 and np.array_equal(got[0], np.arange(n, dtype=np.uint32)) and got[1] == n
            if x == 1 and n > 1 and np.isfinite(dense).all():  # everything passes: slot 0 covers all
                assert nhits == dense.size and not got[0].any() and got[1] == 1
            # many bands, rows cut across bands, diagonal blocks of one row: the same labels
            ctx.set_option("threshold_band_bytes", 64 << 10)
            for cap in (1, 7, 129):
                ctx.set_option("greedy_band_rows", cap)
                assert_labels(ctx.greedy_threshold(t, estim=2, result_type=rt, k=k), want, (name, rt, t, cap))
            restore(ctx)
    finally:
        restore(ctx)


def test_representatives_are_not_components(ctx):
    """related700p12 JI at the 1 % threshold: single linkage chains (82 components on the CPU oracle), the greedy pass does
    not (198 representatives); every greedy cluster lies inside one component"""
    name, make, rt, k, _ = thr_ref.oracle_cases()[2]
    assert name == "related700p12" and rt == D.JI
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    t = 0.0312421937  # inside a gap of 3.5e-5 of the oracle's values (test_against_oracle): 1 % of the pairs pass
    lab, nr = ctx.greedy_threshold(t, estim=2, result_type=rt, k=k)
    comp, nc = ctx.cluster_threshold(t, estim=2, result_type=rt, k=k)
    print("t = %.9g: %d representatives, %d components, %d labels differ" % (t, nr, nc, int((lab != comp).sum())))
    assert nr > nc
    assert np.array_equal(comp[lab], comp)


def test_long_rows_cross_chunks(ctx):
    """rows longer than one chunk of the band kernel (4096 values), starting at every alignment; duplicates of sketch 3 a
    chunk and two chunks further on.  With greedy_band_rows = 8192 the first band holds 8192 rows and a thread of
    k_greedy_diag owns eight band columns (t, t + 1024, ...): the duplicates at 4100 and 7777 are then settled inside the
    band, in the fifth and the eighth column of their threads"""
    n, p = 9000, 8
    regs = synth.synthetic_sketches(n, p, seed=5)
    regs[4100] = regs[3]
    regs[7777] = regs[3]
    regs[8999] = regs[3]
    ctx.set_sketches(regs)
    dense = ctx.dist_rows(estim=2, result_type=D.JI, k=31)
    try:
        for t in quantile_thresholds(dense, D.JI, n)[2:4] + [1.0]:
            want = reference(ctx, n, t, D.JI, 31)
            got = ctx.greedy_threshold(t, estim=2, result_type=D.JI, k=31)
            print("t=%.9g: %d hits, %d representatives" % (t, want[2], want[1]))
            assert_labels(got, want, t)
            if t == 1.0:
                assert got[0][3] == 3 and got[0][4100] == 3 and got[0][8999] == 3
            ctx.set_option("greedy_band_rows", 129)
            assert_labels(ctx.greedy_threshold(t, estim=2, result_type=D.JI, k=31), want, (t, 129))
            ctx.set_option("greedy_band_rows", 8192)
            wide = ctx.greedy_threshold(t, estim=2, result_type=D.JI, k=31)
            assert_labels(wide, want, (t, 8192))
            if t == 1.0:
                assert wide[0][3] == 3 and wide[0][4100] == 3 and wide[0][7777] == 3 and wide[0][8999] == 3
                assert got[0][7777] == 3
            restore(ctx)
    finally:
        restore(ctx)


def test_prefix_property(ctx):
    """the labels of the first m slots are those of a call on the first m sketches alone"""
    name, make, rt, k, _ = thr_ref.oracle_cases()[6]
    assert name == "survey3000p12" and rt == D.JI
    regs = make()
    n, m = regs.shape[0], 1000
    ctx.set_sketches(regs)
    dense = ctx.dist_rows(estim=2, result_type=rt, k=k)
    t = quantile_thresholds(dense, rt, n)[3]
    whole, nr = ctx.greedy_threshold(t, estim=2, result_type=rt, k=k)
    assert 1 < nr < n
    ctx.set_sketches(regs[:m])
    first, _ = ctx.greedy_threshold(t, estim=2, result_type=rt, k=k)
    assert first.shape == (m,) and np.array_equal(first, whole[:m])
    assert (first != np.arange(m)).any()  # (some of them are covered: the comparison says something)


# ---- against the CPU oracle ------------------------------------------------------------------------------------------
# (case of thr_ref.oracle_cases(), hit fraction or None for 1 / n, representatives): found with the oracle alone
ORACLE = [(0, None, 209), (0, 0.01, 150), (0, 0.1, 38), (1, None, 209), (1, 0.01, 150), (1, 0.1, 37),
          (2, None, 490), (2, 0.01, 198), (3, None, 490), (3, 0.01, 193)]


@pytest.mark.parametrize("case,frac,reps", ORACLE)
def test_against_oracle(ctx, oracle, case, frac, reps):
    """GPU and oracle values agree to 1e-6 relative, so a pair within that of t may fall either way.  The test chooses t
    inside a gap of the ORACLE's values (as tests/test_gpu_cluster.py does): then both graphs are the same and the labels
    must be equal exactly.  Gaps found with the oracle alone, on the CPU (hit fraction 1/n, 1 %):
      synthetic300p10 JI        t = 0.617909402 gap 6.3e-2   t = 0.291205764  gap 1.3e-1   209 / 150 representatives
      synthetic300p10 MASH_DIST t = 0.0128808934 gap 3.0e-3  t = 0.0391090969 gap 1.7e-2   209 / 150
      related700p12   JI        t = 0.632687539 gap 8.3e-2   t = 0.0312421937 gap 3.5e-5   490 / 198
      related700p12   MASH_DIST t = 0.00828078762 gap 2.6e-3 t = 0.0915163197 gap 3.6e-5   490 / 193
    and synthetic300p10 at 10 %: JI t = 0.0236767204 gap 1.3e-5, 38; MASH_DIST t = 0.146508582 gap 2.6e-5, 37.
    (related700p12 JI at 10 % has a gap of 1.7e-6, below the 2e-6 asked for: not used.)"""
    name, make, rt, k, _ = thr_ref.oracle_cases()[case]
    assert name in ("synthetic300p10", "related700p12") and rt in (D.JI, D.MASH_DIST)
    regs = make()
    n = regs.shape[0]
    ov = np.asarray(oracle.dist_tri(regs, 2, rt, k), np.float64)
    ctx.set_sketches(regs)
    sim = rt in thr_ref.SIMILARITY
    t, gap = gap_threshold(ov, 1.0 / n if frac is None else frac, sim)
    print("%s rt=%d fraction %s: t = %.9g, gap %.3g" % (name, rt, frac, t, gap))
    assert gap > 2e-6
    assert not thr_ref.undecided(ov, t).any()
    with np.errstate(invalid="ignore"):
        hit = (ov >= t) if sim else (ov <= t)
    h = np.zeros((n, n), bool)
    h[np.triu_indices(n, 1)] = hit
    want, wr = greedy_ref.labels_from_definition(n, h)
    assert wr == reps
    got, gr = ctx.greedy_threshold(t, estim=2, result_type=rt, k=k)
    assert np.array_equal(got, want) and gr == wr


# ---- the device form writes n labels and nothing else ----------------------------------------------------------------
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_device_form_between_guard_bands(ctx, misalign):
    import torch

    n, p = 700, 12
    regs = synth.related_sketches(n, p, seed=91)[0]
    ctx.set_sketches(regs)
    for t in (0.03, 0.6, 2.0):
        want, wr = ctx.greedy_threshold(t, estim=2, result_type=D.JI, k=31)
        buf = guard.Guarded(n, np.uint32, front=4096, back=4096, misalign=misalign, device=torch.device("cuda:0"))
        nr = ctx.greedy_threshold_device(buf.ptr, t, estim=2, result_type=D.JI, k=31)
        buf.check("greedy_threshold_device t=%g" % t)
        assert buf.unwritten() == 0
        assert np.array_equal(buf.host(), want) and nr == wr
    assert wr == n  # (t = 2: nothing passes, and still every label is written)


# ---- the context afterwards ------------------------------------------------------------------------------------------
def test_dense_and_threshold_calls_around_a_greedy_call(ctx):
    n, p = 3000, 12
    regs = synth.survey_sketches(n, p, seed=0x5EED0000)[0]
    ctx.set_sketches(regs)
    for rt, t in ((D.JI, 0.03), (D.MASH_DIST, 0.1)):
        sub = ctx.dist_rows(100, 900, estim=2, result_type=rt, k=31)
        before = ctx.dist_rows(estim=2, result_type=rt, k=31)
        csr = ctx.dist_threshold(t, estim=2, result_type=rt, k=31)
        lab, nr = ctx.greedy_threshold(t, estim=2, result_type=rt, k=31)
        after = ctx.dist_rows(estim=2, result_type=rt, k=31)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        assert thr_ref.same(ctx.dist_threshold(t, estim=2, result_type=rt, k=31), csr)
        assert_labels((lab, nr), greedy_ref.labels(n, csr[0], csr[1]), (rt, t))
        again, nr2 = ctx.greedy_threshold(t, estim=2, result_type=rt, k=31)
        assert np.array_equal(again, lab) and nr2 == nr
        assert np.array_equal(sub.view(np.uint32), ctx.dist_rows(100, 900, estim=2, result_type=rt, k=31).view(np.uint32))


# ---- error codes -----------------------------------------------------------------------------------------------------
def test_error_codes(ctx):
    def code(fn, *a, **kw):
        with pytest.raises(D.DshError) as e:
            fn(*a, **kw)
        return e.value.code

    fresh = D.Context(0)
    try:
        assert code(fresh.greedy_threshold, 0.5) == ESTATE
        assert code(fresh.greedy_threshold_device, 0, 0.5) == ESTATE
    finally:
        fresh.close()
    regs = synth.synthetic_sketches(129, 10, seed=0x77 + 129)
    ctx.set_sketches(regs)
    try:
        assert code(ctx.set_option, "greedy_band_rows", 0) == EINVAL
        assert code(ctx.set_option, "greedy_band_rows", 8193) == EINVAL
        ctx.set_option("greedy_band_rows", 8192)
        ctx.set_option("greedy_band_rows", 1)
    finally:
        restore(ctx)
    import ctypes

    nr = ctypes.c_uint64()  # a NULL output with n > 0, straight at the C entry points
    lib = D.api.load_library()
    assert lib.dsh_greedy_threshold(ctx._h, 2, 1, 31, 0.5, None, ctypes.byref(nr)) == EINVAL
    assert lib.dsh_greedy_threshold_device(ctx._h, 2, 1, 31, 0.5, None, ctypes.byref(nr)) == EINVAL
    # after the refusals the context still answers
    lab, n_reps = ctx.greedy_threshold(2.0)
    assert np.array_equal(lab, np.arange(129, dtype=np.uint32)) and n_reps == 129
