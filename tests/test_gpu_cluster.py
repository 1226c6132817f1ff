"""GPU: the threshold clusters (dsh_cluster_threshold*, dsh_cluster_pairs, dsh_cluster_csr).  labels[x] is
the smallest slot of x's connected component, which has ONE answer: every comparison here is an exact comparison of uint32
arrays with the numpy reference (tests/cluster_ref.py) -- on graphs handed in as edge lists, on the graph of the hits
Context.dist_threshold returns for the same context (the same float32 values: no tolerance), and on the graph of the CPU
oracle at thresholds chosen inside a gap of the oracle's values.  No test here tries to reach the step-bound give-up path
(tests/test_cluster_host.py does that on the CPU)."""
import numpy as np
import pytest

import cluster_ref
import dashing_amd
import guard
import thr_ref
from dashing_amd import synth

pytestmark = pytest.mark.gpu

D = dashing_amd
EINVAL, ESTATE = -22, -11


def check_pairs(ctx, n, lhs, rhs, what=""):
    want, wc = cluster_ref.labels(n, lhs, rhs)
    got, gc = ctx.cluster_pairs(n, lhs, rhs)
    assert got.dtype == np.uint32 and got.shape == (n,)
    assert np.array_equal(got, want) and gc == wc, what
    return want, wc


# ---- the edge-list form --------------------------------------------------------------------------------------------
def test_chain_of_100k_in_three_orders(ctx):
    """deep paths (descending order hooks every root under the next) and contended hooks (shuffled)"""
    n = 100_000
    a, b = cluster_ref.chain(n)
    perm = np.random.default_rng(7).permutation(a.size)
    for name, lhs, rhs in (("ascending", a, b), ("descending", b[::-1].copy(), a[::-1].copy()), ("shuffled", a[perm], b[perm])):
        got, nc = ctx.cluster_pairs(n, lhs, rhs)
        assert not got.any() and nc == 1, name
    # and cut in two: the label of the second half is its first node
    keep = a != n // 2
    got, nc = ctx.cluster_pairs(n, a[perm][keep[perm]], b[perm][keep[perm]])
    assert nc == 2 and not got[: n // 2 + 1].any() and (got[n // 2 + 1 :] == n // 2 + 1).all()


def test_star_cliques_and_degenerate_graphs(ctx):
    for hub in (0, 4999, 9999):
        check_pairs(ctx, 10_000, *cluster_ref.star(10_000, hub), what="star %d" % hub)
    l, r, (jl, jr) = cluster_ref.two_cliques(300)
    want, wc = check_pairs(ctx, 600, l, r, "cliques apart")
    assert wc == 2 and want[599] == 300
    for name, lhs, rhs in (("joined last", np.concatenate([l, jl]), np.concatenate([r, jr])),
                           ("joined first", np.concatenate([jl, l]), np.concatenate([jr, r]))):
        want, wc = check_pairs(ctx, 600, lhs, rhs, name)
        assert wc == 1
    e = np.zeros(0, np.uint32)
    ar = np.arange(1000, dtype=np.uint32)
    check_pairs(ctx, 1000, ar, ar, "self loops")
    want, wc = check_pairs(ctx, 1000, e, e, "no edges")
    assert wc == 1000 and np.array_equal(want, ar)
    check_pairs(ctx, 1, e, e, "one node")
    check_pairs(ctx, 1, np.zeros(3, np.uint32), np.zeros(3, np.uint32), "one node, self loops")
    got, nc = ctx.cluster_pairs(0, e, e)
    assert got.size == 0 and nc == 0
    lhs, rhs = cluster_ref.random_graph(5000, 2000, 9)
    want, _ = check_pairs(ctx, 5000, np.tile(lhs, 4), np.tile(rhs, 4), "every edge four times")
    assert np.array_equal(want, cluster_ref.labels(5000, lhs, rhs)[0])
    for name, n, lhs, rhs in cluster_ref.small_graphs():
        check_pairs(ctx, n, lhs, rhs, name)


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("m_of_n", [0.25, 0.5, 1.0, 4.0])
def test_random_graphs_around_percolation(ctx, m_of_n, seed):
    """n = 50 000, m / n in {1/4, 1/2, 1, 4}: from many small trees through the point where the giant component forms"""
    n = 50_000
    m = int(n * m_of_n)
    lhs, rhs = cluster_ref.random_graph(n, m, 1000 * seed + int(8 * m_of_n))
    want, wc = check_pairs(ctx, n, lhs, rhs)
    assert cluster_ref.is_labelling(want)
    # the CSR form of the same graph: rows = the smaller end, in row order
    lo, hi = np.minimum(lhs, rhs), np.maximum(lhs, rhs)
    order = np.argsort(lo, kind="stable")
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(lo, minlength=n))]).astype(np.uint64)
    got, gc = ctx.cluster_csr(n, row_ptr, hi[order])
    assert np.array_equal(got, want) and gc == wc
    # a row range of its own: rows [r0, n) alone, then the rest seeded with it
    r0 = n // 3
    h0 = int(row_ptr[r0])
    part, _ = ctx.cluster_csr(n, row_ptr[r0:], hi[order], row_begin=r0)
    assert np.array_equal(part, cluster_ref.labels(n, lo[order][h0:], hi[order][h0:])[0])
    both, bc = ctx.cluster_csr(n, row_ptr[: r0 + 1], hi[order], labels_in=part)
    assert np.array_equal(both, want) and bc == wc


def test_labels_in_chains_three_calls(ctx):
    n = 50_000
    lhs, rhs = cluster_ref.random_graph(n, n, 77)
    want, wc = check_pairs(ctx, n, lhs, rhs)
    cut = (0, n // 5, n // 2, n)
    lab = None
    for a, b in zip(cut[:-1], cut[1:]):
        lab, nc = ctx.cluster_pairs(n, lhs[a:b], rhs[a:b], labels_in=lab)
        assert np.array_equal(lab, cluster_ref.labels(n, lhs[:b], rhs[:b])[0])
    assert np.array_equal(lab, want) and nc == wc
    # a seed alone (no edges) returns the seed's components; it need not be in normal form
    again, nc = ctx.cluster_pairs(n, [], [], labels_in=want)
    assert np.array_equal(again, want) and nc == wc
    seed = np.arange(n, dtype=np.uint32)[::-1].copy()  # x with n - 1 - x
    got, nc = ctx.cluster_pairs(n, [], [], labels_in=seed)
    assert np.array_equal(got, np.minimum(np.arange(n), n - 1 - np.arange(n)).astype(np.uint32)) and nc == n // 2


def test_chunk_size_changes_nothing(ctx):
    n = 20_000
    lhs, rhs = cluster_ref.random_graph(n, 3000, 5)
    a, b = cluster_ref.chain(2000)
    lhs, rhs = np.concatenate([lhs, b[::-1]]), np.concatenate([rhs, a[::-1]])
    want, wc = check_pairs(ctx, n, lhs, rhs)
    lo, hi = np.minimum(lhs, rhs), np.maximum(lhs, rhs)
    order = np.argsort(lo, kind="stable")
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(lo, minlength=n))]).astype(np.uint64)
    try:
        for chunk in (1, 7, 4096):
            ctx.set_option("cluster_chunk", chunk)
            got, gc = ctx.cluster_pairs(n, lhs, rhs)
            assert np.array_equal(got, want) and gc == wc, chunk
            got, gc = ctx.cluster_csr(n, row_ptr, hi[order])
            assert np.array_equal(got, want) and gc == wc, chunk
    finally:
        ctx.set_option("cluster_chunk", 1 << 20)
    with pytest.raises(D.DshError):
        ctx.set_option("cluster_chunk", 0)


# ---- the threshold form against the hits of the same context ------------------------------------------------------
def quantile_thresholds(dense, rt, n):
    """thresholds out of the dense values: nothing passes, everything passes, and hit fractions of about 1/n (the graph
    near percolation: the informative case), 1 % and 50 %"""
    fin = np.sort(dense[np.isfinite(dense)])
    if not fin.size:
        return [0.5]
    sim = rt in thr_ref.SIMILARITY
    if sim:
        fin = fin[::-1]  # best first
    past = np.float32(np.inf) if sim else np.float32(-np.inf)
    ts = [float(np.nextafter(fin[0], past)), float(fin[-1])]
    ts += [float(fin[min(int(q * fin.size), fin.size - 1)]) for q in (1.0 / n, 0.01, 0.5)]
    return ts


def tri_shapes():
    seen, out = set(), []
    for name, make, rt, k, ts in thr_ref.oracle_cases():
        if name not in seen:
            seen.add(name)
            out.append((name, make, k))
    for n in (1, 2, 129):
        out.append(("synthetic%dp10" % n, (lambda n=n: synth.synthetic_sketches(n, 10, seed=0x77 + n)), 31))
    return out


@pytest.mark.parametrize("rt", [D.JI, D.MASH_DIST, D.CONTAINMENT_INDEX])
@pytest.mark.parametrize("shape", range(len(tri_shapes())))
def test_threshold_form_equals_the_components_of_the_hits(ctx, shape, rt):
    name, make, k = tri_shapes()[shape]
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    dense = ctx.dist_rows(estim=2, result_type=rt, k=k)
    ts = quantile_thresholds(dense, rt, n)
    for x, t in enumerate(ts + [float("nan")]):
        rp, col, val = ctx.dist_threshold(t, estim=2, result_type=rt, k=k)
        lhs, rhs = cluster_ref.csr_edges(rp, col)
        want, wc = cluster_ref.labels_fast(n, lhs, rhs)
        got, gc = ctx.cluster_threshold(t, estim=2, result_type=rt, k=k)
        print("%s rt=%d t=%.9g: %d hits of %d, %d clusters" % (name, rt, t, col.size, dense.size, wc))
        assert got.dtype == np.uint32 and np.array_equal(got, want) and gc == wc, (name, rt, t)
        if x == 0 or t != t:  # nothing passes; NaN: n singletons
            assert col.size == 0 and gc == n
        if x == 1 and n > 1 and np.isfinite(dense).all():
            assert col.size == dense.size and gc == 1
        # many bands, rows cut across bands: the same labels
        try:
            ctx.set_option("threshold_band_bytes", 64 << 10)
            many, mc = ctx.cluster_threshold(t, estim=2, result_type=rt, k=k)
        finally:
            ctx.set_option("threshold_band_bytes", 1 << 30)
        assert np.array_equal(many, want) and mc == wc
        # the CSR form over the hits: the same labels
        viacsr, cc = ctx.cluster_csr(n, rp, col)
        assert np.array_equal(viacsr, want) and cc == wc


def test_long_rows_cross_chunks(ctx):
    """rows longer than one chunk of the band kernel (4096 values), starting at every alignment"""
    n, p = 9000, 8
    regs = synth.synthetic_sketches(n, p, seed=5)
    regs[4100] = regs[3]
    regs[8999] = regs[3]
    ctx.set_sketches(regs)
    dense = ctx.dist_rows(estim=2, result_type=D.JI, k=31)
    for t in quantile_thresholds(dense, D.JI, n)[2:4] + [1.0]:
        rp, col, _ = ctx.dist_threshold(t, estim=2, result_type=D.JI, k=31)
        want, wc = cluster_ref.labels_fast(n, *cluster_ref.csr_edges(rp, col))
        got, gc = ctx.cluster_threshold(t, estim=2, result_type=D.JI, k=31)
        assert np.array_equal(got, want) and gc == wc, t
        assert got[4100] == got[3] == got[8999]  # the duplicates of sketch 3, a chunk and two chunks further on


# ---- against the CPU oracle ------------------------------------------------------------------------------------------
def gap_threshold(ov, frac, sim):
    """the midpoint of the widest gap among the 200 oracle values around the wanted quantile, and that gap"""
    fin = np.sort(ov[np.isfinite(ov)])
    if sim:
        fin = fin[::-1]
    kth = int(round(frac * fin.size))
    w = fin[max(kth - 100, 0) : max(kth - 100, 0) + 200]
    d = np.abs(np.diff(w))
    x = int(np.argmax(d))
    return float((w[x] + w[x + 1]) / 2), float(d[x])


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_against_oracle(ctx, oracle, case):
    """GPU and oracle values agree to 1e-6 relative, so a pair within that of t may fall either way and the graphs may
    differ.  The test therefore chooses t itself, inside a gap of the ORACLE's values: then both graphs are the same and
    the labels must be equal exactly.  Gaps found with the oracle alone, on the CPU (hit fraction 1/n, 1 %):
      synthetic300p10 JI        t = 0.617909402 gap 6.3e-2   t = 0.291205764  gap 1.3e-1
      synthetic300p10 MASH_DIST t = 0.0128808934 gap 3.0e-3  t = 0.0391090969 gap 1.7e-2
      related700p12   JI        t = 0.632687539 gap 8.3e-2   t = 0.0312421937 gap 3.5e-5
      related700p12   MASH_DIST t = 0.00828078762 gap 2.6e-3 t = 0.0915163197 gap 3.6e-5
    all above the 2e-6 asked for, none with an undecided pair."""
    name, make, rt, k, _ = thr_ref.oracle_cases()[case]
    assert name in ("synthetic300p10", "related700p12") and rt in (D.JI, D.MASH_DIST)
    regs = make()
    n = regs.shape[0]
    ov = np.asarray(oracle.dist_tri(regs, 2, rt, k), np.float64)
    ctx.set_sketches(regs)
    sim = rt in thr_ref.SIMILARITY
    i, j = np.triu_indices(n, 1)
    for frac in (1.0 / n, 0.01):
        t, gap = gap_threshold(ov, frac, sim)
        print("%s rt=%d fraction %.5f: t = %.9g, gap %.3g" % (name, rt, frac, t, gap))
        assert gap > 2e-6
        assert not thr_ref.undecided(ov, t).any()
        with np.errstate(invalid="ignore"):
            hit = (ov >= t) if sim else (ov <= t)
        want, wc = cluster_ref.labels_fast(n, i[hit], j[hit])
        assert 1 < wc < n
        got, gc = ctx.cluster_threshold(t, estim=2, result_type=rt, k=k)
        assert np.array_equal(got, want) and gc == wc


# ---- the device form writes n labels and nothing else ----------------------------------------------------------------
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_device_form_between_guard_bands(ctx, misalign):
    import torch

    n, p = 700, 12
    regs = synth.related_sketches(n, p, seed=91)[0]
    ctx.set_sketches(regs)
    for t in (0.03, 0.6, 2.0):
        want, wc = ctx.cluster_threshold(t, estim=2, result_type=D.JI, k=31)
        buf = guard.Guarded(n, np.uint32, front=4096, back=4096, misalign=misalign, device=torch.device("cuda:0"))
        nc = ctx.cluster_threshold_device(buf.ptr, t, estim=2, result_type=D.JI, k=31)
        buf.check("cluster_threshold_device t=%g" % t)
        assert buf.unwritten() == 0
        assert np.array_equal(buf.host(), want) and nc == wc
    assert wc == n  # (t = 2: nothing passes, and still every label is written)


# ---- the context afterwards ------------------------------------------------------------------------------------------
def test_dense_and_threshold_calls_around_a_cluster_call(ctx):
    n, p = 3000, 12
    regs = synth.survey_sketches(n, p, seed=0x5EED0000)[0]
    ctx.set_sketches(regs)
    for rt, t in ((D.JI, 0.03), (D.MASH_DIST, 0.1)):
        before = ctx.dist_rows(estim=2, result_type=rt, k=31)
        csr = ctx.dist_threshold(t, estim=2, result_type=rt, k=31)
        lab, nc = ctx.cluster_threshold(t, estim=2, result_type=rt, k=31)
        after = ctx.dist_rows(estim=2, result_type=rt, k=31)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        assert thr_ref.same(ctx.dist_threshold(t, estim=2, result_type=rt, k=31), csr)
        sub = ctx.dist_rows(100, 900, estim=2, result_type=rt, k=31)  # a row range, a graph call, the range again
        lab2, _ = ctx.cluster_pairs(n, *cluster_ref.csr_edges(csr[0], csr[1]))
        assert np.array_equal(lab2, lab)
        assert np.array_equal(sub.view(np.uint32), ctx.dist_rows(100, 900, estim=2, result_type=rt, k=31).view(np.uint32))
        again, nc2 = ctx.cluster_threshold(t, estim=2, result_type=rt, k=31)
        assert np.array_equal(again, lab) and nc2 == nc


# ---- error codes -----------------------------------------------------------------------------------------------------
def test_error_codes(ctx):
    u = lambda *a: np.array(a, np.uint32)

    def code(fn, *a, **kw):
        with pytest.raises(D.DshError) as e:
            fn(*a, **kw)
        return e.value.code

    assert code(ctx.cluster_pairs, 4, u(0, 4), u(1, 2)) == EINVAL
    assert code(ctx.cluster_pairs, 4, u(0, 1), u(1, 4)) == EINVAL
    assert code(ctx.cluster_pairs, 4, u(0), u(1), labels_in=u(0, 1, 2, 4)) == EINVAL
    import ctypes

    nc = ctypes.c_uint64()  # (straight at the C entry point: the binding would allocate 2^32 labels first)
    assert D.api.load_library().dsh_cluster_pairs(ctx._h, 1 << 32, None, None, 0, None, None, ctypes.byref(nc)) == EINVAL
    assert code(ctx.cluster_csr, 4, np.array([0, 1], np.uint64), u(4)) == EINVAL
    assert code(ctx.cluster_csr, 4, np.array([0, 2, 1], np.uint64), u(1, 2)) == EINVAL
    assert code(ctx.cluster_csr, 4, np.array([0, 1, 2], np.uint64), u(1, 2), row_begin=3) == EINVAL
    assert code(ctx.cluster_csr, 4, np.array([0, 1], np.uint64), u(1), labels_in=u(9, 0, 0, 0)) == EINVAL
    # after the refusals the context still answers
    got, nc = ctx.cluster_pairs(4, u(0), u(3))
    assert got.tolist() == [0, 1, 2, 0] and nc == 3
    got, nc = ctx.cluster_csr(4, np.array([0, 0], np.uint64), u())
    assert got.tolist() == [0, 1, 2, 3] and nc == 4
    # the threshold forms need sketches; the graph forms do not
    fresh = D.Context(0)
    try:
        assert code(fresh.cluster_threshold, 0.5) == ESTATE
        assert code(fresh.cluster_threshold_device, 0, 0.5) == ESTATE
        got, nc = fresh.cluster_pairs(5, u(4), u(2))
        assert got.tolist() == [0, 1, 2, 3, 2] and nc == 4
    finally:
        fresh.close()
