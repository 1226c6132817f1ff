"""GPU: the minimum spanning tree of the pair values (dsh_mst, dsh_mst_tri).  The result has ONE answer -- the
forest Kruskal's algorithm builds from the edges in the total order (value, i, j) -- so every comparison here is an exact
comparison of arrays with the reference models (tests/mst_ref.py): on matrices handed in (mst_tri), and on the values
Context.dist_rows returns for the same context (the same float32 values: no tolerance).  No test here tries to reach the
round-bound give-up path (tests/test_mst_host.py does that on the CPU)."""
import ctypes

import numpy as np
import pytest

import dashing_amd
import mst_ref as R
import thr_ref
from dashing_amd import synth

pytestmark = pytest.mark.gpu

D = dashing_amd
EINVAL, ESTATE = -22, -11
SMALL_BAND, BAND = 64 << 10, 1 << 30


def same(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32), w.view(np.uint32)), what


def both_bands(ctx, call):
    """the call at the default band size and with many bands, rows cut across bands: the same bytes"""
    one = call()
    try:
        ctx.set_option("threshold_band_bytes", SMALL_BAND)
        many = call()
    finally:
        ctx.set_option("threshold_band_bytes", BAND)
    same(many, one, "band size")
    return one


# ---- a caller's triangle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,tri", R.families(), ids=[f[0] for f in R.families()])
def test_mst_tri_equals_kruskal(ctx, name, n, tri):
    for desc in (0, 1):
        for cut in R.cutoffs(tri, desc):
            got = both_bands(ctx, lambda: ctx.mst_tri(tri, desc, cut, labels=True, n_nodes=n))
            same(got, R.kruskal(n, tri, desc, cut), (name, desc, cut))
            same(ctx.mst_tri(tri, desc, cut, n_nodes=n), got[:3], "without labels")
    same(ctx.mst_tri(tri, 1, labels=True, n_nodes=n), R.kruskal(n, tri, 1, -np.inf), "the default is no cutoff")
    same(ctx.mst_tri(tri, 0, labels=True, n_nodes=n), R.kruskal(n, tri, 0, np.inf), "the default is no cutoff")


def test_all_equal_values_give_the_star(ctx):
    lhs, rhs, val, lab = ctx.mst_tri(R.all_equal(50), 0, labels=True)
    assert lhs.tolist() == [0] * 49 and rhs.tolist() == list(range(1, 50)) and not lab.any()
    assert ctx.info("mst_rounds") == 1


@pytest.mark.parametrize("desc", [0, 1])
def test_the_ultrametric_matrix_takes_exactly_eight_rounds(ctx, desc):
    tri = R.ultrametric(256, desc)
    got = both_bands(ctx, lambda: ctx.mst_tri(tri, desc, labels=True))
    same(got, R.kruskal(256, tri, desc, R.no_cutoff(desc)), desc)
    assert ctx.info("mst_rounds") == 8


# ---- the resident sketches against the dense values of the same context ----------------------------------------------
def shapes():
    """those of tests/test_gpu_cluster.py::tri_shapes up to 700 sketches, and exact ties: 43 distinct rows three times each"""
    seen, out = set(), []
    for name, make, rt, k, ts in thr_ref.oracle_cases():
        if name not in seen and name in ("synthetic300p10", "related700p12"):
            seen.add(name)
            out.append((name, make, k))
    for n in (1, 2, 129):
        out.append(("synthetic%dp10" % n, (lambda n=n: synth.synthetic_sketches(n, 10, seed=0x77 + n)), 31))
    out.append(("triples129p10", lambda: np.tile(synth.synthetic_sketches(43, 10, seed=0x99), (3, 1)), 31))
    return out


def dense_cutoffs(dense, sim):
    """none, the 1 % and 50 % quantiles of the dense values (best first), one that nothing passes, NaN"""
    fin = np.sort(dense[np.isfinite(dense)])
    if sim:
        fin = fin[::-1]
    out = [None]
    if fin.size:
        out += [float(fin[min(int(q * fin.size), fin.size - 1)]) for q in (0.01, 0.5)]
        out.append(float(np.nextafter(fin[0], np.float32(np.inf if sim else -np.inf))))
    return out + [float("nan")]


@pytest.mark.parametrize("rt", [D.JI, D.MASH_DIST, D.CONTAINMENT_INDEX])
@pytest.mark.parametrize("shape", range(len(shapes())), ids=[s[0] for s in shapes()])
def test_mst_equals_kruskal_over_the_dense_values(ctx, shape, rt):
    name, make, k = shapes()[shape]
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    kw = dict(estim=2, result_type=rt, k=k)
    dense = ctx.dist_rows(**kw)
    sim = rt in thr_ref.SIMILARITY
    for x, cut in enumerate(dense_cutoffs(dense, sim)):
        got = both_bands(ctx, lambda: ctx.mst(cut, labels=True, **kw))
        want = R.kruskal(n, dense, sim, R.no_cutoff(sim) if cut is None else cut)
        print("%s rt=%d cutoff=%s: %d edges, %d rounds" % (name, rt, cut, got[0].size, ctx.info("mst_rounds")))
        same(got, want, (name, rt, cut))
        lhs, rhs, val, lab = got
        t = float(R.no_cutoff(sim)) if cut is None else cut
        assert np.array_equal(lab, ctx.cluster_threshold(t, **kw)[0])
        at = np.array([D.tri_index(n, int(i), int(j)) for i, j in zip(lhs, rhs)], np.int64)
        assert np.array_equal(val.view(np.uint32), (dense[at] + np.float32(0)).view(np.uint32))  # bit for bit, up to the sign of zero
        if x >= len(dense_cutoffs(dense, sim)) - 2:  # nothing passes; NaN
            assert lhs.size == 0 and np.array_equal(lab, np.arange(n, dtype=np.uint32))
    if name.startswith("triples") and rt == D.JI:
        lhs, rhs, val = ctx.mst(**kw)
        assert np.all(val[:86] == val[0]) and val[86] < val[0] and lhs[:86].tolist() == sorted(list(range(43)) * 2)  # (x, x + 43), (x, x + 86) first


@pytest.mark.parametrize("rt", [D.JI, D.MASH_DIST])
def test_every_prefix_gives_the_clusters_at_its_threshold(ctx, rt):
    regs = synth.related_sketches(700, 12, seed=91)[0]
    n = regs.shape[0]
    ctx.set_sketches(regs)
    kw = dict(estim=2, result_type=rt, k=31)
    sim = rt in thr_ref.SIMILARITY
    lhs, rhs, val = ctx.mst(**kw)
    assert lhs.size == n - 1  # (every value is finite: a spanning tree)
    for q in (0, lhs.size // 100, lhs.size // 10, lhs.size // 2, lhs.size - 1):
        t = float(val[q])
        passes = (val >= np.float32(t)) if sim else (val <= np.float32(t))
        m = int(passes.sum())
        assert passes[:m].all() and not passes[m:].any() and m > q  # a prefix
        got, gc = ctx.cluster_pairs(n, lhs[:m], rhs[:m])
        want, wc = ctx.cluster_threshold(t, **kw)
        assert np.array_equal(got, want) and gc == wc == n - m, (rt, q, t)


def test_long_rows_cross_chunks(ctx):
    """rows longer than one chunk of the band kernel (4096 values), starting at every alignment; the duplicates of sketch 3
    lie a chunk and two chunks further on"""
    n, p = 9000, 8
    regs = synth.synthetic_sketches(n, p, seed=5)
    regs[4100] = regs[3]
    regs[8999] = regs[3]
    ctx.set_sketches(regs)
    kw = dict(estim=2, result_type=D.JI, k=31)
    dense = ctx.dist_rows(**kw)
    got = ctx.mst(labels=True, **kw)
    print("n = %d: %d edges, %d rounds" % (n, got[0].size, ctx.info("mst_rounds")))
    same(got, R.prim(n, dense, 1, -np.inf), "long rows")
    first = list(zip(got[0][:2].tolist(), got[1][:2].tolist()))
    assert first == [(3, 4100), (3, 8999)] and got[2][0] == got[2][1]


# ---- the context afterwards ------------------------------------------------------------------------------------------
def test_dense_calls_around_an_mst_call(ctx):
    regs = synth.related_sketches(700, 12, seed=91)[0]
    ctx.set_sketches(regs)
    for rt in (D.JI, D.MASH_DIST):
        kw = dict(estim=2, result_type=rt, k=31)
        before = ctx.dist_rows(**kw)
        got = ctx.mst(labels=True, **kw)
        after = ctx.dist_rows(**kw)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        sim = rt in thr_ref.SIMILARITY
        same(got, R.kruskal(700, before, sim, R.no_cutoff(sim)), rt)
    other = synth.synthetic_sketches(129, 10, seed=0x1234)
    ctx.set_sketches(other)
    kw = dict(estim=2, result_type=D.JI, k=31)
    got = ctx.mst(labels=True, **kw)
    same(got, R.kruskal(129, ctx.dist_rows(**kw), 1, -np.inf), "after set_sketches")
    same(ctx.mst_tri(R.ties(40, 3), 0, labels=True), R.kruskal(40, R.ties(40, 3), 0, np.inf), "a triangle after sketches")
    same(ctx.mst(labels=True, **kw), got, "and the sketches again")


# ---- error codes -----------------------------------------------------------------------------------------------------
def test_error_codes(ctx):
    lib = D.api.load_library()
    ne = ctypes.c_uint64()
    buf = np.zeros(8, np.uint32)
    val = np.zeros(8, np.float32)
    tri = np.zeros(6, np.float32)
    p, v, t = buf.ctypes.data, val.ctypes.data, tri.ctypes.data
    ctx.set_sketches(synth.synthetic_sketches(4, 10, seed=1))
    assert lib.dsh_mst(ctx._h, 2, 1, 31, 0.5, None, p, v, ctypes.byref(ne), None) == EINVAL
    assert lib.dsh_mst(ctx._h, 2, 1, 31, 0.5, p, None, v, ctypes.byref(ne), None) == EINVAL
    assert lib.dsh_mst(ctx._h, 2, 1, 31, 0.5, p, p, None, ctypes.byref(ne), None) == EINVAL
    assert lib.dsh_mst(ctx._h, 2, 1, 31, 0.5, p, p, v, None, None) == EINVAL
    assert lib.dsh_mst_tri(ctx._h, 4, None, 0, 0.5, p, p, v, ctypes.byref(ne), None) == EINVAL
    assert lib.dsh_mst_tri(ctx._h, 4, t, 0, 0.5, None, p, v, ctypes.byref(ne), None) == EINVAL
    assert lib.dsh_mst_tri(ctx._h, 1 << 32, t, 0, 0.5, p, p, v, ctypes.byref(ne), None) == EINVAL
    # n == 0 and n == 1 succeed with 0 edges, whatever the pointers
    assert lib.dsh_mst_tri(ctx._h, 0, None, 0, 0.5, None, None, None, ctypes.byref(ne), None) == 0 and ne.value == 0
    assert lib.dsh_mst_tri(ctx._h, 1, None, 0, 0.5, None, None, None, ctypes.byref(ne), p) == 0 and ne.value == 0 and buf[0] == 0
    # after the refusals the context still answers
    lhs, rhs, val3, lab = ctx.mst(labels=True)
    assert lhs.size == 3 and not lab.any()
    fresh = D.Context(0)
    try:
        with pytest.raises(D.DshError) as e:
            fresh.mst()
        assert e.value.code == ESTATE
        same(fresh.mst_tri(R.tie_free(9, 1), 0, labels=True), R.kruskal(9, R.tie_free(9, 1), 0, np.inf), "no sketches needed")
    finally:
        fresh.close()
