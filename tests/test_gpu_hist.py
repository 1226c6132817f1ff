"""GPU: dsh_dist_histogram*  -- the values of a triangle or rectangle call counted over caller-given edges,
optionally split by a labelling.  The result has ONE answer, so every comparison is exact array equality with the numpy
reference (tests/hist_ref.py) fed with Context.dist_rows / Context.dist_rect of the SAME context: the same float32 values,
no tolerance, no excluded share."""
import ctypes

import numpy as np
import pytest

import dashing_amd
import guard
import hist_ref as H
from dashing_amd import synth
from test_gpu_cluster import quantile_thresholds, tri_shapes
from test_gpu_group_stats import random_groups

pytestmark = pytest.mark.gpu

D = dashing_amd
F = np.float32
EINVAL, ESTATE = -22, -11
MEASURES = [D.JI, D.MASH_DIST, D.CONTAINMENT_INDEX]


def shapes():
    return tri_shapes() + [("synthetic4200p10", (lambda: synth.synthetic_sketches(4200, 10, seed=0x4200)), 31)]


def data_edges(dense):
    """edges taken FROM the data: the minimum, the maximum and quantiles of the finite values (ties on an edge test the
    closed side)"""
    fin = np.unique(dense[np.isfinite(dense)])
    if not fin.size:
        return np.array([0.25], F)
    return np.unique(fin[np.round(np.linspace(0, fin.size - 1, 13)).astype(np.int64)]).astype(F)


def many_edges(dense):
    """4096 edges: a sorted unique sample of data values with their nextafter neighbours on both sides, filled up with
    the float32 values that follow the largest one"""
    fin = np.unique(dense[np.isfinite(dense)])
    if not fin.size:
        fin = np.array([0.5], F)
    s = fin[np.round(np.linspace(0, fin.size - 1, min(fin.size, 1300))).astype(np.int64)]
    e = np.unique(np.concatenate([s, np.nextafter(s, F(np.inf)), np.nextafter(s, F(-np.inf))]).astype(F))
    e = e[np.isfinite(e)]  # (at most 3 x 1300 of them)
    base = e[-1] if e[-1] > 0 else F(0)  # (from a value >= +0.0 on, the next floats are the next bit patterns)
    fill = (np.array([base], F).view(np.uint32)[0] + np.arange(1, D.HIST_MAX_EDGES - e.size + 1, dtype=np.uint32)).view(F)
    e = np.concatenate([e, fill])
    assert e.size == D.HIST_MAX_EDGES and (np.diff(e) > 0).all() and np.isfinite(e).all()
    return e.astype(F)


def edge_sets(dense):
    return {
        "one edge": np.array([0.5], F),
        "100 uniform bins": np.linspace(0, 1, 101).astype(F),
        "from the data": data_edges(dense),
        "4096 edges": many_edges(dense),
        "-inf 0 inf": np.array([-np.inf, 0.0, np.inf], F),
        "all below": np.array([-3.0, -2.0], F),
        "all above": np.array([5.0, 6.0, 7.0], F),
    }


def labellings(ctx, dense, rt, k, n):
    ar = np.arange(n, dtype=np.uint32)
    ts = quantile_thresholds(dense, rt, n)
    return {
        "singletons": ar,
        "one group": np.full(n, 0xFFFFFFF0, np.uint32),  # (any values are legal: only equality matters)
        "random groups": random_groups(np.random.default_rng(n + rt), n, max(n // 16, 2)),
        "clusters": ctx.cluster_threshold(float(F(ts[min(4, len(ts) - 1)])), estim=2, result_type=rt, k=k)[0],
    }


def checked(got, planes, ne, pairs, what):
    assert got.dtype == np.uint64 and got.shape == (planes, ne + 2), what
    assert int(got.sum()) == pairs, what
    return got


@pytest.mark.parametrize("rt", MEASURES)
@pytest.mark.parametrize("shape", range(len(shapes())))
def test_triangle_equals_the_reference(ctx, shape, rt):
    name, make, k = shapes()[shape]
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    kw = dict(estim=2, result_type=rt, k=k)
    dense = ctx.dist_rows(**kw)
    pairs = n * (n - 1) // 2
    assert dense.size == pairs
    descending = rt in H.SIMILARITY
    labs = labellings(ctx, dense, rt, k, n)
    ti, tj = H.tri_ij(n)
    same = {ln: lab[ti] == lab[tj] for ln, lab in labs.items()}
    for en, edges in edge_sets(dense).items():
        cls = H.classes(dense, edges, descending)  # the reference's classes once, counted per labelling
        want = H.count_classes(cls, edges.size)
        assert np.array_equal(want, H.histogram(dense, edges, descending))
        got = checked(ctx.dist_histogram(edges, **kw), 1, edges.size, pairs, (name, rt, en))
        print("%s rt=%d %s: %d classes in use, largest holds %d of %d" % (name, rt, en, int((got > 0).sum()), int(got.max()), pairs))
        assert np.array_equal(got, want), (name, rt, en)
        small = None
        if n <= 700 or n == 4200:  # independence of geometry: many bands, rows cut across bands
            try:
                ctx.set_option("threshold_band_bytes", 64 << 10)
                small = ctx.dist_histogram(edges, **kw)
            finally:
                ctx.set_option("threshold_band_bytes", 1 << 30)
            assert small.tobytes() == got.tobytes(), (name, rt, en, "64 KiB bands")
        for ln, lab in labs.items():
            what = (name, rt, en, ln)
            two = checked(ctx.dist_histogram(edges, labels=lab, **kw), 2, edges.size, pairs, what)
            assert np.array_equal(two, H.count_classes(cls, edges.size, same[ln])), what
            assert np.array_equal(two[0] + two[1], got[0]), what
            if ln == "singletons":
                assert not two[0].any()
            if ln == "one group":
                assert not two[1].any()
        if small is not None:
            try:
                ctx.set_option("threshold_band_bytes", 64 << 10)
                two_small = ctx.dist_histogram(edges, labels=labs["random groups"], **kw)
            finally:
                ctx.set_option("threshold_band_bytes", 1 << 30)
            assert two_small.tobytes() == ctx.dist_histogram(edges, labels=labs["random groups"], **kw).tobytes()
        if en == "all below":  # every value that is a number passes every edge
            assert int(got[0, edges.size]) + int(got[0, -1]) == pairs
        if en == "from the data":
            # the classes against the threshold kernels' own predicate, not only against numpy
            hits = D.histogram_hits(got, rt)[0]
            for b, e in enumerate(edges):
                rp = ctx.dist_threshold_count(float(e), **kw)
                assert int(rp[-1]) == int(hits[b]), (name, rt, b, float(e))


def test_sizes_count_as_the_threshold_forms_take_them(ctx):
    """DSH_SIZES is no *_DIST form: the library ranks it descending, so an edge is closed below (e <= v) and the hits at
    an edge are the classes above it -- in the kernel, in histogram_hits and in dist_threshold alike"""
    n, k, rt = 300, 21, D.SIZES
    regs = synth.synthetic_sketches(n, 10, seed=55)
    regs[7] = regs[8] = regs[9]
    ctx.set_sketches(regs)
    kw = dict(estim=2, result_type=rt, k=k)
    dense = ctx.dist_rows(**kw)
    lab = random_groups(np.random.default_rng(2), n, 20)
    assert rt in H.SIMILARITY and rt not in D.DISTANCE_TYPES
    for edges in (data_edges(dense), many_edges(dense)):
        got = checked(ctx.dist_histogram(edges, labels=lab, **kw), 2, edges.size, dense.size, "sizes")
        assert np.array_equal(got, H.histogram(dense, edges, True, H.tri_same(lab, n)))
        hits = D.histogram_hits(got, rt).sum(axis=0)
        assert np.array_equal(hits, H.hits(got, True).sum(axis=0))
        for b in range(0, edges.size, max(edges.size // 13, 1)):
            assert int(ctx.dist_threshold_count(float(edges[b]), **kw)[-1]) == int(hits[b]), (b, float(edges[b]))


@pytest.mark.parametrize("rt", [D.JI, D.MASH_DIST])
def test_row_ranges_add_up(ctx, rt):
    n, k = 700, 31
    ctx.set_sketches(synth.related_sketches(n, 12, seed=91)[0])
    kw = dict(estim=2, result_type=rt, k=k)
    dense = ctx.dist_rows(**kw)
    lab = random_groups(np.random.default_rng(3), n, 40)
    descending = rt in H.SIMILARITY
    for edges in (data_edges(dense), np.linspace(0, 1, 101).astype(F)):
        whole = ctx.dist_histogram(edges, labels=lab, **kw)
        assert np.array_equal(whole, H.histogram(dense, edges, descending, H.tri_same(lab, n)))
        assert np.array_equal(ctx.dist_histogram(edges, 0, 10**9, labels=lab, **kw), whole)  # row_end is cut at n
        for a in (77, 128, 384, 699, 700):  # inside a tile, on multiples of 128, the last (empty) row alone, nothing
            lo, hi = ctx.dist_histogram(edges, 0, a, labels=lab, **kw), ctx.dist_histogram(edges, a, n, labels=lab, **kw)
            assert np.array_equal(lo + hi, whole), a
            span = ctx.dist_rows(0, a, **kw)
            assert np.array_equal(lo, H.histogram(span, edges, descending, H.tri_same(lab, n, 0, a))), a
        mid = ctx.dist_histogram(edges, 100, 333, **kw)
        assert np.array_equal(mid, H.histogram(ctx.dist_rows(100, 333, **kw), edges, descending))
        # empty ranges: all zero, every entry written
        for rb, re in ((5, 5), (9, 3), (n, n), (n + 5, n + 9), (n - 1, n)):
            z = ctx.dist_histogram(edges, rb, re, labels=lab, **kw)
            assert z.shape == (2, edges.size + 2) and not z.any(), (rb, re)


@pytest.mark.parametrize("rt", MEASURES)
def test_rectangle_equals_the_reference(ctx, rt):
    k = 31
    descending = rt in H.SIMILARITY
    for name, make in (("related700p12", lambda: synth.related_sketches(700, 12, seed=91)[0]),
                       ("synthetic4200p10", lambda: synth.synthetic_sketches(4200, 10, seed=0x4200)),
                       ("synthetic129p10", lambda: synth.synthetic_sketches(129, 10, seed=0x77 + 129))):
        regs = make()
        n = regs.shape[0]
        ctx.set_sketches(regs)
        kw = dict(estim=2, result_type=rt, k=k)
        lab = random_groups(np.random.default_rng(n), n, max(n // 16, 2))
        rects = [(0, n // 3, n // 2, n), (n // 4, 3 * n // 4, n // 2, n), (n // 2, n // 2 + 37, 0, n), (5, 5, 0, n), (0, n, 7, 7)]
        if n > 700:
            rects = [(0, 40, 0, n), (n - 130, n, 3, n - 1)]  # rows of more than one 4096-value chunk, at an odd offset
        for q0, q1, r0, r1 in rects:
            dense = ctx.dist_rect(q0, q1, r0, r1, **kw)
            edges = data_edges(dense) if dense.size else np.array([0.5], F)
            for e in (edges, np.linspace(0, 1, 101).astype(F)):
                what = (name, rt, q0, q1, r0, r1, e.size)
                got = checked(ctx.dist_rect_histogram(e, q0, q1, r0, r1, **kw), 1, e.size, dense.size, what)
                assert np.array_equal(got, H.histogram(dense, e, descending)), what
                two = checked(ctx.dist_rect_histogram(e, q0, q1, r0, r1, labels=lab, **kw), 2, e.size, dense.size, what)
                assert np.array_equal(two, H.histogram(dense, e, descending, H.rect_same(lab, q0, q1, r0, r1))), what
                try:
                    ctx.set_option("threshold_band_bytes", 64 << 10)
                    assert ctx.dist_rect_histogram(e, q0, q1, r0, r1, labels=lab, **kw).tobytes() == two.tobytes(), what
                finally:
                    ctx.set_option("threshold_band_bytes", 1 << 30)
        if rt == D.JI and n <= 700:  # symmetric: the square is twice the triangle plus the diagonal
            e = np.linspace(0, 1, 101).astype(F)
            sq = ctx.dist_rect_histogram(e, 0, n, 0, n, labels=lab, **kw)
            tri = ctx.dist_histogram(e, labels=lab, **kw)
            diag = np.diagonal(ctx.dist_rect(0, n, 0, n, **kw)).copy()
            want = 2 * tri
            want[0] += H.histogram(diag, e, descending)[0]  # (a self pair is intra)
            assert np.array_equal(sq, want), name


@pytest.mark.parametrize("misalign", [0, 1])  # (in items of 8 bytes: the buffer stays 8-byte aligned)
def test_device_form_between_guard_bands(ctx, misalign):
    import torch

    n, k = 700, 31
    ctx.set_sketches(synth.related_sketches(n, 12, seed=91)[0])
    dense = ctx.dist_rows(estim=2, result_type=D.JI, k=k)
    lab = random_groups(np.random.default_rng(8), n, 40)
    for edges in (np.array([0.5], F), data_edges(dense), many_edges(dense)):
        for labels in (None, lab):
            planes = 1 if labels is None else 2
            want = ctx.dist_histogram(edges, labels=labels, estim=2, result_type=D.JI, k=k)
            buf = guard.Guarded(planes * (edges.size + 2), np.uint64, front=4096, back=4096, misalign=misalign, device=torch.device("cuda:0"))
            assert buf.ptr % 8 == 0
            for rnd in range(2):  # the second call finds the first one's numbers: counts are overwritten, not added to
                ctx.dist_histogram_device(buf.ptr, edges, labels=labels, estim=2, result_type=D.JI, k=k)
                buf.check("dist_histogram_device %d edges" % edges.size)
                assert buf.unwritten() == 0
                assert buf.host().tobytes() == want.tobytes()
            buf.fill(np.full(buf.n_items, 12345, np.uint64))
            ctx.dist_histogram_device(buf.ptr, edges, 300, 300, labels=labels, estim=2, result_type=D.JI, k=k)  # empty: zeros
            buf.check("empty range")
            assert not buf.host().any()


def test_cached_state_is_that_of_a_threshold_call(ctx):
    n = 3000
    ctx.set_sketches(synth.survey_sketches(n, 12, seed=0x5EED0000)[0])
    e = np.linspace(0, 1, 51).astype(F)
    lab = random_groups(np.random.default_rng(1), n, 100)
    for rt, t in ((D.JI, 0.03), (D.MASH_DIST, 0.1)):
        kw = dict(estim=2, result_type=rt, k=31)
        before = ctx.dist_rows(**kw)
        csr = ctx.dist_threshold(t, **kw)
        h1 = ctx.dist_histogram(e, labels=lab, **kw)
        after = ctx.dist_rows(**kw)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        again = ctx.dist_threshold(t, **kw)
        assert all(np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)) for a, b in zip(csr[1:], again[1:]))
        assert np.array_equal(csr[0], again[0])
        sub = ctx.dist_rows(100, 900, **kw)  # a row range, histograms of another range and of a rectangle, the range again
        ctx.dist_histogram(e, 1000, 1500, **kw)
        ctx.dist_rect_histogram(e, 0, 200, 1000, 1300, labels=lab, **kw)
        assert np.array_equal(sub.view(np.uint32), ctx.dist_rows(100, 900, **kw).view(np.uint32))
        assert ctx.dist_histogram(e, labels=lab, **kw).tobytes() == h1.tobytes()  # the same call, the same bytes


def test_error_codes(ctx):
    n = 300
    ctx.set_sketches(synth.synthetic_sketches(n, 10, seed=55))
    good = np.array([0.1, 0.2, 0.3], F)

    def err(fn, *a, **kw):
        with pytest.raises(D.DshError) as e:
            fn(*a, **kw)
        return e.value.code, str(e.value)

    assert err(ctx.dist_histogram, np.zeros(0, F))[0] == EINVAL
    assert err(ctx.dist_histogram, np.arange(D.HIST_MAX_EDGES + 1, dtype=F))[0] == EINVAL
    assert ctx.dist_histogram(np.arange(D.HIST_MAX_EDGES, dtype=F)).shape == (1, D.HIST_MAX_EDGES + 2)
    for bad, idx in (([0.1, 0.2, 0.2, 0.3], 2), ([0.3, 0.2], 1), ([-0.0, 0.0], 1), ([0.0, np.nan, 1.0], 1), ([np.nan], 0),
                     ([-np.inf, -np.inf], 1), ([0.0, 1.0, np.inf, np.inf], 3)):
        for call in (lambda e: ctx.dist_histogram(e), lambda e: ctx.dist_rect_histogram(e, 0, 10, 0, 10),
                     lambda e: ctx.dist_histogram(e, labels=np.zeros(n, np.uint32))):
            code, msg = err(call, np.array(bad, F))
            assert code == EINVAL and "edges[%d]" % idx in msg, (bad, msg)
    assert ctx.dist_histogram(np.array([-np.inf, np.inf], F)).shape == (1, 4)  # +-inf are legal edges
    lib = D.api.load_library()
    out = np.zeros(16, np.uint64)
    assert lib.dsh_dist_histogram(ctx._h, 2, 1, 31, 0, n, None, 3, None, out.ctypes.data) == EINVAL
    assert lib.dsh_dist_histogram(ctx._h, 2, 1, 31, 0, n, good.ctypes.data, 3, None, None) == EINVAL
    assert lib.dsh_dist_histogram_device(ctx._h, 2, 1, 31, 0, n, good.ctypes.data, 3, None, None) == EINVAL
    assert lib.dsh_dist_rect_histogram(ctx._h, 2, 1, 31, 0, 5, 0, 5, good.ctypes.data, 3, None, None) == EINVAL
    assert not out.any()
    assert err(ctx.dist_rect_histogram, good, 0, n + 1, 0, 5)[0] == EINVAL
    assert err(ctx.dist_rect_histogram, good, 0, 5, 0, n + 1)[0] == EINVAL
    assert err(ctx.dist_histogram, good, estim=3)[0] == EINVAL
    assert err(ctx.dist_histogram, good, result_type=9)[0] == EINVAL
    assert err(ctx.dist_histogram, good, result_type=-1)[0] == EINVAL
    assert err(ctx.dist_rect_histogram, good, 0, 5, 0, 5, estim=-1)[0] == EINVAL
    with pytest.raises(ValueError):
        ctx.dist_histogram(good, labels=np.zeros(n - 1, np.uint32))
    # out-of-order ranges are empty, as the threshold forms judge them
    assert not ctx.dist_rect_histogram(good, 9, 3, 0, 5).any() and not ctx.dist_histogram(good, 9, 3).any()
    # after the refusals the context still answers
    dense = ctx.dist_rows(estim=2, result_type=D.JI, k=31)
    assert np.array_equal(ctx.dist_histogram(good), H.histogram(dense, good, True))
    fresh = D.Context(0)
    try:
        for call in (lambda: fresh.dist_histogram(good), lambda: fresh.dist_rect_histogram(good, 0, 0, 0, 0)):
            with pytest.raises(D.DshError) as e:
                call()
            assert e.value.code == ESTATE
        assert lib.dsh_dist_histogram_device(fresh._h, 2, 1, 31, 0, 0, good.ctypes.data, 3, None, ctypes.c_void_p(8)) == ESTATE
    finally:
        fresh.close()
