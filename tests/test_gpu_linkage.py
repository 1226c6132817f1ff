"""GPU: the linkage clusters at a threshold (dsh_linkage_threshold*, dsh_linkage_tri).  The result has ONE
answer, so every comparison here is an exact comparison of uint32 arrays with the numpy model (tests/linkage_ref.py): on
matrices handed in as triangles, and on the values Context.dist_rows returns for the same context (the same float32 values:
no tolerance).  Routes, bands, chunks, batches, the partition and the LDS limit must not change a byte.  No test here tries
to reach the step-bound give-up path (tests/test_linkage_host.py does that on the CPU)."""
import ctypes

import numpy as np
import pytest

import cluster_ref
import dashing_amd
import guard
import linkage_ref as R
import thr_ref
from dashing_amd import synth

pytestmark = pytest.mark.gpu

D = dashing_amd
EINVAL, ESTATE, ENOMEM = -22, -11, -12
LINKAGES = (R.SINGLE, R.COMPLETE, R.AVERAGE)
KW = dict(estim=2, k=31)


def code(fn, *a, **kw):
    with pytest.raises(D.DshError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


def check_tri(ctx, n, tri, t, linkage, desc=0, what=""):
    want, wc = R.labels(n, tri, desc, t, linkage)
    got, gc = ctx.linkage_tri(n, tri, t, linkage, descending=bool(desc))
    assert got.dtype == np.uint32 and got.shape == (n,)
    assert np.array_equal(got, want) and gc == wc, (what, n, t, linkage, desc)
    return want, wc


# ---- the tri form ----------------------------------------------------------------------------------------------------
def test_hand_examples(ctx):
    for n in (1, 2, 3, 64, 65, 257):  # a path under COMPLETE pairs up: (0, 1), (2, 3), ...
        want, _ = check_tri(ctx, n, R.path(n), 0.5, R.COMPLETE, what="path")
        assert want.tolist() == [x - x % 2 for x in range(n)]
        check_tri(ctx, n, R.path(n), 0.5, R.AVERAGE, what="path")
        want, wc = check_tri(ctx, n, R.path(n), 0.5, R.SINGLE, what="path")
        assert wc == 1
    nan = np.array([0.1, np.nan, 0.1], np.float32)  # a NaN that blocks one merge
    assert check_tri(ctx, 3, nan, 0.5, R.COMPLETE)[0].tolist() == [0, 0, 2]
    assert check_tri(ctx, 3, nan, 0.5, R.AVERAGE)[0].tolist() == [0, 0, 2]
    assert check_tri(ctx, 3, nan, 0.5, R.SINGLE)[0].tolist() == [0, 0, 0]
    two = np.array([0.1, 2.0, 0.1], np.float32)  # a value of 2 blocks AVERAGE alone
    assert check_tri(ctx, 3, two, 1.9, R.AVERAGE)[0].tolist() == [0, 0, 2]
    assert check_tri(ctx, 3, two, 2.0, R.COMPLETE)[0].tolist() == [0, 0, 0]
    for linkage in LINKAGES:  # a NaN threshold: n singletons; nothing and one node
        got, gc = ctx.linkage_tri(7, R.path(7), float("nan"), linkage)
        assert got.tolist() == list(range(7)) and gc == 7
        got, gc = ctx.linkage_tri(0, [], 0.5, linkage)
        assert got.size == 0 and gc == 0
        got, gc = ctx.linkage_tri(1, [], 0.5, linkage)
        assert got.tolist() == [0] and gc == 1
        for t, one in ((0.5, True), (0.05, False)):
            got, gc = ctx.linkage_tri(2, [0.1], t, linkage)
            assert got.tolist() == ([0, 0] if one else [0, 1])


@pytest.mark.parametrize("n", [3, 64, 65, 129, 257, 1025])
def test_all_values_equal_every_decision_a_tie(ctx, n):
    """every pair passes and every comparison is a tie: the tie rule alone decides, and every row's nearest neighbour is one
    of the merged two at every step.  (AVERAGE up to 129, COMPLETE alone at 1025: the model's exact tie decisions are slow.)"""
    tri = np.full(n * (n - 1) // 2, 0.25, np.float32)
    for linkage in LINKAGES:
        if (linkage == R.AVERAGE and n > 129) or (linkage == R.SINGLE and n > 257):
            continue
        want, wc = check_tri(ctx, n, tri, 0.25, linkage)
        assert wc == 1 and not want.any()
        want, wc = check_tri(ctx, n, tri, 0.25, linkage, desc=1)
        assert wc == 1
        got, gc = ctx.linkage_tri(n, tri, 0.2, linkage)
        assert gc == n and got.tolist() == list(range(n))


@pytest.mark.parametrize("linkage", LINKAGES)
def test_nan_rows(ctx, linkage):
    """slots whose every value is NaN stay alone and never block the others under SINGLE; under COMPLETE and AVERAGE a
    cluster that holds a slot with one NaN cannot take the partner of that pair"""
    n = 130
    v = R.square(n, R.random_tri(n, 41, special=False))
    v[[5, 64, 129], :] = np.nan
    v[:, [5, 64, 129]] = np.nan
    v[7, 70] = v[70, 7] = np.nan
    tri = R.tri_of(v)
    for t in (0.05, 0.4, 1.0):
        want, _ = check_tri(ctx, n, tri, t, linkage)
        assert want[5] == 5 and want[64] == 64 and want[129] == 129
        if linkage != R.SINGLE:
            assert want[7] != want[70]
    all_nan = np.full(n * (n - 1) // 2, np.nan, np.float32)
    assert check_tri(ctx, n, all_nan, 0.5, linkage)[1] == n


@pytest.mark.parametrize("linkage", LINKAGES)
def test_every_row_rescans_at_every_step(ctx, linkage):
    """600 members, and at every step the nearest neighbour of every cluster is the cluster of slot 0"""
    n = 600
    tri = R.funnel(n)
    want, wc = check_tri(ctx, n, tri, 1.0, linkage)
    assert wc == 1
    want, wc = check_tri(ctx, n, tri, 0.25, linkage)
    assert 1 < wc < n


@pytest.mark.parametrize("linkage", LINKAGES)
def test_two_blocks_joined_by_one_passing_pair(ctx, linkage):
    m = 300
    tri = R.two_blocks(m, seed=5)
    want, wc = check_tri(ctx, 2 * m, tri, 0.5, linkage)
    assert wc == (1 if linkage == R.SINGLE else 2)
    if linkage != R.SINGLE:
        assert want.tolist() == [0] * m + [m] * m
    # the same with the state of the one 600-member component in global scratch, and with several small workgroups' worth
    try:
        for lds_max in (0, 64, 599, 600):
            ctx.set_option("linkage_lds_max", lds_max)
            got, gc = ctx.linkage_tri(2 * m, tri, 0.5, linkage)
            assert np.array_equal(got, want) and gc == wc, lds_max
    finally:
        ctx.set_option("linkage_lds_max", 4096)


@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 256, 257, 1025])
def test_random_matrices_at_three_thresholds(ctx, n, linkage):
    """NaN, +-0.0, +-inf, values at and above 2, ties, q at exact halves; below, around and above the point where the graph
    of passing pairs becomes one component"""
    tri = R.random_tri(n, 900 + n)
    # (at 1025 the third threshold under COMPLETE alone: the graph is one component from the second on, and the model's
    # SINGLE and AVERAGE runs take seconds)
    for t in (min(2.0 / n, 0.6), min(0.02 + 4.0 / n, 0.8), 0.3)[: 3 if n < 1025 or linkage == R.COMPLETE else 2]:
        for desc in ((0,) if n == 1025 else (0, 1)):
            check_tri(ctx, n, tri, t if not desc else 1.0 - t, linkage, desc=desc)


@pytest.mark.parametrize("linkage", LINKAGES)
def test_global_state_path_gives_the_same_bytes(ctx, linkage):
    """"linkage_lds_max" lowered so that components of 300 members keep their per-row state in global scratch; batches of a
    small budget; the whole collection as one component"""
    n = 700
    v = np.full((n, n), 0.9, np.float32)
    rng = np.random.default_rng(77)
    for b0, b1 in ((0, 300), (300, 600), (600, 650)):
        v[b0:b1, b0:b1] = rng.random((b1 - b0, b1 - b0)).astype(np.float32) * 0.4
    v = np.minimum(v, v.T)
    tri = R.tri_of(v)
    want, wc = check_tri(ctx, n, tri, 0.45, linkage)
    cell = 8 if linkage == R.AVERAGE else 4
    try:
        for opts in ({"linkage_lds_max": 100}, {"linkage_lds_max": 0, "linkage_budget_bytes": 300 * 300 * cell},
                     {"linkage_budget_bytes": 300 * 300 * cell + 50 * 50 * cell}, {"linkage_partition": 0},
                     {"threshold_band_bytes": 64 << 10}):
            for name, val in opts.items():
                ctx.set_option(name, val)
            got, gc = ctx.linkage_tri(n, tri, 0.45, linkage)
            assert np.array_equal(got, want) and gc == wc, opts
            for name, val in (("linkage_lds_max", 4096), ("linkage_budget_bytes", 8 << 30), ("linkage_partition", 1),
                              ("threshold_band_bytes", 1 << 30)):
                ctx.set_option(name, val)
        # a budget below the largest component: refused with its size and the bytes, and the context goes on
        ctx.set_option("linkage_budget_bytes", 300 * 300 * cell - 1)
        c, msg = code(ctx.linkage_tri, n, tri, 0.45, linkage)
        assert c == ENOMEM and "m = 300" in msg and str(300 * 300 * cell) in msg
    finally:
        for name, val in (("linkage_lds_max", 4096), ("linkage_budget_bytes", 8 << 30), ("linkage_partition", 1),
                          ("threshold_band_bytes", 1 << 30)):
            ctx.set_option(name, val)
    got, gc = ctx.linkage_tri(n, tri, 0.45, linkage)
    assert np.array_equal(got, want) and gc == wc


# ---- the sketch form against the model on the same context's dist_rows ----------------------------------------------
def quantile_thresholds(dense, rt):
    """five thresholds out of the dense values: hit fractions of about 0.1 %, 1 %, 5 %, 20 % and 50 %"""
    fin = np.sort(dense[np.isfinite(dense)])
    if not fin.size:
        return [0.5]
    if rt in thr_ref.SIMILARITY:
        fin = fin[::-1]
    return [float(fin[min(int(f * fin.size), fin.size - 1)]) for f in (0.001, 0.01, 0.05, 0.2, 0.5)]


def tri_shapes():
    seen, out = set(), []
    for name, make, rt, k, ts in thr_ref.oracle_cases():
        if name not in seen and name != "survey3000p12":
            seen.add(name)
            out.append((name, make, k))
    for n in (1, 2, 129):
        out.append(("synthetic%dp10" % n, (lambda n=n: synth.synthetic_sketches(n, 10, seed=0x77 + n)), 31))
    return out


def routes(ctx, t, linkage, rt, k, want, wc, what):
    """both routes, and what must not matter: many bands, small pair chunks, no partition"""
    try:
        for route in (0, 1):
            ctx.set_option("linkage_route", route)
            got, gc = ctx.linkage_threshold(t, linkage, estim=2, result_type=rt, k=k)
            assert got.dtype == np.uint32 and np.array_equal(got, want) and gc == wc, (what, "route", route)
            assert ctx.info("linkage_route") == route
        ctx.set_option("linkage_route", 0)
        ctx.set_option("threshold_band_bytes", 64 << 10)
        got, gc = ctx.linkage_threshold(t, linkage, estim=2, result_type=rt, k=k)
        assert np.array_equal(got, want) and gc == wc, (what, "bands")
        ctx.set_option("threshold_band_bytes", 1 << 30)
        ctx.set_option("linkage_route", 1)
        ctx.set_option("pairs_chunk", 257)
        got, gc = ctx.linkage_threshold(t, linkage, estim=2, result_type=rt, k=k)
        assert np.array_equal(got, want) and gc == wc, (what, "chunks")
    finally:
        ctx.set_option("linkage_route", -1)
        ctx.set_option("threshold_band_bytes", 1 << 30)
        ctx.set_option("pairs_chunk", 1 << 18)


@pytest.mark.parametrize("rt", [D.JI, D.MASH_DIST, D.CONTAINMENT_INDEX])
@pytest.mark.parametrize("shape", range(len(tri_shapes())))
def test_sketch_form_equals_the_model_on_dist_rows(ctx, shape, rt):
    name, make, k = tri_shapes()[shape]
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    dense = ctx.dist_rows(estim=2, result_type=rt, k=k)
    desc = 1 if rt in thr_ref.SIMILARITY else 0
    for x, t in enumerate(quantile_thresholds(dense, rt) + [float("nan")]):
        if abs(t) >= 2:
            continue
        single, sc = ctx.cluster_threshold(t, estim=2, result_type=rt, k=k)
        for linkage in LINKAGES:
            want, wc = R.labels(n, dense, desc, t, linkage)
            got, gc = ctx.linkage_threshold(t, linkage, estim=2, result_type=rt, k=k)
            print("%s rt=%d t=%.9g linkage %d: %d clusters (single: %d)" % (name, rt, t, linkage, wc, sc))
            assert np.array_equal(got, want) and gc == wc, (name, rt, t, linkage)
            if linkage == R.SINGLE:  # byte for byte the components
                assert np.array_equal(got, single) and gc == sc
            elif t == t:  # every cluster inside one single-linkage cluster: of the float graph, AVERAGE of the quantised one
                loose = single
                if linkage == R.AVERAGE:
                    ok = np.abs(dense) < 2  # (NaN: False)
                    qv, Q = R.q(np.where(ok, dense, 0)), int(R.q(np.float32(t)))
                    hit = ok & ((qv >= Q) if desc else (qv <= Q))
                    i, j = np.triu_indices(n, 1)
                    loose = cluster_ref.labels_fast(n, i[hit], j[hit])[0]
                assert np.array_equal(loose[got], loose)
            if linkage == R.COMPLETE and n > 1 and t == t:  # every member's worst value inside its cluster passes t
                st = ctx.group_stats(got, estim=2, result_type=rt, k=k)
                has = st.cnt > 0
                assert (st.worst[has] >= np.float32(t)).all() if desc else (st.worst[has] <= np.float32(t)).all()
            if x in (1, 3) and n > 2:
                routes(ctx, t, linkage, rt, k, want, wc, (name, rt, t, linkage))


@pytest.mark.parametrize("linkage", [R.COMPLETE, R.AVERAGE])
def test_3000_sketches(ctx, linkage):
    name, make, _, k, _ = thr_ref.oracle_cases()[6]
    assert name == "survey3000p12"
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    rt = D.MASH_DIST
    dense = ctx.dist_rows(estim=2, result_type=rt, k=k)
    ts = quantile_thresholds(dense, rt)
    t = ts[0]  # 0.1 % of the pairs pass: small components, every route and batching variant
    want, wc = first = R.labels(n, dense, 0, t, linkage)
    single, _ = ctx.cluster_threshold(t, estim=2, result_type=rt, k=k)
    routes(ctx, t, linkage, rt, k, want, wc, (name, t, linkage))
    if linkage == R.COMPLETE:
        assert np.array_equal(single[want], single)
    big, bc = R.labels(n, dense, 0, ts[1], linkage)  # 1 %: one component of nearly all sketches, once
    got, gc = ctx.linkage_threshold(ts[1], linkage, estim=2, result_type=rt, k=k)
    assert np.array_equal(got, big) and gc == bc
    # batches: a budget that holds the largest component and little more; then one that does not hold it
    t = ts[0]
    want, wc = first
    single, _ = ctx.cluster_threshold(t, estim=2, result_type=rt, k=k)
    m = int(np.bincount(single).max())
    cell = 8 if linkage == R.AVERAGE else 4
    try:
        ctx.set_option("linkage_budget_bytes", max(m * m * cell, 64))
        for route in (0, 1):
            ctx.set_option("linkage_route", route)
            got, gc = ctx.linkage_threshold(t, linkage, estim=2, result_type=rt, k=k)
            assert np.array_equal(got, want) and gc == wc, route
        if m * m * cell > 64:
            ctx.set_option("linkage_budget_bytes", m * m * cell - 1)
            c, msg = code(ctx.linkage_threshold, t, linkage, estim=2, result_type=rt, k=k)
            assert c == ENOMEM and "m = %d" % m in msg and str(m * m * cell) in msg
    finally:
        ctx.set_option("linkage_budget_bytes", 8 << 30)
        ctx.set_option("linkage_route", -1)
    got, gc = ctx.linkage_threshold(t, linkage, estim=2, result_type=rt, k=k)  # the next call on the context works
    assert np.array_equal(got, want) and gc == wc
    try:
        ctx.set_option("linkage_partition", 0)  # one component of 3000
        got, gc = ctx.linkage_threshold(t, linkage, estim=2, result_type=rt, k=k)
        assert np.array_equal(got, want) and gc == wc
    finally:
        ctx.set_option("linkage_partition", 1)


def test_all_zero_sketches(ctx):
    n = 70
    ctx.set_sketches(np.zeros((n, 1 << 10), np.uint8))
    for rt in (D.JI, D.MASH_DIST):
        dense = ctx.dist_rows(estim=2, result_type=rt, k=31)
        desc = 1 if rt in thr_ref.SIMILARITY else 0
        for t in (0.0, 0.5, 1.0):
            for linkage in LINKAGES:
                want, wc = R.labels(n, dense, desc, t, linkage)
                for route in (0, 1):
                    try:
                        ctx.set_option("linkage_route", route)
                        got, gc = ctx.linkage_threshold(t, linkage, estim=2, result_type=rt, k=31)
                    finally:
                        ctx.set_option("linkage_route", -1)
                    assert np.array_equal(got, want) and gc == wc, (rt, t, linkage, route)


@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_device_form_between_guard_bands(ctx, misalign):
    import torch

    n, p = 700, 12
    regs = synth.related_sketches(n, p, seed=91)[0]
    ctx.set_sketches(regs)
    for linkage in (R.COMPLETE, R.AVERAGE):
        for t in (0.03, 0.6, 1.5):
            want, wc = ctx.linkage_threshold(t, linkage, result_type=D.JI, **KW)
            buf = guard.Guarded(n, np.uint32, front=4096, back=4096, misalign=misalign, device=torch.device("cuda:0"))
            nc = ctx.linkage_threshold_device(buf.ptr, t, linkage, result_type=D.JI, **KW)
            buf.check("linkage_threshold_device t=%g" % t)
            assert buf.unwritten() == 0
            assert np.array_equal(buf.host(), want) and nc == wc
        assert wc == n  # (t = 1.5: nothing passes, and still every label is written)


def test_dense_calls_around_a_linkage_call(ctx):
    n, p = 3000, 12
    regs = synth.survey_sketches(n, p, seed=0x5EED0000)[0]
    ctx.set_sketches(regs)
    for rt, t in ((D.JI, 0.3), (D.MASH_DIST, 0.02)):
        before = ctx.dist_rows(estim=2, result_type=rt, k=31)
        labs = []
        for route in (0, 1):
            try:
                ctx.set_option("linkage_route", route)
                labs.append(ctx.linkage_threshold(t, "average", estim=2, result_type=rt, k=31))
            finally:
                ctx.set_option("linkage_route", -1)
            after = ctx.dist_rows(estim=2, result_type=rt, k=31)
            assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        assert np.array_equal(labs[0][0], labs[1][0]) and labs[0][1] == labs[1][1]
        sub = ctx.dist_rows(100, 900, estim=2, result_type=rt, k=31)
        again = ctx.linkage_threshold(t, "average", estim=2, result_type=rt, k=31)
        assert np.array_equal(again[0], labs[0][0])
        assert np.array_equal(sub.view(np.uint32), ctx.dist_rows(100, 900, estim=2, result_type=rt, k=31).view(np.uint32))


def test_error_codes(ctx):
    ctx.set_sketches(synth.synthetic_sketches(40, 10, seed=3))
    tri = R.path(5)
    assert code(ctx.linkage_threshold, 0.5, 3)[0] == EINVAL
    assert code(ctx.linkage_threshold, 0.5, -1)[0] == EINVAL
    assert code(ctx.linkage_threshold, 0.5, "average", result_type=D.SIZES)[0] == EINVAL
    assert code(ctx.linkage_threshold, 2.0, "average")[0] == EINVAL
    assert code(ctx.linkage_threshold, -2.0, "average")[0] == EINVAL
    assert code(ctx.linkage_threshold, float("inf"), "average")[0] == EINVAL
    assert code(ctx.linkage_threshold_device, 0, 0.5, "complete")[0] == EINVAL  # no buffer
    assert code(ctx.linkage_tri, 5, tri, 0.5, 7)[0] == EINVAL
    assert code(ctx.linkage_tri, 5, tri, 2.0, "average")[0] == EINVAL
    with pytest.raises(ValueError):
        ctx.linkage_threshold(0.5, "ward")
    with pytest.raises(ValueError):
        ctx.linkage_tri(5, tri[:-1], 0.5, "complete")
    lib = D.api.load_library()
    nc = ctypes.c_uint64()
    lab = np.zeros(5, np.uint32)
    assert lib.dsh_linkage_tri(ctx._h, 5, None, 0, 0.5, 1, lab.ctypes.data, ctypes.byref(nc)) == EINVAL  # no values
    assert lib.dsh_linkage_tri(ctx._h, 5, tri.ctypes.data, 0, 0.5, 1, None, ctypes.byref(nc)) == EINVAL  # no labels
    assert lib.dsh_linkage_tri(ctx._h, 1 << 32, tri.ctypes.data, 0, 0.5, 1, lab.ctypes.data, ctypes.byref(nc)) == EINVAL
    assert lib.dsh_linkage_threshold(ctx._h, 2, 1, 31, 0.5, 1, None, ctypes.byref(nc)) == EINVAL
    for bad in (("linkage_route", 2), ("linkage_partition", 2), ("linkage_lds_max", 6145), ("linkage_budget_bytes", 0)):
        with pytest.raises(D.DshError):
            ctx.set_option(*bad)
    # inf thresholds are ordinary values for SINGLE and COMPLETE
    got, gc = ctx.linkage_threshold(float("inf"), "complete", result_type=D.MASH_DIST, **KW)
    want, wc = R.labels(40, ctx.dist_rows(result_type=D.MASH_DIST, **KW), 0, float("inf"), R.COMPLETE)
    assert np.array_equal(got, want) and gc == wc
    # after the refusals the context still answers
    got, gc = ctx.linkage_tri(5, tri, 0.5, "complete")
    assert got.tolist() == [0, 0, 2, 2, 4] and gc == 3
    # the sketch forms need sketches; the tri form does not
    fresh = D.Context(0)
    try:
        assert code(fresh.linkage_threshold, 0.5)[0] == ESTATE
        assert code(fresh.linkage_threshold_device, 0, 0.5)[0] == ESTATE
        got, gc = fresh.linkage_tri(5, tri, 0.5, "complete")
        assert got.tolist() == [0, 0, 2, 2, 4] and gc == 3
    finally:
        fresh.close()


def test_n_0_1_2_sketches(ctx):
    for n in (1, 2):
        ctx.set_sketches(synth.synthetic_sketches(n, 10, seed=9))
        dense = ctx.dist_rows(result_type=D.JI, **KW)
        for linkage in LINKAGES:
            for t in (0.0, 1.0):
                got, gc = ctx.linkage_threshold(t, linkage, result_type=D.JI, **KW)
                want, wc = R.labels(n, dense, 1, t, linkage)
                assert np.array_equal(got, want) and gc == wc
    ctx.alloc(0, 10)
    for linkage in LINKAGES:
        got, gc = ctx.linkage_threshold(0.5, linkage)
        assert got.size == 0 and gc == 0
