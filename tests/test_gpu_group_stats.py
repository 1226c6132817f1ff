"""GPU: dsh_group_stats*  -- per-group counts, sums, worst values and medoids of a labelling.  The result
has ONE answer, so every comparison is exact array equality (worst as float values with NaN == NaN) with the numpy
reference (tests/group_stats_ref.py) fed with Context.dist_rows of the SAME context: the same float32 values, no tolerance.
Every case runs under both routes ("stats_route" 0 dense, 1 pairs), which must equal the reference and each other."""
import numpy as np
import pytest

import dashing_amd
import group_stats_ref as R
import guard
from dashing_amd import synth
from test_gpu_cluster import quantile_thresholds, tri_shapes

pytestmark = pytest.mark.gpu

D = dashing_amd
EINVAL, ESTATE = -22, -11
MEASURES = [D.JI, D.MASH_DIST, D.CONTAINMENT_INDEX]
ROUTES = ("dense", "pairs")


def shapes():
    return tri_shapes() + [("synthetic4200p10", (lambda: synth.synthetic_sketches(4200, 10, seed=0x4200)), 31)]


def reference(ctx, rt, k):
    n = ctx.n
    dense = ctx.dist_rows(estim=2, result_type=rt, k=k)
    return dense, R.Ref(R.square(dense, n), rt in R.SIMILARITY)


def random_groups(rng, n, groups):
    """group ids that are slots of OTHER groups as often as not: not idempotent"""
    ids = rng.choice(n, size=min(max(groups, 1), n), replace=False).astype(np.uint32)
    return ids[rng.integers(ids.size, size=n)]


def labellings(ctx, dense, rt, k, n):
    """name -> labels, equal labellings once"""
    ar = np.arange(n, dtype=np.uint32)
    out = {"singletons": ar, "one group": np.zeros(n, np.uint32), "even / odd": (ar % 2) % max(n, 1),
           "random groups": random_groups(np.random.default_rng(n + rt), n, max(n // 16, 2))}
    ts = quantile_thresholds(dense, rt, n)
    for x, t in enumerate(ts):
        out["cluster t%d" % x] = ctx.cluster_threshold(float(np.float32(t)), estim=2, result_type=rt, k=k)[0]
    out["greedy best"] = ctx.greedy_extend(float(np.float32(ts[3 if len(ts) > 3 else 0])), 0, None, "best", estim=2, result_type=rt, k=k)[0]
    seen, uniq = set(), {}
    for name, lab in out.items():
        if lab.tobytes() not in seen:
            seen.add(lab.tobytes())
            uniq[name] = lab
    return uniq


def check(ctx, ref, lab, rt, k, what):
    want = ref.stats(lab)
    got = {}
    for route in ROUTES:
        r = ctx.group_stats(lab, estim=2, result_type=rt, k=k, route=route)
        assert ctx.info("stats_route") == ROUTES.index(route)
        assert [a.dtype for a in r] == [np.uint32, np.uint32, np.int64, np.float32] and all(a.shape == (ctx.n,) for a in r)
        assert R.same(r, want), (what, route)
        got[route] = r
    for a, b in zip(got["dense"], got["pairs"]):
        assert a.tobytes() == b.tobytes(), what  # byte for byte: also the sign of a zero and the NaN's payload
    return got["dense"]


@pytest.mark.parametrize("rt", MEASURES)
@pytest.mark.parametrize("shape", range(len(shapes())))
def test_both_routes_equal_the_reference(ctx, shape, rt):
    name, make, k = shapes()[shape]
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    dense, ref = reference(ctx, rt, k)
    descending = rt in R.SIMILARITY
    for lname, lab in labellings(ctx, dense, rt, k, n).items():
        r = check(ctx, ref, lab, rt, k, (name, rt, lname))
        print("%s rt=%d %s: %d groups, %d slots with pairs" % (name, rt, lname, np.unique(lab).size, int((r.cnt > 0).sum())))
        # the derived quantities of the binding
        assert np.array_equal(r.diameter, R.diameter(lab, r.worst, descending), equal_nan=True)
        ok = r.cnt > 0
        assert np.isnan(r.mean[~ok]).all() and np.array_equal(r.mean[ok], r.sum[ok] / r.cnt[ok] / 2.0**30)
        if lname == "singletons":
            assert np.array_equal(r.medoid, lab) and not r.cnt.any() and not r.sum.any() and np.isnan(r.worst).all()
        if lname == "one group" and n > 1 and np.isfinite(dense).all():
            assert (r.cnt == n - 1).all() and (r.medoid == r.medoid[0]).all()
        # independence of geometry: many bands with rows cut across bands; chunks of 257 pairs (n <= 700: the chunks
        # of the larger shapes are test_geometry_at_4200's)
        if n <= 700:
            try:
                ctx.set_option("threshold_band_bytes", 64 << 10)
                ctx.set_option("pairs_chunk", 257)
                again = check(ctx, ref, lab, rt, k, (name, rt, lname, "small bands and chunks"))
            finally:
                ctx.set_option("threshold_band_bytes", 1 << 30)
                ctx.set_option("pairs_chunk", 1 << 18)
            for a, b in zip(again, r):
                assert a.tobytes() == b.tobytes()


def test_geometry_at_4200(ctx):
    """rows of more than one 4096-value chunk under 64 KiB bands (about four rows each), and a pair list of many chunks"""
    n, rt, k = 4200, D.MASH_DIST, 31
    ctx.set_sketches(synth.synthetic_sketches(n, 10, seed=0x4200))
    dense, ref = reference(ctx, rt, k)
    rng = np.random.default_rng(5)
    few, many = random_groups(rng, n, 3), random_groups(rng, n, 600)  # P_in: a third of the triangle; about 13 000 pairs
    want_few, want_many = ref.stats(few), ref.stats(many)
    try:
        ctx.set_option("threshold_band_bytes", 64 << 10)
        ctx.set_option("pairs_chunk", 257)
        assert R.same(ctx.group_stats(few, estim=2, result_type=rt, k=k, route="dense"), want_few)
        assert R.same(ctx.group_stats(many, estim=2, result_type=rt, k=k, route="dense"), want_many)
        assert R.same(ctx.group_stats(many, estim=2, result_type=rt, k=k, route="pairs"), want_many)
        ctx.set_option("pairs_chunk", 100_003)
        assert R.same(ctx.group_stats(few, estim=2, result_type=rt, k=k, route="pairs"), want_few)
    finally:
        ctx.set_option("threshold_band_bytes", 1 << 30)
        ctx.set_option("pairs_chunk", 1 << 18)


def test_auto_route(ctx):
    """20 * P_in <= n (n - 1) / 2 takes the pairs route; the option holds until it is set back"""
    n = 300
    ctx.set_sketches(synth.synthetic_sketches(n, 10, seed=3))
    ar = np.arange(n, dtype=np.uint32)
    a = ctx.group_stats(ar)
    assert ctx.info("stats_route") == 1
    b = ctx.group_stats(np.zeros(n, np.uint32))
    assert ctx.info("stats_route") == 0
    # groups of s: P_in = n (s - 1) / 2; 20 P_in <= n (n - 1) / 2 iff 20 (s - 1) <= n - 1: s = 15 pairs, s = 20 dense
    ctx.group_stats(ar // 15)
    assert ctx.info("stats_route") == 1
    ctx.group_stats(ar // 20)
    assert ctx.info("stats_route") == 0
    try:
        ctx.set_option("stats_route", 0)
        assert R.same(ctx.group_stats(ar), a) and ctx.info("stats_route") == 0
        ctx.set_option("stats_route", 1)
        assert R.same(ctx.group_stats(np.zeros(n, np.uint32)), b) and ctx.info("stats_route") == 1
        for bad in (-2, 2):
            with pytest.raises(D.DshError):
                ctx.set_option("stats_route", bad)
    finally:
        ctx.set_option("stats_route", -1)
    with pytest.raises(ValueError):
        ctx.group_stats(ar, route="fastest")


def test_empty_sketches_inside_a_group(ctx):
    """two all-zero sketches: the value of a pair with one is whatever the measure gives, NaN where it is 0 / 0 -- such a
    pair is excluded, cnt and the medoid follow"""
    n = 129
    regs = synth.synthetic_sketches(n, 10, seed=0x77 + n)
    regs[5] = 0
    regs[77] = 0
    ctx.set_sketches(regs)
    nans = 0
    for rt in MEASURES:
        dense, ref = reference(ctx, rt, 31)
        V = R.square(dense, n)
        nans += int(np.isnan(dense).sum())
        for lab in (np.zeros(n, np.uint32), (np.arange(n, dtype=np.uint32) % 3) + 2):  # (5 and 77 share the group x % 3 == 2)
            r = check(ctx, ref, lab, rt, 31, ("empty", rt))
            same = lab[:, None] == lab[None, :]
            with np.errstate(invalid="ignore"):
                assert np.array_equal(r.cnt, (same & ~np.isnan(V) & (np.abs(V) < 2)).sum(1))
    assert nans > 0  # (the case exists: at least one measure gives NaN for the empty pair)


def test_null_outputs_one_at_a_time(ctx):
    n = 300
    ctx.set_sketches(synth.synthetic_sketches(n, 10, seed=3))
    lab = random_groups(np.random.default_rng(1), n, 7)
    lib = D.api.load_library()
    for route in ROUTES:
        want = ctx.group_stats(lab, route=route)
        ctx.set_option("stats_route", ROUTES.index(route))
        try:
            for skip in range(5):  # (4: none left out)
                bufs = [guard.Guarded(n, dt, device=None) for dt in (np.uint32, np.uint32, np.uint64, np.float32)]
                ptrs = [None if x == skip else b.ptr for x, b in enumerate(bufs)]
                assert lib.dsh_group_stats(ctx._h, 2, D.JI, 31, lab.ctypes.data, *ptrs) == 0
                for x, b in enumerate(bufs):
                    b.check("output %d, without %d" % (x, skip))
                    if x == skip:
                        assert b.unwritten() == n
                    else:
                        assert b.unwritten() == 0 and b.host().tobytes() == want[x].tobytes()
            assert lib.dsh_group_stats(ctx._h, 2, D.JI, 31, lab.ctypes.data, None, None, None, None) == 0
        finally:
            ctx.set_option("stats_route", -1)


@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_device_form_between_guard_bands(ctx, misalign):
    import torch

    n = 700
    ctx.set_sketches(synth.related_sketches(n, 12, seed=91)[0])
    dev = torch.device("cuda:0")
    for lab in (np.zeros(n, np.uint32), random_groups(np.random.default_rng(2), n, 40)):
        for route in ROUTES:
            want = ctx.group_stats(lab, result_type=D.MASH_DIST, route=route)
            for skip in (4, 0, 2):
                bufs = [guard.Guarded(n, dt, front=4096, back=4096, misalign=misalign, device=dev)
                        for dt in (np.uint32, np.uint32, np.uint64, np.float32)]
                ptrs = [0 if x == skip else b.ptr for x, b in enumerate(bufs)]
                ctx.group_stats_device(lab, *ptrs, result_type=D.MASH_DIST, route=route)
                for x, b in enumerate(bufs):
                    b.check("group_stats_device output %d" % x)
                    if x == skip:
                        assert b.unwritten() == n
                    else:
                        assert b.unwritten() == 0 and b.host().tobytes() == want[x].tobytes()


def test_dense_calls_around_a_stats_call(ctx):
    n = 700
    ctx.set_sketches(synth.related_sketches(n, 12, seed=91)[0])
    lab = random_groups(np.random.default_rng(3), n, 20)
    for rt in (D.JI, D.MASH_DIST):
        before = ctx.dist_rows(estim=2, result_type=rt, k=31)
        sub = ctx.dist_rows(100, 300, estim=2, result_type=rt, k=31)
        pl, pr = np.array([5, 699, 3], np.uint32), np.array([2, 0, 3], np.uint32)
        pairs = ctx.dist_pairs(pl, pr, [rt], estim=2, k=31)
        first = None
        for route in ROUTES:
            r = ctx.group_stats(lab, estim=2, result_type=rt, k=31, route=route)
            assert np.array_equal(before.view(np.uint32), ctx.dist_rows(estim=2, result_type=rt, k=31).view(np.uint32)), route
            assert np.array_equal(sub.view(np.uint32), ctx.dist_rows(100, 300, estim=2, result_type=rt, k=31).view(np.uint32))
            assert np.array_equal(pairs.view(np.uint32), ctx.dist_pairs(pl, pr, [rt], estim=2, k=31).view(np.uint32))
            again = ctx.group_stats(lab, estim=2, result_type=rt, k=31, route=route)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r, again))
            first = first or r
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r, first))


def test_error_codes_and_tiny_collections(ctx):
    def err(fn, *a, **kw):
        with pytest.raises(D.DshError) as e:
            fn(*a, **kw)
        return e.value

    fresh = D.Context(0)
    try:
        for route in ("auto",) + ROUTES:
            assert err(fresh.group_stats, np.zeros(0, np.uint32), route=route).code == ESTATE
        assert err(fresh.group_stats_device, np.zeros(0, np.uint32), 0, 0, 0, 0).code == ESTATE
    finally:
        fresh.close()
    n = 129
    ctx.set_sketches(synth.synthetic_sketches(n, 10, seed=0x77 + n))
    lab = np.zeros(n, np.uint32)
    lab[17] = n
    for route in ROUTES:
        e = err(ctx.group_stats, lab, route=route)
        assert e.code == EINVAL and "labels[17]" in str(e)
        assert err(ctx.group_stats, np.zeros(n, np.uint32), result_type=D.SIZES, route=route).code == EINVAL
        assert err(ctx.group_stats, np.zeros(n, np.uint32), result_type=9, route=route).code == EINVAL
        assert err(ctx.group_stats, np.zeros(n, np.uint32), estim=3, route=route).code == EINVAL
    e = err(ctx.group_stats_device, lab, 0, 0, 0, 0)
    assert e.code == EINVAL and "labels[17]" in str(e)
    lib = D.api.load_library()
    assert lib.dsh_group_stats(ctx._h, 2, D.JI, 31, None, None, None, None, None) == EINVAL  # no labels for n > 0
    # after the refusals the context still answers
    r = ctx.group_stats(np.zeros(n, np.uint32))
    assert (r.cnt == n - 1).all()
    # n == 1, n == 2, n == 0
    for m in (1, 2):
        ctx.set_sketches(synth.synthetic_sketches(m, 10, seed=0x77 + m))
        _, ref = reference(ctx, D.JI, 31)
        for lab in (np.zeros(m, np.uint32), np.arange(m, dtype=np.uint32), np.full(m, m - 1, np.uint32)):
            check(ctx, ref, lab, D.JI, 31, ("tiny", m))
    ctx.alloc(0, 10)
    for route in ("auto",) + ROUTES:
        r = ctx.group_stats(np.zeros(0, np.uint32), route=route)
        assert all(a.size == 0 for a in r)
    assert lib.dsh_group_stats_device(ctx._h, 2, D.JI, 31, None, None, None, None, None) == 0
