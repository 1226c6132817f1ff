"""GPU: the density clusters at a threshold (dsh_dbscan_threshold*, dsh_dbscan_tri, dsh_degree_threshold*).
The definition has ONE answer, so every comparison here is an exact comparison of integer arrays -- labels, kind, degree and
both counts -- with the numpy model (tests/dbscan_ref.py, held to a textbook DBSCAN by tests/test_dbscan_ref.py): on matrices
built by hand (dbscan_tri), on the graph of the hits Context.dist_threshold returns for the same context (the same float32
values: no tolerance), and on the graph of the CPU oracle at thresholds chosen inside a gap of the oracle's values.  Every case
runs with a small band (walk 2 recomputes its bands) and with the whole triangle as one band (walk 2 reuses walk 1's values).
No test here tries to reach the union-find's step-bound give-up path."""
import ctypes

import numpy as np
import pytest

import cluster_ref
import dashing_amd
import dbscan_ref
import guard
import thr_ref
from dashing_amd import synth
from test_gpu_cluster import gap_threshold, quantile_thresholds, tri_shapes

pytestmark = pytest.mark.gpu

D = dashing_amd
EINVAL, ESTATE = -22, -11
SMALL_BAND, ONE_BAND = 64 << 10, 1 << 30  # "threshold_band_bytes": the recompute route and the kept one-band route
SLAB = 512  # kDbSlab (csrc/kernels.h): the band rows a thread of k_db_deg_cols walks
NOISE, BORDER, CORE = dbscan_ref.NOISE, dbscan_ref.BORDER, dbscan_ref.CORE


def same(got, want, what):
    for name, g, w in zip(("labels", "kind", "degree"), got[:3], want[:3]):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.flatnonzero(g != w)[:8])
    assert got[3] == want[3] and got[4] == want[4], (what, got[3:], want[3:])


def both_bands(ctx, call, want, what, small=SMALL_BAND):
    try:
        for band in (small, ONE_BAND):
            ctx.set_option("threshold_band_bytes", band)
            same(call(), want, (what, band))
    finally:
        ctx.set_option("threshold_band_bytes", ONE_BAND)


def check_tri(ctx, n, tri, desc, t, min_pts, assign, what):
    """dbscan_tri against the model over the values of `tri` that pass; returns the model's result"""
    lhs, rhs, val = dbscan_ref.tri_edges(n, tri, t, desc)
    want = dbscan_ref.dbscan(n, lhs, rhs, val, min_pts, assign, desc)
    both_bands(ctx, lambda: ctx.dbscan_tri(tri, desc, t, min_pts, assign, n_nodes=n), want, (what, min_pts, assign, desc))
    assert dbscan_ref.is_labelling(want[0])
    return want


def built(n, edges, desc):
    """the triangle with the edges' values where desc, else 2 - value, and the threshold both pass at: a non-edge holds 0 (desc:
    below 0.5) or 2 (above 1.5)"""
    lhs, rhs, val = edges
    if desc:
        return dbscan_ref.to_tri(n, lhs, rhs, val, 0.0), 0.5
    return dbscan_ref.to_tri(n, lhs, rhs, 2.0 - val, 2.0), 1.5


# ---- dbscan_tri on built matrices ------------------------------------------------------------------------------------
def test_chain_of_2000(ctx):
    n = 2000
    tri, t = built(n, dbscan_ref.chain(n), True)
    lab, kind, deg, nc, nn = check_tri(ctx, n, tri, True, t, 3, "first", "chain")
    assert (lab == 1).all() and nc == 1 and nn == 0  # the label is the smallest CORE: larger than the border 0
    assert kind[0] == kind[n - 1] == BORDER and (kind[1 : n - 1] == CORE).all()
    assert check_tri(ctx, n, tri, True, t, 4, "best", "chain")[4] == n


@pytest.mark.parametrize("hub", [0, 350, 699])
def test_stars(ctx, hub):
    n = 700
    for desc in (True, False):
        tri, t = built(n, dbscan_ref.star(n, hub), desc)
        lab, kind, deg, nc, nn = check_tri(ctx, n, tri, desc, t, n, "first", "star")  # leaves + 1
        assert (lab == hub).all() and nc == 1 and nn == 0 and kind[hub] == CORE and (np.delete(kind, hub) == BORDER).all()
        assert deg[hub] == n - 1
        assert check_tri(ctx, n, tri, desc, t, n + 1, "best", "star")[4] == n  # leaves + 2


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_two_cliques_and_a_bridge(ctx, where):
    m = 40
    for desc in (True, False):
        for va, vb in ((0.9, 0.8), (0.8, 0.9), (0.75, 0.75)):
            n, bridge, (ca, cb), edges = dbscan_ref.bridged_cliques(m, where, va, vb)
            tri, t = built(n, edges, desc)
            for assign in ("first", "best"):
                lab, kind, deg, nc, nn = check_tri(ctx, n, tri, desc, t, m, assign, ("bridge", where, va, vb))
                assert nc == 2 and nn == 0 and kind[bridge] == BORDER and deg[bridge] == 2 and lab[ca] != lab[cb]
                # built() keeps the order of the values in both directions: the larger of va, vb is the better one
                to = min(ca, cb) if assign == "first" or va == vb else (ca if va > vb else cb)
                assert lab[bridge] == lab[to]
            # single linkage over the same hits welds the two cliques through the bridge
            lhs, rhs, _ = dbscan_ref.tri_edges(n, tri, t, desc)
            assert ctx.cluster_pairs(n, lhs, rhs)[1] == 1


def test_a_core_whose_neighbours_all_go_elsewhere(ctx):
    """min_pts 4: the core 0 has the non-cores 1, 2, 3 as its only neighbours; each of them also touches a core of its own (4, 5,
    6, which have two leaves each) with a better value.  Under "best" they leave, and 0 is a cluster of one core."""
    pairs = [(0, 1), (0, 2), (0, 3), (1, 4), (2, 5), (3, 6)] + [(4 + x, 7 + 2 * x + y) for x in range(3) for y in range(2)]
    vals = [0.6] * 3 + [0.9] * 3 + [1.0] * 6
    edges = dbscan_ref.edge_list(pairs, vals)
    for desc in (True, False):
        tri, t = built(13, edges, desc)
        lab, kind, _, nc, nn = check_tri(ctx, 13, tri, desc, t, 4, "best", "lonely core")
        assert nc == 4 and nn == 0 and lab[0] == 0 and kind[0] == CORE and not (lab[1:] == 0).any()
        assert lab[1:4].tolist() == [4, 5, 6] and (kind[1:4] == BORDER).all()
        lab, _, _, nc, _ = check_tri(ctx, 13, tri, desc, t, 4, "first", "lonely core")
        assert nc == 4 and lab[:4].tolist() == [0, 0, 0, 0]


def test_nan_and_infinities(ctx):
    n = 200
    rng = np.random.default_rng(31)
    tri = (rng.random(n * (n - 1) // 2) < 0.03).astype(np.float32)
    special = rng.permutation(tri.size)[:900]
    tri[special[:300]] = np.nan
    tri[special[300:600]] = np.inf
    tri[special[600:]] = -np.inf
    for desc, t in ((True, 0.5), (False, 0.5), (True, np.inf), (False, -np.inf), (True, float("nan"))):
        for min_pts, assign in ((2, "first"), (5, "best"), (9, "best")):
            lab, kind, deg, nc, nn = check_tri(ctx, n, tri, desc, t, min_pts, assign, "specials")
            if t != t:
                assert nn == n and not deg.any()


def test_no_node_one_node_two_nodes(ctx):
    e = np.zeros(0, np.float32)
    for min_pts in (1, 2, 3):
        for assign in ("first", "best"):
            got = ctx.dbscan_tri(e, True, 0.5, min_pts, assign, n_nodes=0)
            assert [a.size for a in got[:3]] == [0, 0, 0] and got[3:] == (0, 0)
            check_tri(ctx, 1, e, True, 0.5, min_pts, assign, "one node")
            for v in (1.0, 0.0, np.nan):
                check_tri(ctx, 2, np.array([v], np.float32), True, 0.5, min_pts, assign, "two nodes")
    assert ctx.dbscan_tri(e, True, 0.5, 1, n_nodes=1)[3:] == (1, 0)
    assert ctx.dbscan_tri(e, True, 0.5, 2, n_nodes=1)[3:] == (0, 1)
    assert ctx.dbscan_tri([1.0], True, 0.5, 2)[3:] == (1, 0)


def test_a_row_that_crosses_the_chunk(ctx):
    """n = 4200: row 3 holds 4196 values, more than one 4096-value chunk; its hits lie in the second chunk"""
    n = 4200
    edges = dbscan_ref.edge_list([(3, 4100), (3, 4199)])
    tri, t = built(n, edges, True)
    for min_pts, kinds in ((2, (CORE, CORE, CORE)), (3, (CORE, BORDER, BORDER)), (4, (NOISE, NOISE, NOISE))):
        lab, kind, deg, nc, nn = check_tri(ctx, n, tri, True, t, min_pts, "best", "long row")
        assert tuple(kind[[3, 4100, 4199]]) == kinds and deg[3] == 2 and deg[4100] == deg[4199] == 1
        assert nn == n - 3 + 3 * (min_pts == 4) and nc == (min_pts < 4)


@pytest.mark.parametrize("n", [SLAB - 1, SLAB, SLAB + 1, SLAB + 2, 2 * SLAB + 1, 2 * SLAB + 2])
def test_around_the_column_kernels_slab(ctx, n):
    """a dense random 0/1 matrix whose band of n - 1 (or n) rows is just short of, exactly, and just over one and two slabs"""
    rng = np.random.default_rng(n)
    tri = (rng.random(n * (n - 1) // 2) < 0.4).astype(np.float32)
    lhs, rhs, val = dbscan_ref.tri_edges(n, tri, 0.5, True)
    deg = dbscan_ref.degrees(n, lhs, rhs)
    mid = int(np.median(deg)) + 1  # about half the slots are cores
    for min_pts in (mid, int(deg.max()) + 1):
        check_tri(ctx, n, tri, True, 0.5, min_pts, "first", "slab")


def test_fuzz_200_random_graphs(ctx):
    rng = np.random.default_rng(0xDB5CA7)
    kinds = np.zeros(3, np.int64)
    for g in range(200):
        n = int(rng.integers(2, 301))
        dens = (1.0 / n, 5.0 / n, 0.5)[g % 3]
        desc = bool(g & 1)
        min_pts = int(rng.integers(1, 9))
        size = n * (n - 1) // 2
        edge = rng.random(size) < dens
        # few distinct values, so that exact ties between a border's core neighbours are common
        tri = np.where(edge, rng.integers(0, 4, size) / 8.0 + (0.5 if desc else 0.0), 0.0 if desc else 1.0).astype(np.float32)
        t = 0.5 if desc else 0.375
        for assign in ("first", "best"):
            kinds += np.bincount(check_tri(ctx, n, tri, desc, t, min_pts, assign, ("fuzz", g, n))[1], minlength=3)
    assert kinds.min() > 1000, kinds  # the fuzz saw every kind often


# ---- the sketch form against the hits of the same context ------------------------------------------------------------
def check_hits(ctx, n, t, rt, k, min_pts_list, small=None, what=""):
    """every min_pts and both rules at threshold t against the model over dist_threshold's hits; returns the hit count.  The
    small band is 64 KiB, or a sixteenth of the triangle where that is more (3 000 sketches: 275 bands would only repeat
    what 16 show, in every one of the 60 calls of a case)"""
    small = max(SMALL_BAND, n * (n - 1) // 2 * 4 // 16) if small is None else small
    desc = rt in thr_ref.SIMILARITY
    rp, col, val = ctx.dist_threshold(t, estim=2, result_type=rt, k=k)
    lhs, rhs = cluster_ref.csr_edges(rp, col)
    deg = dbscan_ref.degrees(n, lhs, rhs)
    assert np.array_equal(ctx.degree_threshold(t, estim=2, result_type=rt, k=k), deg), (what, t)
    single = ctx.cluster_threshold(t, estim=2, result_type=rt, k=k)
    seen = {}  # core set -> labels of the core-core edges: loose thresholds make every small min_pts the same graph
    for min_pts in min_pts_list:
        core = deg.astype(np.int64) + 1 >= min_pts
        if core.tobytes() not in seen:
            seen[core.tobytes()] = dbscan_ref.core_labels(n, lhs, rhs, core)
        for assign in ("first", "best"):
            want = dbscan_ref.dbscan(n, lhs, rhs, val, min_pts, assign, desc, core_lab=seen[core.tobytes()], deg=deg)
            both_bands(ctx, lambda: ctx.dbscan_threshold(t, min_pts, assign, estim=2, result_type=rt, k=k), want,
                       (what, rt, t, min_pts, assign), small)
            if min_pts <= 2:  # the single-linkage components, byte for byte
                assert want[0].tobytes() == single[0].tobytes() and want[3] == single[1] - want[4]
                assert min_pts == 2 or ((want[1] == CORE).all() and want[4] == 0)
            if min_pts > n:
                assert want[4] == n and want[3] == 0
            assert (deg[want[1] != CORE].astype(np.int64) <= min_pts - 2).all()
    return col.size


@pytest.mark.parametrize("rt", [D.JI, D.MASH_DIST, D.CONTAINMENT_INDEX])
@pytest.mark.parametrize("shape", range(len(tri_shapes())))
def test_sketch_form_equals_the_model_over_the_hits(ctx, shape, rt):
    name, make, k = tri_shapes()[shape]
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    dense = ctx.dist_rows(estim=2, result_type=rt, k=k)
    for t in quantile_thresholds(dense, rt, n) + [float("nan")]:
        hits = check_hits(ctx, n, t, rt, k, (1, 2, 3, 5, n + 1), what=name)
        print("%s rt=%d t=%.9g: %d hits of %d" % (name, rt, t, hits, dense.size))


def test_long_rows_cross_chunks(ctx):
    """rows longer than one chunk of the band kernels (4096 values), starting at every alignment: the shape of
    tests/test_gpu_cluster.py::test_long_rows_cross_chunks.  The small band is 16 MiB here (ten bands of 40 million values)."""
    n, p = 9000, 8
    regs = synth.synthetic_sketches(n, p, seed=5)
    regs[4100] = regs[3]
    regs[8999] = regs[3]
    ctx.set_sketches(regs)
    dense = ctx.dist_rows(estim=2, result_type=D.JI, k=31)
    for t in quantile_thresholds(dense, D.JI, n)[2:4] + [1.0]:
        check_hits(ctx, n, t, D.JI, 31, (1, 3, 5), small=16 << 20, what="long rows")
    lab, kind, deg, nc, nn = ctx.dbscan_threshold(1.0, 3, estim=2, result_type=D.JI, k=31)
    assert lab[3] == lab[4100] == lab[8999] == 3 and (kind[[3, 4100, 8999]] == CORE).all() and (deg[[3, 4100, 8999]] >= 2).all()


# ---- against the CPU oracle --------------------------------------------------------------------------------------------
ORACLE_MIN_PTS = {
    # (case, hit fraction; 0 = 1 / n): (min_pts, cores, borders, noise) of the ORACLE's graph at the gap threshold; found on the
    # CPU with the oracle alone (choose_min_pts)
    (0, 0): (3, 122, 0, 178), (0, 0.01): (3, 181, 0, 119),
    (1, 0): (3, 122, 0, 178), (1, 0.01): (3, 181, 0, 119),
    (2, 0): (3, 280, 0, 420), (2, 0.01): (3, 576, 44, 80),
    (3, 0): (3, 280, 0, 420), (3, 0.01): (3, 587, 48, 65),
}


def oracle_graph(oracle, case, frac):
    name, make, rt, k, _ = thr_ref.oracle_cases()[case]
    regs = make()
    n = regs.shape[0]
    ov = np.asarray(oracle.dist_tri(regs, 2, rt, k), np.float64)
    sim = rt in thr_ref.SIMILARITY
    t, gap = gap_threshold(ov, frac if frac else 1.0 / n, sim)
    assert gap > 2e-6
    assert not thr_ref.undecided(ov, t).any()
    with np.errstate(invalid="ignore"):
        hit = (ov >= t) if sim else (ov <= t)
    i, j = np.triu_indices(n, 1)
    return regs, rt, k, sim, t, i[hit].astype(np.uint32), j[hit].astype(np.uint32), ov[hit]


def choose_min_pts(n, lhs, rhs, val, sim):
    """the first of 3, 4, 5, 8 with at least one core, one border and one noise point in the reference; where none has all
    three, the first of them"""
    tried = []
    for min_pts in (3, 4, 5, 8):
        counts = np.bincount(dbscan_ref.dbscan(n, lhs, rhs, val.astype(np.float32), min_pts, "first", sim)[1], minlength=3)
        tried.append((min_pts, int(counts[CORE]), int(counts[BORDER]), int(counts[NOISE])))
        if counts.min() > 0:
            return tried[-1]
    return tried[0]


def near_tied_borders(n, lhs, rhs, val, kind, sim):
    """the borders whose two best core neighbours have oracle values within 2e-6 relative: "best" may go either way on the GPU"""
    a, b = lhs.astype(np.int64), rhs.astype(np.int64)
    core = kind == CORE
    one = core[a] != core[b]
    bo = np.where(core[a[one]], b[one], a[one])
    rank = -val[one] if sim else val[one]
    order = np.lexsort((rank, bo))
    bo, v = bo[order], val[one][order]
    second = np.flatnonzero(np.concatenate([[True], bo[1:] != bo[:-1]])) + 1  # behind the first of every border's run ...
    second = second[second < bo.size]
    second = second[bo[second] == bo[second - 1]]                             # ... where the run goes on
    close = np.abs(v[second] - v[second - 1]) <= 2e-6 * np.maximum(np.abs(v[second - 1]), 1e-9)
    return np.unique(bo[second[close]])


@pytest.mark.parametrize("frac", [0, 0.01])
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_against_oracle(ctx, oracle, case, frac):
    """The four oracle cases at the gap thresholds of tests/test_gpu_cluster.py::test_against_oracle (hit fractions 1/n and 1 %,
    gaps from 3.5e-5 up, no undecided pair): both graphs are the same, so labels, kinds, degrees and counts are equal exactly.
    min_pts is chosen on the CPU with the oracle alone, the first of 3, 4, 5, 8 that leaves a core, a border and a noise point
    (cores / borders / noise of the reference):
      synthetic300p10 JI         1/n: min_pts 3, 122 / 0 / 178    1 %: min_pts 3, 181 / 0 / 119
      synthetic300p10 MASH_DIST  1/n: min_pts 3, 122 / 0 / 178    1 %: min_pts 3, 181 / 0 / 119
      related700p12   JI         1/n: min_pts 3, 280 / 0 / 420    1 %: min_pts 3, 576 / 44 / 80
      related700p12   MASH_DIST  1/n: min_pts 3, 280 / 0 / 420    1 %: min_pts 3, 587 / 48 / 65
    In six of the eight graphs the BORDER kind is absent under every one of the four (the hits form small cliques: a slot with
    a neighbour has enough of them); they are kept with the first candidate, 3, as cases of cores and noise.  The two 1 % graphs of related700p12 hold all three kinds.
    "first" is compared everywhere.  "best" is compared on every border whose two best core neighbours differ by more than 2e-6
    relative in the oracle; the others (under 0.5 % of the borders, asserted) are only held to be borders."""
    regs, rt, k, sim, t, lhs, rhs, val = oracle_graph(oracle, case, frac)
    n = regs.shape[0]
    min_pts, cores, borders, noise = choose_min_pts(n, lhs, rhs, val, sim)
    print("case %d frac %g: t = %.9g, min_pts %d, %d cores, %d borders, %d noise" % (case, frac, t, min_pts, cores, borders, noise))
    assert ORACLE_MIN_PTS[(case, frac)] == (min_pts, cores, borders, noise)
    ctx.set_sketches(regs)
    want = dbscan_ref.dbscan(n, lhs, rhs, val.astype(np.float32), min_pts, "first", sim)
    both_bands(ctx, lambda: ctx.dbscan_threshold(t, min_pts, "first", estim=2, result_type=rt, k=k), want, ("oracle first", case, frac))
    best = dbscan_ref.dbscan(n, lhs, rhs, val.astype(np.float32), min_pts, "best", sim)
    drop = near_tied_borders(n, lhs, rhs, val, want[1], sim)
    assert drop.size <= 0.005 * borders
    got = ctx.dbscan_threshold(t, min_pts, "best", estim=2, result_type=rt, k=k)
    keep = np.ones(n, bool)
    keep[drop] = False
    assert np.array_equal(got[0][keep], best[0][keep]) and (got[1][drop] == BORDER).all()
    assert np.array_equal(got[1], best[1]) and np.array_equal(got[2], best[2]) and got[3:] == best[3:]


# ---- the device form writes its n items per array and nothing else ---------------------------------------------------
@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
def test_device_form_between_guard_bands(ctx, misalign):
    import torch

    n, p = 700, 12
    regs = synth.related_sketches(n, p, seed=91)[0]
    ctx.set_sketches(regs)
    dev = torch.device("cuda:0")

    def bufs():
        return [guard.Guarded(n, dt, front=4096, back=4096, misalign=misalign, device=dev) for dt in (np.uint32, np.uint8, np.uint32)]

    for t, min_pts, assign in ((0.03, 5, "first"), (0.03, 40, "best"), (0.6, 3, "best"), (2.0, 1, "first")):
        want = ctx.dbscan_threshold(t, min_pts, assign, estim=2, result_type=D.JI, k=31)
        lab, kind, deg = bufs()
        got = ctx.dbscan_threshold_device(lab.ptr, t, min_pts, assign, kind_ptr=kind.ptr, degree_ptr=deg.ptr, estim=2, result_type=D.JI, k=31)
        for b in (lab, kind, deg):
            b.check("dbscan_threshold_device t=%g" % t)
            assert b.unwritten() == 0
        same((lab.host(), kind.host(), deg.host()) + got, want, ("device form", t, min_pts))
        # a NULL optional output is not written: each alone, with the other's buffer left out of the call
        for give_kind in (True, False):
            lab, kind, deg = bufs()
            got = ctx.dbscan_threshold_device(lab.ptr, t, min_pts, assign, kind_ptr=kind.ptr if give_kind else None,
                                              degree_ptr=None if give_kind else deg.ptr, estim=2, result_type=D.JI, k=31)
            for b in (lab, kind, deg):
                b.check("dbscan_threshold_device with a NULL output")
            assert lab.unwritten() == 0 and kind.unwritten() == (0 if give_kind else n) and deg.unwritten() == (n if give_kind else 0)
            assert np.array_equal(lab.host(), want[0]) and got == want[3:]
            assert np.array_equal(kind.host(), want[1]) if give_kind else np.array_equal(deg.host(), want[2])
        d = guard.Guarded(n, np.uint32, front=4096, back=4096, misalign=misalign, device=dev)
        ctx.degree_threshold_device(d.ptr, t, estim=2, result_type=D.JI, k=31)
        d.check("degree_threshold_device")
        assert d.unwritten() == 0 and np.array_equal(d.host(), want[2])
    assert want[4] == 0 and want[3] == n  # (t = 2, min_pts 1: nothing passes, every slot a cluster, and still all is written)


# ---- the context afterwards ------------------------------------------------------------------------------------------
def test_dense_and_pair_calls_around_a_dbscan_call(ctx):
    n, p = 3000, 12
    regs = synth.survey_sketches(n, p, seed=0x5EED0000)[0]
    ctx.set_sketches(regs)
    rng = np.random.default_rng(3)
    pl, pr = rng.integers(0, n, 500).astype(np.uint32), rng.integers(0, n, 500).astype(np.uint32)
    for rt, t in ((D.JI, 0.03), (D.MASH_DIST, 0.1)):
        desc = rt in thr_ref.SIMILARITY
        before = ctx.dist_rows(estim=2, result_type=rt, k=31)
        pairs = ctx.dist_pairs(pl, pr, (rt,), estim=2, k=31)
        rp, col, val = csr = ctx.dist_threshold(t, estim=2, result_type=rt, k=31)
        lhs, rhs = cluster_ref.csr_edges(rp, col)
        for band in (ONE_BAND, 1 << 20):
            try:
                ctx.set_option("threshold_band_bytes", band)
                a = ctx.dbscan_threshold(t, 40, "best", estim=2, result_type=rt, k=31)
                after = ctx.dist_rows(estim=2, result_type=rt, k=31)
                # another min_pts on the same context: its own answer, nothing stale in degree[] or best[]
                b = ctx.dbscan_threshold(t, 4, "first", estim=2, result_type=rt, k=31)
                c = ctx.dbscan_threshold(t, 40, "best", estim=2, result_type=rt, k=31)
            finally:
                ctx.set_option("threshold_band_bytes", ONE_BAND)
            assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
            same(a, dbscan_ref.dbscan(n, lhs, rhs, val, 40, "best", desc), ("min_pts 40", rt, band))
            same(b, dbscan_ref.dbscan(n, lhs, rhs, val, 4, "first", desc), ("min_pts 4", rt, band))
            same(c, a, ("min_pts 40 again", rt, band))
        assert np.array_equal(ctx.dist_pairs(pl, pr, (rt,), estim=2, k=31).view(np.uint32), pairs.view(np.uint32))
        assert thr_ref.same(ctx.dist_threshold(t, estim=2, result_type=rt, k=31), csr)
        sub = ctx.dist_rows(100, 900, estim=2, result_type=rt, k=31)  # a row range, a degree call, the range again
        assert np.array_equal(ctx.degree_threshold(t, estim=2, result_type=rt, k=31), a[2])
        assert np.array_equal(sub.view(np.uint32), ctx.dist_rows(100, 900, estim=2, result_type=rt, k=31).view(np.uint32))


# ---- error codes -----------------------------------------------------------------------------------------------------
def test_error_codes(ctx):
    def code(fn, *a, **kw):
        with pytest.raises(D.DshError) as e:
            fn(*a, **kw)
        return e.value.code

    lib = D.api.load_library()
    ctx.set_sketches(synth.synthetic_sketches(50, 10, seed=1))
    n = 50
    lab, kind, deg = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    nc, nn = ctypes.c_uint64(7), ctypes.c_uint64(7)
    raw = lambda fn, head, min_pts, mode, labels: fn(ctx._h, *head, 0.5, min_pts, mode, labels, kind.ctypes.data, deg.ctypes.data,
                                                     ctypes.byref(nc), ctypes.byref(nn))
    sk = (2, 1, 31)
    tri = np.zeros(n * (n - 1) // 2, np.float32)
    assert code(ctx.dbscan_threshold, 0.5, 0) == EINVAL  # min_pts counts the point itself: at least 1
    assert code(ctx.dbscan_tri, tri, True, 0.5, 0) == EINVAL
    for fn in (lib.dsh_dbscan_threshold, lib.dsh_dbscan_threshold_device):
        assert raw(fn, sk, 3, 2, lab.ctypes.data) == EINVAL   # an unknown assign_mode (the binding would refuse it first)
        assert raw(fn, sk, 3, -1, lab.ctypes.data) == EINVAL
        assert raw(fn, sk, 3, 0, None) == EINVAL              # NULL labels with n > 0
    assert raw(lib.dsh_dbscan_tri, (n, tri.ctypes.data, 1), 3, 5, lab.ctypes.data) == EINVAL
    assert raw(lib.dsh_dbscan_tri, (n, tri.ctypes.data, 1), 3, 0, None) == EINVAL
    assert raw(lib.dsh_dbscan_tri, (n, None, 1), 3, 0, lab.ctypes.data) == EINVAL  # no values for n >= 2
    assert raw(lib.dsh_dbscan_tri, (1 << 32, tri.ctypes.data, 1), 3, 0, lab.ctypes.data) == EINVAL  # labels are 32-bit
    assert lib.dsh_degree_threshold(ctx._h, 2, 1, 31, 0.5, None) == EINVAL
    assert lib.dsh_degree_threshold_device(ctx._h, 2, 1, 31, 0.5, None) == EINVAL
    # n = 0: OK with zero counts, no output needed
    assert raw(lib.dsh_dbscan_tri, (0, None, 1), 3, 0, None) == 0 and (nc.value, nn.value) == (0, 0)
    # after the refusals the context still answers
    same(ctx.dbscan_threshold(2.0, 1), (np.arange(n, dtype=np.uint32), np.full(n, CORE, np.uint8), np.zeros(n, np.uint32), n, 0), "after")
    # the sketch forms need sketches; the triangle form does not
    fresh = D.Context(0)
    try:
        assert code(fresh.dbscan_threshold, 0.5, 3) == ESTATE
        assert code(fresh.dbscan_threshold_device, 0, 0.5, 3) == ESTATE
        assert code(fresh.degree_threshold, 0.5) == ESTATE
        assert code(fresh.degree_threshold_device, 0, 0.5) == ESTATE
        got = fresh.dbscan_tri([1.0, 0.0, 1.0], True, 0.5, 3)
        assert got[0].tolist() == [1, 1, 1] and got[1].tolist() == [BORDER, CORE, BORDER] and got[2].tolist() == [1, 2, 1] and got[3:] == (1, 0)
    finally:
        fresh.close()
