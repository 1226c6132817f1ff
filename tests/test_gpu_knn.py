"""GPU: dsh_knn's three paths -- the n x n square, the bands of the key-ordered triangle, the blocks of queries -- against
the numpy model of the selection (tests/knn_ref.py).  For the measures that never see 1/k (JI, SIZES, CONTAINMENT_INDEX,
SYMMETRIC_CONTAINMENT_INDEX) the expected lists are the model's selection over the SAME context's dense rectangle, bit for
bit, indices and values; the distance forms (kNN uses the double 1/k, the dense calls the float) and the oracle go through
knn_ref.check_tolerant.  Whatever the path, two calls that answer the same question give the same bytes."""
import os

import numpy as np
import pytest

import knn_ref
from dashing_amd import synth
from test_gpu_fuzz import _regs

pytestmark = pytest.mark.gpu

EXACT = (1, 2, 5, 7)       # no 1/k: the kNN values are the dense path's bytes
DIST = (0, 3, 4, 6, 8)
DEFAULT_BUDGET = 96 << 30
TILE = 128


def _npad(n):
    return (n + TILE - 1) // TILE * TILE


def band_rows(n, budget):
    """knn.hip: band = min(Npad, max(min(budget, 16 GiB), 2 * 128 * Npad * 4) / (2 * Npad * 4) / 128 * 128)"""
    npad = _npad(n)
    b = max(min(budget, 16 << 30), 2 * TILE * npad * 4)
    return min(npad, b // (2 * npad * 4) // TILE * TILE)


def band_budget(n, rows):
    """the smallest budget that gives bands of `rows` rows (a multiple of 128)"""
    assert rows % TILE == 0 and rows > 0
    b = rows * 2 * _npad(n) * 4
    assert band_rows(n, b) == min(rows, _npad(n))
    return b


def knn_banded(ctx, budget, nn, **kw):
    """the all-vs-all call with the square switched off: bands of band_rows(n, budget) rows (query blocks for nn > 1024)"""
    ctx.set_option("knn_square_budget_bytes", budget)
    try:
        return ctx.knn(nn, **kw)
    finally:
        ctx.set_option("knn_square_budget_bytes", DEFAULT_BUDGET)


def knn_blocks(ctx, n, nn, **kw):
    """the all-vs-all question asked as two rectangles of queries (first half, second half) x all references: the
    query-block path, with self-exclusion, the second call starting at a row that is not 0"""
    h = n // 2
    if h == 0:
        return ctx.knn(nn, 0, n, 0, n, **kw)
    a = ctx.knn(nn, 0, h, 0, n, **kw)
    b = ctx.knn(nn, h, n, 0, n, **kw)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def all_paths(ctx, n, nn, budgets, **kw):
    out = [("square", ctx.knn(nn, **kw))]
    for b in budgets:
        out.append(("bands@%d" % band_rows(n, b), knn_banded(ctx, b, nn, **kw)))
    out.append(("blocks", knn_blocks(ctx, n, nn, **kw)))
    return out


def check_all_vs_all(ctx, n, nn, budgets, estim, rt, k, dense=None, note=()):
    """every path against the model over this context's dense rectangle, and against each other"""
    if dense is None:
        dense = ctx.dist_rect(0, n, 0, n, estim=estim, result_type=rt, k=k)
    got = all_paths(ctx, n, nn, budgets, estim=estim, result_type=rt, k=k)
    for name, g in got:
        assert g[0].shape == (n, nn) and g[1].shape == (n, nn)
        assert knn_ref.same(g, got[0][1]), (note, n, nn, estim, rt, k, name, "differs from the square path")
    if rt in EXACT:
        want = knn_ref.select(dense, nn, 0, 0, True, rt)
        assert knn_ref.same(want, got[0][1]), (note, n, nn, estim, rt, k, np.argwhere(want[0] != got[0][1][0])[:5])
    else:
        knn_ref.check_tolerant(dense.astype(np.float64), got[0][1][0], got[0][1][1], nn, 0, 0, True, rt)
    return dense


def budgets_for(n):
    """the smallest bands (128 rows), and 256-row bands where that is still more than one band"""
    return [0] + ([band_budget(n, 256)] if n > 256 else [])


def shape_regs(n, p, seed):
    regs = synth.synthetic_sketches(n, p, seed=seed)
    if n >= 30:  # exact ties, an empty sketch
        regs[7] = regs[8] = regs[9]
        regs[n - 1] = regs[n // 2]
        regs[20] = 0
    return regs


SHAPES = [(1, 10), (2, 10), (3, 10), (127, 10), (128, 10), (129, 10), (300, 10), (1300, 10), (260, 14), (40, 16), (33, 4)]
ALL_ESTIMATORS = ((129, 10), (260, 14), (33, 4))


def _nns(n):
    return sorted({1, min(9, max(n - 1, 1)), min(70, n + 2)})


@pytest.mark.parametrize("n,p", SHAPES)
def test_exact_measures_equal_the_model_on_all_paths(ctx, n, p):
    """1. bit for bit, no exclusions"""
    ctx.set_sketches(shape_regs(n, p, seed=100 + n))
    for estim in ((0, 1, 2) if (n, p) in ALL_ESTIMATORS else (2,)):
        for rt in EXACT:
            dense = None
            for nn in _nns(n):
                dense = check_all_vs_all(ctx, n, nn, budgets_for(n), estim, rt, 21, dense)


@pytest.mark.parametrize("n,p", SHAPES)
def test_distance_measures_against_the_dense_rectangle(ctx, n, p):
    """2. the dense rectangle uses the float 1/k: values within 1e-6, the order exact on the lists' own values, decided
    positions exact; the paths among themselves bit for bit"""
    ctx.set_sketches(shape_regs(n, p, seed=100 + n))
    for estim in ((0, 1, 2) if (n, p) in ALL_ESTIMATORS else (2,)):
        for rt in DIST:
            dense = None
            for nn in _nns(n):
                dense = check_all_vs_all(ctx, n, nn, budgets_for(n), estim, rt, 21, dense)


def test_mash_values_are_the_same_bits_on_all_three_paths(ctx):
    """All three paths go through the general instance of k_finalize with exact histograms and 1/k as a DOUBLE (PairJob's
    ksinv_double); only the layout differs.  A path that lost the switch would hand over the float and move a Mash distance
    by an ulp -- inside every tolerance above -- so each row's values are compared bit for bit across the paths.  (Indices
    may differ under ties.)  n = 300 is three tile rows, the last one partial, and three bands of 128 rows."""
    import dashing_amd

    n, p, nn = 300, 10, 5
    ctx.set_sketches(shape_regs(n, p, seed=100 + n))
    got = all_paths(ctx, n, nn, [0], result_type=dashing_amd.MASH_DIST, k=21)
    assert [name for name, _ in got] == ["square", "bands@128", "blocks"]
    want = got[0][1][1]
    assert want.shape == (n, nn) and want.dtype == np.float32
    for name, (_, val) in got[1:]:
        assert val.shape == (n, nn) and val.dtype == np.float32
        differ = np.argwhere(val.view(np.uint32) != want.view(np.uint32))
        assert differ.size == 0, (name, differ[:5])


# ---- 3. edges ----------------------------------------------------------------------------------------------------------
def test_nn_values_around_the_lanes_and_the_band_paths_limit(ctx):
    """nn around the 64 lanes that stride the running list in LDS, the two ends of the band path's range (1024 stays on the
    bands, 1025 falls back to query blocks), all neighbours, more than exist"""
    n, p = 1200, 10
    ctx.set_sketches(shape_regs(n, p, seed=12))
    assert band_rows(n, 0) == 128 and n % 128  # ten bands, the last one ragged
    for rt in (1, 0):
        dense = None
        for nn in (1, 2, 63, 64, 65, 127, 128, 1023, 1024, 1025, n - 1, n + 5):
            dense = check_all_vs_all(ctx, n, nn, [0], 2, rt, 21, dense)


@pytest.mark.parametrize("n", [1200, 1281, 1024, 515])
def test_band_sizes_with_a_ragged_last_band(ctx, n):
    """bands of 128, 256, 384 and 512 rows over n that is and is not a multiple of 128, and n just above one (Npad - n =
    127 padding columns).  CONTAINMENT_INDEX is asymmetric: V and Vt must each carry their own orientation."""
    ctx.set_sketches(shape_regs(n, 10, seed=n))
    for rt in (1, 5, 4):
        budgets = []
        for rows in (128, 256, 384, 512):
            b = band_budget(n, rows)
            if band_rows(n, b) < n:  # more than one band
                budgets.append(b)
        assert len(budgets) >= 3 and any(n % band_rows(n, b) for b in budgets)
        check_all_vs_all(ctx, n, 20, budgets, 2, rt, 31)
        knn_banded(ctx, budgets[0], 20, result_type=rt, k=31)
        assert ctx.info("npad") == _npad(n) and ctx.info("sorted") == 1  # the layout band_rows() assumed


def test_rectangles_partly_overlapping_empty_narrow(ctx):
    n, p = 400, 10
    ctx.set_sketches(shape_regs(n, p, seed=31))
    rects = [
        (100, 300, 200, 400),  # self left of the window (q < 200) and inside it
        (200, 400, 100, 300),  # self inside and right of the window
        (150, 250, 100, 300),  # the window holds every self
        (0, n, 1, n),          # row 0 has no self column
        (0, n, 0, n - 1),      # the last row has none
        (50, 60, 30, 30),      # no references
        (50, 60, 70, 40),      # r_begin > r_end: none either
        (0, 100, 95, 100),     # fewer references than nn, self among them for five rows
        (17, 18, 0, n),        # one query
        (0, n, 17, 18),        # one reference; query 17 has no candidate at all
        (399, 400, 399, 400),  # only itself
    ]
    for rt in (1, 5, 0, 4):
        for q0, q1, r0, r1 in rects:
            dense = ctx.dist_rect(q0, q1, r0, max(r0, r1), result_type=rt, k=21)
            assert dense.shape == (q1 - q0, max(r1 - r0, 0))
            for nn in (1, 9):
                got = ctx.knn(nn, q0, q1, r0, r1, result_type=rt, k=21)
                if rt in EXACT:
                    want = knn_ref.select(dense, nn, q0, r0, True, rt)
                    assert knn_ref.same(want, got), (rt, q0, q1, r0, r1, nn, np.argwhere(want[0] != got[0])[:5])
                else:
                    knn_ref.check_tolerant(dense.astype(np.float64), got[0], got[1], nn, q0, r0, True, rt)


def tied_regs(n, p, seed):
    """every fourth sketch empty, several duplicated: most of a row is exactly 0 / 1 / NaN"""
    regs = synth.synthetic_sketches(n, p, seed=seed, cluster=4)
    regs[::4] = 0
    for a, b in ((1, 901), (2, 902), (5, 3), (6, 3), (n - 1, 3), (450, 451), (10, 998)):
        regs[a] = regs[b]
    return regs


def test_rows_of_exact_ties_keep_the_slot_order(ctx):
    """nn = 200 reaches deep into the ties.  The band path sees its candidates in key order, band by band, in two
    orientations, and must rank them by ORIGINAL slot"""
    n, p = 1000, 10
    ctx.set_sketches(tied_regs(n, p, seed=77))
    for rt in (1, 0, 5, 7, 8):
        dense = check_all_vs_all(ctx, n, 200, [0, band_budget(n, 384)], 2, rt, 21)
        got = knn_banded(ctx, 0, 200, result_type=rt, k=21)
        assert ctx.info("sorted") == 1  # (that call ran on the key-ordered layout, not the identity)
        if rt == 1:
            frac = float(np.mean(dense == 0))
            assert frac > 0.4, frac  # the ties are there
            assert (np.diff(got[0][4].astype(np.int64)) > 0).all()  # an empty sketch's row: one value, slots ascending


def test_nan_and_infinity_through_the_bands(ctx):
    """two empty sketches (their containment measures are NaN, and so is SYMMETRIC_* of anything with them) and two
    saturated ones (MLE: +inf).  At nn = 150 a row's list is not full after its first band (at most 128 + its own band's
    candidates), so NaN candidates enter it early and are displaced by finite ones of later bands; at nn = n - 1 they
    stay; an empty sketch's own row is all NaN and must come out in slot order whatever band brought which."""
    n, p = 700, 10
    regs = synth.synthetic_sketches(n, p, seed=5)
    regs[3] = 0
    regs[n - 2] = 0
    regs[0] = 64 - p + 1
    regs[n // 2] = 64 - p + 1
    ctx.set_sketches(regs)
    assert band_rows(n, 0) == 128
    for estim in (2, 0):
        for rt in (5, 7, 1, 2, 8, 6):
            dense = None
            for nn in (3, 150, n - 1):
                dense = check_all_vs_all(ctx, n, nn, [0, band_budget(n, 256)], estim, rt, 21, dense)
            if rt == 7:
                assert np.isnan(dense[3]).all() and np.isnan(dense[:, 3]).all()
                gi, gv = knn_banded(ctx, 0, 150, estim=estim, result_type=rt, k=21)
                assert np.isnan(gv[3]).all() and gi[3].tolist() == [j for j in range(151) if j != 3]


# ---- 4. more than one query block ---------------------------------------------------------------------------------------
def test_two_query_blocks_at_their_real_size(ctx):
    """dsh_knn's rectangle path works in blocks of (256 << 20) / nr queries: a second block needs nq * nr > 2^28.  17 000
    queries x 16 999 references are two blocks (15 791 + 1 209 queries): the second block's output offset and the row0 its
    self-exclusion starts from are exercised here and nowhere else.  The reference is taken in slices of 2 000 queries, so
    the host never holds the 1.1 GB rectangle.  nn = 3 is the prefix of nn = 70 in the model (tests/test_knn_ref.py,
    test_select_prefix_property_and_same), so one sort per slice serves both."""
    n, p = 17_000, 4
    rng = np.random.default_rng(17)
    regs = rng.integers(0, 12, size=(n, 1 << p)).astype(np.uint8)
    regs[rng.choice(n, 400, replace=False)] = 0
    dup = rng.choice(n, (300, 2), replace=False)
    regs[dup[:, 0]] = regs[dup[:, 1]]
    regs[15_900] = regs[15_700]  # a tie across the block boundary, a row right behind it
    nr = n - 1
    qblock = (256 << 20) // nr
    print("query block = %d rows, blocks = %d" % (qblock, -(-n // qblock)))
    assert qblock == 15_791 and -(-n // qblock) >= 2
    ctx.set_sketches(regs)
    g70 = ctx.knn(70, 0, n, 1, n, result_type=1, k=21)
    g3 = ctx.knn(3, 0, n, 1, n, result_type=1, k=21)
    for q0 in range(0, n, 2000):
        q1 = min(n, q0 + 2000)
        dense = ctx.dist_rect(q0, q1, 1, n, result_type=1, k=21)
        want = knn_ref.select(dense, 70, q0, 1, True, 1)
        assert knn_ref.same(want, (g70[0][q0:q1], g70[1][q0:q1])), (q0, np.argwhere(want[0] != g70[0][q0:q1])[:5])
        assert knn_ref.same((want[0][:, :3].copy(), want[1][:, :3].copy()), (g3[0][q0:q1], g3[1][q0:q1])), q0


# ---- 5. against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", knn_ref.oracle_cases(), ids=lambda c: "%s-rt%d-nn%d" % (c[0], c[2], c[4]))
def test_square_and_bands_against_the_oracle(ctx, oracle, case):
    name, _, rt, k, nn = case
    regs, ref = knn_ref.oracle_rect(oracle, case)
    n = regs.shape[0]
    ctx.set_sketches(regs)
    for path, got in (("square", ctx.knn(nn, result_type=rt, k=k)), ("bands", knn_banded(ctx, 0, nn, result_type=rt, k=k))):
        und, pos = knn_ref.check_tolerant(ref, got[0], got[1], nn, 0, 0, True, rt)
        print("%s rt=%d nn=%d %s: %d of %d list positions undecided (%.3g), %d decided and equal to the oracle's" %
              (name, rt, nn, path, und, pos, und / pos, pos - und))
        assert pos == n * nn and pos - und >= 1
        assert und / pos <= knn_ref.UNDECIDED_CAP


# ---- 6. seeded fuzz ---------------------------------------------------------------------------------------------------------
_FIRST = int(os.environ.get("DSH_KNN_FIRST", "0"))  # e.g. DSH_KNN_FIRST=200 DSH_KNN_CASES=2000 for a soak on fresh seeds


@pytest.mark.parametrize("case", range(_FIRST, _FIRST + int(os.environ.get("DSH_KNN_CASES", "200"))))
def test_random_knn_case(ctx, case):
    rng = np.random.default_rng(52_000 + case)
    p = int(rng.integers(4, 17))
    n = int(rng.integers(1, 600 if p <= 12 else 150))
    kind = str(rng.choice(["law", "related", "uniform", "narrow"]))
    estim = int(rng.integers(0, 3))
    rt = int(rng.integers(0, 9))
    k = int(rng.choice([15, 21, 31, 32]))
    regs = _regs(rng, n, p, kind)
    planted = int(rng.integers(0, 4)) if n > 4 else 0
    for _ in range(planted):  # duplicates, empties, saturated rows
        a, b = rng.choice(n, 2, replace=False)
        regs[a] = regs[b]
        regs[int(rng.integers(n))] = 0
        if rng.random() < 0.5:
            regs[int(rng.integers(n))] = 64 - p + 1
    if n > 8 and rng.random() < 0.25:  # mostly ties
        regs[rng.random(n) < 0.5] = 0
    nn = int(rng.choice([1, int(rng.integers(1, 9)), int(rng.integers(1, 130)), int(rng.integers(1, n + 4))]))
    whole = bool(rng.random() < 0.5)
    q0 = int(rng.integers(0, n)); q1 = int(rng.integers(q0 + 1, n + 1))
    r0 = int(rng.integers(0, n)); r1 = int(rng.integers(r0, n + 1))
    budget = int(rng.choice([0, band_budget(n, 128 * int(rng.integers(1, 5)))]))
    recipe = "case=%d p=%d n=%d kind=%s planted=%d estim=%d rt=%d k=%d nn=%d %s budget=%d" % (
        case, p, n, kind, planted, estim, rt, k, nn, "all-vs-all" if whole else "q=[%d,%d) r=[%d,%d)" % (q0, q1, r0, r1), budget)
    try:
        ctx.set_sketches(regs)
        if whole:
            check_all_vs_all(ctx, n, nn, [budget], estim, rt, k)
        else:
            dense = ctx.dist_rect(q0, q1, r0, r1, estim=estim, result_type=rt, k=k)
            got = ctx.knn(nn, q0, q1, r0, r1, estim=estim, result_type=rt, k=k)
            if rt in EXACT:
                assert knn_ref.same(knn_ref.select(dense, nn, q0, r0, True, rt), got)
            else:
                knn_ref.check_tolerant(dense.astype(np.float64), got[0], got[1], nn, q0, r0, True, rt)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (recipe, e)) from e
