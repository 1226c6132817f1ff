"""CPU: tests/knn_ref.py -- the numpy model of dsh_knn's selection -- by hand-written cases and against oracle.knn; the
undecided share of every oracle case the GPU test takes (on the oracle alone); and that check_tolerant rejects wrong lists."""
import numpy as np
import pytest

import knn_ref
from dashing_amd import synth

F = knn_ref.FILL
inf, nan = np.inf, np.nan


def _sel(dense, nn, rt=1, q_begin=0, r_begin=0, exclude_self=False):
    i, v = knn_ref.select(np.array(dense, np.float32), nn, q_begin, r_begin, exclude_self, rt)
    return i.tolist(), v.tolist()


def _eq(got, want):  # lists with NaN
    return np.array_equal(np.array(got, np.float64), np.array(want, np.float64), equal_nan=True)


def test_descending_is_the_rule_of_the_similarity_forms():
    assert [knn_ref.descending(rt) for rt in range(9)] == [False, True, True, False, False, True, False, True, False]
    with pytest.raises(AssertionError):
        knn_ref.descending(9)


def test_select_ties_go_to_the_lower_slot():
    i, v = _sel([[0.5, 0.7, 0.5, 0.7, 0.5]], 4, rt=1)
    assert i == [[1, 3, 0, 2]] and v == [[np.float32(0.7)] * 2 + [0.5] * 2]
    i, v = _sel([[0.5, 0.7, 0.5, 0.7, 0.5]], 4, rt=0)
    assert i == [[0, 2, 4, 1]]
    i, v = _sel([[0.0, -0.0, 0.0]], 3, rt=0)  # the two zeros are one value
    assert i == [[0, 1, 2]]


def test_select_nan_ranks_last_and_is_reported():
    i, v = _sel([[nan, 0.2, nan, 0.9]], 4, rt=1)
    assert i == [[3, 1, 0, 2]] and _eq(v, [[np.float32(0.9), np.float32(0.2), nan, nan]])
    i, v = _sel([[nan, 0.2, nan, 0.9]], 3, rt=0)
    assert i == [[1, 3, 0]] and _eq(v, [[np.float32(0.2), np.float32(0.9), nan]])
    i, v = _sel([[nan, nan, nan]], 2, rt=7)  # a row of only NaN
    assert i == [[0, 1]] and _eq(v, [[nan, nan]])


def test_select_infinities_are_values_and_tie_with_nan_by_slot():
    # distances: +inf is the worst real value, it ties with NaN (lower slot first); -inf is the best
    i, v = _sel([[nan, inf, 1.0, -inf, inf]], 7, rt=0)
    assert i == [[3, 2, 0, 1, 4, F, F]] and _eq(v, [[-inf, 1.0, nan, inf, inf, inf, inf]])
    # similarities: the mirror image
    i, v = _sel([[-inf, nan, 1.0, inf]], 5, rt=1)
    assert i == [[3, 2, 0, 1, F]] and _eq(v, [[inf, 1.0, -inf, nan, -inf]])


def test_select_fewer_candidates_than_nn_none_and_no_neighbours_asked():
    i, v = _sel([[0.1, 0.3]], 4, rt=1)
    assert i == [[1, 0, F, F]] and v[0][2:] == [-inf, -inf]
    i, v = _sel([[0.1, 0.3]], 4, rt=0, exclude_self=True, q_begin=1)
    assert i == [[0, F, F, F]] and v[0][1:] == [inf, inf, inf]
    i, v = knn_ref.select(np.zeros((3, 5), np.float32), 0, 0, 0, True, 1)
    assert i.shape == (3, 0) and v.shape == (3, 0) and i.dtype == np.uint32 and v.dtype == np.float32
    i, v = knn_ref.select(np.zeros((3, 0), np.float32), 2, 0, 0, True, 1)  # no references
    assert (i == F).all() and (v == -inf).all() and i.shape == (3, 2)
    i, v = knn_ref.select(np.zeros((3, 0), np.float32), 2, 0, 0, True, 8)
    assert (i == F).all() and (v == inf).all()


def test_select_self_inside_left_and_right_of_the_window():
    d = [[0.9, 0.8, 0.7, 0.6]] * 3
    # queries 4..6, references 5..8: query 4 lies left of the window, 5 and 6 inside
    i, _ = _sel(d, 4, rt=1, q_begin=4, r_begin=5, exclude_self=True)
    assert i == [[5, 6, 7, 8], [6, 7, 8, F], [5, 7, 8, F]]
    # queries 8..10, references 5..8: 8 is the last column, 9 and 10 lie right of the window
    i, _ = _sel(d, 4, rt=1, q_begin=8, r_begin=5, exclude_self=True)
    assert i == [[5, 6, 7, F], [5, 6, 7, 8], [5, 6, 7, 8]]
    # not excluded: the same slots are ordinary candidates
    i, _ = _sel(d, 4, rt=1, q_begin=4, r_begin=5, exclude_self=False)
    assert i == [[5, 6, 7, 8]] * 3


def test_select_prefix_property_and_same():
    rng = np.random.default_rng(3)
    d = rng.integers(0, 6, size=(40, 50)).astype(np.float32)  # mostly ties
    d[rng.random(d.shape) < 0.1] = nan
    for rt in (1, 0):
        big = knn_ref.select(d, 49, 0, 0, True, rt)
        for nn in (1, 7, 30):
            small = knn_ref.select(d, nn, 0, 0, True, rt)
            assert knn_ref.same(small, (big[0][:, :nn], big[1][:, :nn]))
    a = knn_ref.select(d, 5, 0, 0, True, 1)
    b = (a[0].copy(), a[1].copy())
    assert knn_ref.same(a, b)
    b[1][0, 0] = -b[1][0, 0] if b[1][0, 0] == 0 else np.nextafter(b[1][0, 0], np.float32(9))
    assert not knn_ref.same(a, b)
    assert not knn_ref.same((a[0].astype(np.int64), a[1]), a)


def _small(seed, n=64, p=8):
    regs = synth.synthetic_sketches(n, p, seed=seed)
    regs[3] = regs[11] = regs[12]     # exact ties
    regs[40] = regs[2]
    regs[5] = 0                       # empty: containment NaN
    regs[30] = 0
    regs[17] = 64 - p + 1             # saturated: MLE +inf
    regs[50] = 64 - p + 1
    return regs


@pytest.mark.parametrize("estim", [0, 1, 2])
@pytest.mark.parametrize("seed", [1, 2])
def test_select_on_the_oracles_rectangle_is_the_oracles_knn(oracle, estim, seed):
    regs = _small(seed)
    n = regs.shape[0]
    for rt in range(9):
        d32 = oracle.dist_rect(regs, regs, estim, rt, 21)
        dknn = oracle.dist_rect(regs, regs, estim, rt, 21, ksinv_double=True)  # the values dsho_knn reports
        for nn in (1, 9, n + 3):
            wi, wv = oracle.knn(regs, nn, estim=estim, result_type=rt, k=21)
            assert knn_ref.same(knn_ref.select(dknn, nn, 0, 0, True, rt), (wi, wv)), (rt, nn)
            if rt in (1, 2, 5, 7):  # no 1/k in these: the plain rectangle is the same bytes
                assert knn_ref.same(knn_ref.select(d32, nn, 0, 0, True, rt), (wi, wv)), (rt, nn)
            # the oracle's own lists pass the tolerant check against either rectangle
            knn_ref.check_tolerant(d32.astype(np.float64), wi, wv, nn, 0, 0, True, rt)
            und, pos = knn_ref.check_tolerant(dknn.astype(np.float64), wi, wv, nn, 0, 0, True, rt)
            assert pos == n * min(nn, n - 1)
        # a rectangle that overlaps the queries in part, and one that does not
        for qb, qe, rb, re in ((10, 40, 25, 60), (40, 64, 0, 30), (0, 20, 1, 64)):
            wi, wv = oracle.knn(regs, 6, qb=qb, qe=qe, rb=rb, re=re, estim=estim, result_type=rt, k=21)
            d = oracle.dist_rect(regs[qb:qe], regs[rb:re], estim, rt, 21, ksinv_double=True)
            assert knn_ref.same(knn_ref.select(d, 6, qb, rb, True, rt), (wi, wv)), (rt, qb, qe, rb, re)
            knn_ref.check_tolerant(d.astype(np.float64), wi, wv, 6, qb, rb, True, rt)


@pytest.mark.parametrize("case", knn_ref.oracle_cases(), ids=lambda c: "%s-rt%d-nn%d" % (c[0], c[2], c[4]))
def test_oracle_cases_stay_under_the_undecided_cap(oracle, case):
    """the share of list positions the GPU may legitimately fill otherwise, measured on the ORACLE's own lists"""
    name, make_regs, rt, k, nn = case
    regs, ref = knn_ref.oracle_rect(oracle, case)
    got = knn_ref.select(ref.astype(np.float32), nn, 0, 0, True, rt)
    und, pos = knn_ref.check_tolerant(ref, got[0], got[1], nn, 0, 0, True, rt)
    print("%s rt=%d nn=%d: %d of %d list positions undecided, share %.3g" % (name, rt, nn, und, pos, und / pos))
    assert pos == regs.shape[0] * nn and und < pos
    assert und / pos <= knn_ref.UNDECIDED_CAP


def _teeth_case():
    rng = np.random.default_rng(11)
    ref = rng.random((6, 30))  # distinct, far apart relative to 2e-6
    nn, qb, rb = 5, 2, 0
    gi, gv = knn_ref.select(ref.astype(np.float32), nn, qb, rb, True, 1)
    return ref, gi, gv, nn, qb, rb


def _rejects(ref, gi, gv, nn, qb, rb, rt=1):
    with pytest.raises(AssertionError):
        knn_ref.check_tolerant(ref, gi, gv, nn, qb, rb, True, rt)


def test_check_tolerant_accepts_the_model_and_rejects_wrong_lists():
    ref, gi, gv, nn, qb, rb = _teeth_case()
    assert knn_ref.check_tolerant(ref, gi, gv, nn, qb, rb, True, 1) == (0, 30)
    # two decided entries swapped
    i, v = gi.copy(), gv.copy()
    i[1, [2, 3]] = i[1, [3, 2]]
    v[1, [2, 3]] = v[1, [3, 2]]
    _rejects(ref, i, v, nn, qb, rb)
    # a better candidate left out: the best one replaced by the first one not taken
    full = knn_ref.select(ref.astype(np.float32), nn + 1, qb, rb, True, 1)
    i, v = full[0][:, 1:].copy(), full[1][:, 1:].copy()
    _rejects(ref, i, v, nn, qb, rb)
    # self included (in the place its value earns)
    si, sv = knn_ref.select(ref.astype(np.float32), nn, qb, rb, False, 1)
    ref2 = ref.copy()
    ref2[3, 5] = 2.0  # query 3 is slot 5: its own column is the best of the row
    si, sv = knn_ref.select(ref2.astype(np.float32), nn, qb, rb, False, 1)
    assert si[3, 0] == 5
    _rejects(ref2, si, sv, nn, qb, rb)
    # a duplicate
    i, v = gi.copy(), gv.copy()
    i[4, 3], v[4, 3] = i[4, 2], v[4, 2]
    _rejects(ref, i, v, nn, qb, rb)
    # wrong fillers: the index, the value, and a filler in front of a real entry
    few = ref[:, :4]
    fi, fv = knn_ref.select(few.astype(np.float32), nn, qb, rb, True, 1)
    assert (fi[0] == [*fi[0, :3], F, F]).all()
    knn_ref.check_tolerant(few, fi, fv, nn, qb, rb, True, 1)
    i, v = fi.copy(), fv.copy()
    i[0, 4] = 0
    _rejects(few, i, v, nn, qb, rb)
    i, v = fi.copy(), fv.copy()
    v[0, 4] = inf  # similarities fill with -inf
    _rejects(few, i, v, nn, qb, rb)
    i, v = fi.copy(), fv.copy()
    v[0, 4] = nan
    _rejects(few, i, v, nn, qb, rb)
    i, v = fi.copy(), fv.copy()
    i[0, 0], v[0, 0] = F, -inf
    _rejects(few, i, v, nn, qb, rb)
    # a value off by more than 1e-6 relative, an index out of range, NaN where the reference is finite
    i, v = gi.copy(), gv.copy()
    v[2, 0] *= np.float32(1 + 4e-6)
    _rejects(ref, i, v, nn, qb, rb)
    i, v = gi.copy(), gv.copy()
    i[2, 4] = 30
    _rejects(ref, i, v, nn, qb, rb)
    i, v = gi.copy(), gv.copy()
    v[2, 4] = nan
    _rejects(ref, i, v, nn, qb, rb)


def test_check_tolerant_undecided_positions():
    # row 0: .9 | two values 1e-7 apart (undecided, either order passes) | .5 .5 exact tie (decided by slot) | .1
    ref = np.array([[0.1, 0.5, 0.7, 0.5, 0.7 * (1 + 1e-7), 0.9]])
    f32 = ref.astype(np.float32)
    for order in ([5, 4, 2, 1, 3], [5, 2, 4, 1, 3]):
        gi = np.array([order], np.uint32)
        gv = f32[:, order].copy()
        gv[0, 1:3] = np.sort(gv[0, 1:3])[::-1]  # (the list's own values must still be sorted)
        assert knn_ref.check_tolerant(ref, gi, gv, 5, 9, 0, True, 1) == (2, 5)
    gi = np.array([[5, 4, 2, 3, 1]], np.uint32)  # the exact tie against the slot order
    _rejects(ref, gi, f32[:, [5, 4, 2, 3, 1]].copy(), 5, 9, 0)
    # the class |v| < 1e-9 of the measures that jump at 0: undecided for JI, decided by slot for a distance
    z = np.array([[0.3, 0.0, 1e-14, 0.0, 0.2]])
    gi = np.array([[0, 4, 2, 1]], np.uint32)
    gv = np.array([[0.3, 0.2, 1e-14, 0.0]], np.float32)
    assert knn_ref.check_tolerant(z, gi, gv, 4, 9, 0, True, 1) == (2, 4)
    gi = np.array([[1, 3, 2, 4]], np.uint32)
    gv = np.array([[0.0, 0.0, 1e-14, 0.2]], np.float32)
    assert knn_ref.check_tolerant(z, gi, gv, 4, 9, 0, True, 0) == (0, 4)  # (2e-6 of the 1e-9 floor is 2e-15)
    gi = np.array([[3, 1, 2, 4]], np.uint32)
    _rejects(z, gi, gv, 4, 9, 0, rt=0)
