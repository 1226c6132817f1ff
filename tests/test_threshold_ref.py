"""CPU: the numpy reference of the thresholded output (tests/thr_ref.py) on hand-made cases, and the oracle-side
precondition of the GPU comparison with the oracle: for every (collection, measure, t) that test uses, the pairs whose
oracle value lies within 2e-6 relative of t are at most 1e-5 of the case's pairs."""
import numpy as np
import pytest

import thr_ref

JI, MASH = 1, 0
NAN = np.float32("nan")


def test_ties_pass_in_both_directions():
    span = np.array([0.5, 0.25, 0.5, 0.75, 0.5, 0.125], np.float32)  # n = 4: rows of 3, 2, 1, 0 values
    rp, col, val = thr_ref.tri(span, 4, 0, 4, 0.5, JI)
    assert rp.tolist() == [0, 2, 4, 4, 4] and col.tolist() == [1, 3, 2, 3] and val.tolist() == [0.5, 0.5, 0.75, 0.5]
    rp, col, val = thr_ref.tri(span, 4, 0, 4, 0.5, MASH)
    assert rp.tolist() == [0, 3, 4, 5, 5] and col.tolist() == [1, 2, 3, 3, 3] and val.tolist() == [0.5, 0.25, 0.5, 0.5, 0.125]
    assert rp.dtype == np.uint64 and col.dtype == np.uint32 and val.dtype == np.float32


def test_threshold_is_compared_as_float32():
    v = np.array([np.float32(0.1)], np.float32)
    assert thr_ref.tri(v, 2, 0, 2, 0.1, JI)[0].tolist() == [0, 1, 1]   # float32(0.1) >= float32(0.1), though > 0.1 as double
    assert thr_ref.tri(v, 2, 0, 2, 0.1, MASH)[0].tolist() == [0, 1, 1]


def test_nan_never_passes():
    span = np.array([NAN, 1.0, NAN], np.float32)
    for rt in (JI, MASH, 2, 5, 6, 7, 8, 3, 4):
        rp, col, val = thr_ref.tri(span, 3, 0, 3, 1.0, rt)
        assert rp.tolist() == [0, 1, 1, 1] and col.tolist() == [2] and val.tolist() == [1.0]
    assert thr_ref.tri(span, 3, 0, 3, NAN, JI)[1].size == 0


def test_empty_rows_last_row_and_sub_ranges():
    n = 5
    span = np.arange(10, dtype=np.float32)  # rows: [0 1 2 3] [4 5 6] [7 8] [9] []
    rp, col, val = thr_ref.tri(span, n, 0, n, 100.0, JI)
    assert rp.tolist() == [0] * 6 and col.size == 0 and val.size == 0
    rp, col, val = thr_ref.tri(span, n, 0, n, -1.0, JI)  # everything passes: the dense result in CSR form
    assert rp.tolist() == [0, 4, 7, 9, 10, 10] and col.tolist() == [1, 2, 3, 4, 2, 3, 4, 3, 4, 4] and (val == span).all()
    rp, col, val = thr_ref.tri(span[4:9], n, 1, 3, 5.0, JI)
    assert rp.tolist() == [0, 2, 4] and col.tolist() == [3, 4, 3, 4] and val.tolist() == [5.0, 6.0, 7.0, 8.0]
    rp, col, val = thr_ref.tri(span[10:], n, 4, 5, 0.0, JI)  # the last row has no values
    assert rp.tolist() == [0, 0] and col.size == 0
    rp, col, val = thr_ref.tri(span[:0], n, 3, 3, 0.0, JI)  # empty range
    assert rp.tolist() == [0]
    rp, col, val = thr_ref.tri(span[9:], n, 3, 99, 9.0, JI)  # row_end beyond n is cut
    assert rp.tolist() == [0, 1, 1] and col.tolist() == [4]


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_collections(n):
    span = np.ones(n * (n - 1) // 2 if n else 0, np.float32)
    rp, col, val = thr_ref.tri(span, n, 0, n, 1.0, JI)
    assert rp.tolist() == ([0] if n == 0 else [0, 0] if n == 1 else [0, 1, 1])
    assert col.tolist() == ([1] if n == 2 else [])


def test_rect():
    d = np.array([[0.1, 0.9, NAN], [0.9, 0.9, 0.0], [0.0, 0.0, 0.0]], np.float32)
    rp, col, val = thr_ref.rect(d, 10, 0.9, JI)
    assert rp.tolist() == [0, 1, 3, 3] and col.tolist() == [11, 10, 11] and (val == np.float32(0.9)).all()
    rp, col, val = thr_ref.rect(d, 10, 0.1, MASH)
    assert rp.tolist() == [0, 1, 2, 5] and col.tolist() == [10, 12, 10, 11, 12]
    rp, col, val = thr_ref.rect(np.zeros((0, 4), np.float32), 0, 0.0, JI)
    assert rp.tolist() == [0] and col.size == 0
    rp, col, val = thr_ref.rect(np.zeros((2, 0), np.float32), 0, 0.0, JI)
    assert rp.tolist() == [0, 0, 0]


def test_same_compares_bits():
    a = (np.array([0, 1], np.uint64), np.array([1], np.uint32), np.array([0.0], np.float32))
    b = (np.array([0, 1], np.uint64), np.array([1], np.uint32), np.array([-0.0], np.float32))
    assert thr_ref.same(a, a) and not thr_ref.same(a, b)


def test_direction_sets_cover_every_measure():
    assert thr_ref.SIMILARITY | thr_ref.DISTANCE == set(range(9)) and not (thr_ref.SIMILARITY & thr_ref.DISTANCE)


@pytest.mark.parametrize("case", range(len(thr_ref.oracle_cases())))
def test_oracle_undecided_share_is_inside_the_cap(oracle, case):
    name, make, rt, k, ts = thr_ref.oracle_cases()[case]
    v = oracle.dist_tri(make(), 2, rt, k)
    for t in ts:
        und = int(thr_ref.undecided(v, t).sum())
        hits = int(thr_ref.passes(v, t, rt).sum())
        print("%s rt=%d k=%d t=%g: %d hits, %d undecided of %d" % (name, rt, k, t, hits, und, v.size))
        assert und <= thr_ref.UNDECIDED_CAP * v.size
        assert 0 < hits < v.size  # a threshold that selects something and not everything
