"""The two references of dsh_greedy_extend* (tests/greedy_extend_ref.py) held to each other, to tests/greedy_ref.py and to
the consequences the header states, on random graphs with random float32 values: exact ties, both zeros, NaN, and
labellings of the old slots that no full call would have produced."""
import numpy as np
import pytest

import greedy_extend_ref as X
import greedy_ref

CASES = [(n, dens, sim, seed) for seed in range(3) for n, dens in ((1, 0.5), (2, 0.5), (30, 0.1), (90, 0.05), (90, 0.5), (200, 0.02), (200, 0.2))
         for sim in (True, False)]


def random_values(n, dens, sim, rng):
    """float32 [n, n] and a threshold about `dens` of the pairs pass: values from a SMALL set (many exact ties), with both
    zeros, a few NaN, and the threshold itself among them"""
    levels = np.array([-0.0, 0.0, 0.125, 0.25, 0.25000003, 0.5, 0.75, 1.0], np.float32)
    v = levels[rng.integers(0, levels.size, (n, n))]
    v[rng.random((n, n)) < 0.02] = np.nan
    fine = rng.random((n, n)).astype(np.float32)  # and some values without ties
    v = np.where(rng.random((n, n)) < 0.3, fine, v).astype(np.float32)
    finite = np.sort(v[np.isfinite(v)])
    t = finite[min(int((1 - dens if sim else dens) * finite.size), finite.size - 1)] if finite.size else np.float32(0.5)
    return v, np.float32(t)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_two_statements_agree_and_the_consequences_hold(case):
    n, dens, sim, seed = CASES[case]
    rng = np.random.default_rng(0xE47E + 97 * case)
    v, t = random_values(n, dens, sim, rng)
    rp, col, val = X.csr_of_values(n, v, t, sim)
    full = {}
    for mode in (X.FIRST, X.BEST):
        lab, nr = X.labels(n, rp, col, val, 0, None, mode, sim)
        want, wr = X.labels_from_definition(n, v, t, 0, None, mode, sim)
        assert lab.dtype == np.uint32 and np.array_equal(lab, want) and nr == wr, (n, mode)
        X.check_consequences(n, v, t, 0, None, lab, mode, sim, (n, mode))
        full[mode] = lab
    # first_new == 0 with FIRST is the greedy pass of dsh_greedy_threshold
    old, onr = greedy_ref.labels(n, rp, col)
    assert np.array_equal(full[X.FIRST], old) and onr == int((full[X.FIRST] == np.arange(n)).sum())
    # BEST and FIRST have the same representatives
    assert np.array_equal(full[X.FIRST] == np.arange(n), full[X.BEST] == np.arange(n))
    for m in sorted({0, 1, n // 3, n // 2, max(n - 1, 0), n}):
        if m > n:
            continue
        arbitrary = [X.random_labelling(m, rng), np.arange(m, dtype=np.uint32), np.zeros(m, np.uint32)]
        for mode in (X.FIRST, X.BEST):
            # the prefix of a full call in the same mode gives the full call
            lab, nr = X.labels(n, rp, col, val, m, full[mode][:m] if m else None, mode, sim)
            assert np.array_equal(lab, full[mode]) and nr == int((lab == np.arange(n)).sum()), (n, m, mode)
            for q, li in enumerate(arbitrary):
                lab, nr = X.labels(n, rp, col, val, m, li if m else None, mode, sim)
                want, wr = X.labels_from_definition(n, v, t, m, li if m else None, mode, sim)
                assert np.array_equal(lab, want) and nr == wr, (n, m, mode, q)
                fast, fr = X.labels_fast(n, rp, col, val, m, li if m else None, mode, sim)
                assert fast.dtype == np.uint32 and np.array_equal(fast, want) and fr == wr, (n, m, mode, q)
                X.check_consequences(n, v, t, m, li, lab, mode, sim, (n, m, mode, q))
                if m == n:  # a copy and a count
                    assert np.array_equal(lab, li) and nr == int((li == np.arange(n)).sum())
        # (the dense form of the CSR: the values that do not pass play no part)
        fill = np.float32(-1.0) if sim else np.float32(9.0)
        if np.isfinite(t) and (t > fill if sim else t < fill):
            dv = X.dense_of_csr(n, rp, col, val, fill)
            for mode in (X.FIRST, X.BEST):
                assert np.array_equal(X.labels_from_definition(n, dv, t, m, arbitrary[0] if m else None, mode, sim)[0],
                                      X.labels(n, rp, col, val, m, arbitrary[0] if m else None, mode, sim)[0])


def test_ties_zeros_and_the_difference_between_the_modes():
    # 0, 1, 2 are representatives; 3 is hit by all three: 0 with 0.5, 1 and 2 with 0.75 -> FIRST 0, BEST 1 (tie to the smaller)
    v = np.full((4, 4), -1.0, np.float32)
    v[0, 3], v[1, 3], v[2, 3] = 0.5, 0.75, 0.75
    for stmt in (lambda mode, sim, t, vv: X.labels_from_definition(4, vv, t, 0, None, mode, sim)[0].tolist(),
                 lambda mode, sim, t, vv: X.labels(4, *X.csr_of_values(4, vv, t, sim), 0, None, mode, sim)[0].tolist()):
        assert stmt(X.FIRST, True, 0.5, v) == [0, 1, 2, 0]
        assert stmt(X.BEST, True, 0.5, v) == [0, 1, 2, 1]
        # distances: -0.0 and +0.0 are the same value, so the smaller slot keeps the column; 0.25 is worse
        d = np.full((4, 4), 9.0, np.float32)
        d[0, 3], d[1, 3], d[2, 3] = 0.25, 0.0, -0.0
        assert stmt(X.FIRST, False, 0.5, d) == [0, 1, 2, 0]
        assert stmt(X.BEST, False, 0.5, d) == [0, 1, 2, 1]
        d[1, 3], d[2, 3] = -0.0, 0.0
        assert stmt(X.BEST, False, 0.5, d) == [0, 1, 2, 1]
        # a NaN threshold: nothing passes
        assert stmt(X.BEST, True, np.nan, v) == [0, 1, 2, 3]


def test_old_slots_are_taken_as_given():
    # 0 hits 1 and 2, but the caller says 1 is a representative of its own and 0's cluster is {0}: 2 (new) goes to 0 in FIRST
    # and to 1 in BEST where 1's value is better; the old slot 1 is not re-judged
    v = np.full((3, 3), -1.0, np.float32)
    v[0, 1], v[0, 2], v[1, 2] = 0.9, 0.6, 0.8
    li = np.array([0, 1], np.uint32)
    assert X.labels_from_definition(3, v, 0.5, 2, li, X.FIRST)[0].tolist() == [0, 1, 0]
    assert X.labels_from_definition(3, v, 0.5, 2, li, X.BEST)[0].tolist() == [0, 1, 1]
    rp, col, val = X.csr_of_values(3, v, 0.5)
    assert X.labels(3, rp, col, val, 2, li, X.BEST)[0].tolist() == [0, 1, 1]
    # an old slot that is NOT a representative covers nobody, although it hits the new slot
    li = np.array([0, 0], np.uint32)
    v[0, 2] = -1.0
    assert X.labels(3, *X.csr_of_values(3, v, 0.5), 2, li, X.FIRST)[0].tolist() == [0, 0, 2]
    assert X.labels_from_definition(3, v, 0.5, 2, li, X.BEST)[0].tolist() == [0, 0, 2]
