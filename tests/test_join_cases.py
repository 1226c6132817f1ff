"""The conditions of tests/join_cases.py, proved on the CPU before the device is asked (tests/test_gpu_join_weighted.py): for
every collection the device tests use, the thresholds are uniform, the lists are within their caps, the designated
pairs hold matches of every value order and near misses in every designated tail, the crowded variants crowd a bucket,
no designated pair's reference is 0 or not finite -- and EVERY join decision of EVERY designated pair, taken wrongly,
moves the float32 reference of each estimator by at least 16 times the suite's tolerance (close() of
tests/test_gpu_compare.py).  The smallest margin per collection and tail is printed (pytest -s).

A collection is built once per parameter and dropped after it (p = 20: 129 MiB)."""
import numpy as np
import pytest

import join_cases as jc
from test_gpu_compare import RTOL, close

UNIFORM = [k for k in jc.KEYS if k[0] != "M"]


@pytest.fixture(scope="module", params=UNIFORM, ids=jc.key_id)
def coll(request):
    return jc.build(request.param)


def passes_close(got, ref):
    try:
        close(got, ref)
    except AssertionError:
        return False
    return True


def test_error_model_moves_one_count_between_a_tail_bin_and_the_boundary():
    H = np.arange(64) + 10
    T, L = 3, 2
    for kind, tail, bin_, at, boundary in (("missed", "upper", 7, +1, T), ("false", "upper", 7, -1, T),
                                           ("missed", "lower", 9, -1, L), ("false", "lower", 9, +1, L)):
        Hw = jc.perturbed(H, jc.Decision(kind, tail, 5, 6, 9, 7), T, L, 14)
        diff = Hw - H
        assert diff[bin_] == at and diff[boundary] == -at and np.count_nonzero(diff) == 2, (kind, tail)


def test_decisions_find_matches_and_near_misses_by_position_group():
    for p, other in ((10, 101), (16, 103)):  # sh = 0: the neighbour; sh = 2: the same group of four
        regs = np.zeros((2, 1 << p), np.uint8)
        regs[0, [7, 100, 300]] = (3, 4, 5)
        regs[1, [7, other, 340]] = (6, 2, 1)
        ds = jc.decisions(regs, 0, 1, p, 0, 0)
        assert ds == [jc.Decision("missed", "upper", 7, 7, 3, 6), jc.Decision("false", "upper", 100, other, 4, 2)]


def test_the_shapes_are_the_ones_the_device_test_runs():
    assert len(jc.KEYS) == 4 * len(jc.SHAPES) + len(jc.MIXED) and len(set(jc.KEYS)) == len(jc.KEYS)
    assert {p for p, _ in jc.SHAPES} == set(jc.C_PARAMS)


def test_uniform_thresholds_and_lists_within_the_caps(coll):
    lo, hi, T, L, nup, nlow = coll.thresholds()
    Tu, Lu = coll.uniform()
    assert (Tu, Lu) == ((0, 0) if coll.family == "S" else (coll.b + 1, coll.b))
    assert (hi == 64 - coll.p + 1).all()  # every sketch lists q + 1: the column order is the same with and without the key
    assert nup.min() >= 8 and (coll.family == "S" or nlow.min() >= 8)
    assert (nup <= coll.emax).all() and (nlow <= coll.elow).all()
    assert coll.regs[:, -1].max() > Tu  # position 2^p - 1 is listed above: position << 8 | value fills its word at p = 24
    if coll.family == "C":
        low = coll.regs[coll.regs < coll.b]
        assert low.min() == 0 and low.max() <= coll.b - coll.deep
    if coll.crowded:
        full, holds = jc.fullest_bucket(coll)
        assert full > holds, (full, holds)


@pytest.mark.parametrize("p,n", jc.MIXED)
def test_mixed_collections_disagree_on_the_thresholds(p, n):
    coll = jc.build(("M", p, n))
    lo, hi, T, L, nup, nlow = coll.thresholds()
    assert len(np.unique(T)) > 2 and len(np.unique(L)) > 2
    assert (nup <= coll.emax).all() and (nlow <= coll.elow).all()
    for order in (jc.jm.key_order(hi, T, L), np.arange(n)):
        cols = order[: jc.TILE]
        # a block's tiles run above the thresholds of some of its sketches: listed entries that are not looked up
        assert T[cols].min() < T[cols].max() and L[cols].min() < L[cols].max()


def test_every_decision_of_a_designated_pair_moves_the_reference(coll, oracle):
    T, L = coll.uniform()
    pairs = jc.designated_pairs(coll)
    npairs = coll.n * (coll.n - 1) // 2
    assert len(pairs) >= min(64, npairs) and len(set(pairs)) == len(pairs), len(pairs)
    kinds = {k for _, _, k in pairs}
    want_kinds = {"all"} if npairs <= 64 else {"diagonal"} if coll.n <= jc.TILE else {"diagonal", "ragged"} if coll.n <= 2 * jc.TILE else {"diagonal", "off-diagonal", "ragged"}
    assert kinds == want_kinds, kinds
    cards = [oracle.cardinalities(coll.regs, e) for e in (0, 1, 2)]
    worst = {t: np.inf for t in coll.tails}
    for i, j, _ in pairs:
        ds, facts = jc.pair_facts(coll, i, j)
        assert jc.structurally_fit(coll, facts), (i, j, facts)
        H = jc.union_hist(coll.regs, i, j)
        for estim in (0, 1, 2):
            ca, cb = cards[estim][i], cards[estim][j]
            ref = jc.reference(oracle, H, ca, cb, coll.p, estim)
            assert np.isfinite(ref) and ref != 0, (i, j, estim, ref)  # a pair clamped to 0 is blind
            for tail in coll.tails:
                mine = [d for d in ds if d.tail == tail]
                got = []
                for d in mine:
                    Hw = jc.perturbed(H, d, T, L, coll.p)
                    assert Hw.min() >= 0 and (Hw.sum() == H.sum() or Hw.max() >= 0xFFFF), d  # (a wrapped bin: jc.perturbed)
                    got.append(jc.reference(oracle, Hw, ca, cb, coll.p, estim))
                # close()'s tolerance depends on ref alone, so the decision that moves ref least stands for all of the
                # pair's: a 16th of its move must still fail close() -- every decision is worth at least 16 tolerances
                move = np.abs(np.array(got, np.float64) - np.float64(ref))
                k = int(np.argmin(np.where(np.isfinite(move), move, np.inf)))
                part = np.float64(ref) + (np.float64(got[k]) - np.float64(ref)) / jc.MARGIN
                assert not passes_close(part, ref), (
                    "pair (%d, %d) estimator %d: %r moves %r to %r, %.3g tolerances" % (i, j, estim, mine[k], ref, got[k], jc.margin(got[k], ref, RTOL)))
                worst[tail] = min(worst[tail], jc.margin(got[k], ref, RTOL))
    for t in coll.tails:
        print("margin %s %s: %.3g tolerances (relative %.3g)" % (coll.name, t, worst[t], worst[t] * RTOL))
