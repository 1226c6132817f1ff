"""The reference of the explicit pair list (tests/pairs_ref.py) against the oracle's own dense entry points, on the CPU:
pinned before the GPU sees it."""
import numpy as np
import pytest

import pairs_ref
from dashing_amd import synth


@pytest.mark.parametrize("estim", (0, 1, 2))
def test_pair_values_equal_the_oracles_dense_results(oracle, estim):
    n, p, k = 60, 10, 31
    regs = synth.synthetic_sketches(n, p, seed=77)
    regs[5] = regs[6]
    regs[11] = 0
    lhs, rhs = pairs_ref.all_tri_pairs(n)
    got = pairs_ref.pair_values(oracle, regs, lhs, rhs, pairs_ref.ALL_TYPES, estim, k)
    rev = pairs_ref.pair_values(oracle, regs, rhs, lhs, pairs_ref.ALL_TYPES, estim, k)
    for t, rt in enumerate(pairs_ref.ALL_TYPES):
        tri = oracle.dist_tri(regs, estim, rt, k)
        rect = oracle.dist_rect(regs, regs, estim, rt, k)
        assert pairs_ref.same_bits(got[t], tri), (estim, rt)
        assert pairs_ref.same_bits(got[t], pairs_ref.pick_tri(tri, n, lhs, rhs)), (estim, rt)
        assert pairs_ref.same_bits(got[t], pairs_ref.pick_rect(rect, lhs, rhs)), (estim, rt)
        assert pairs_ref.same_bits(rev[t], pairs_ref.pick_rect(rect, rhs, lhs)), (estim, rt)  # the other orientation


def test_self_pairs(oracle):
    regs = synth.synthetic_sketches(8, 10, seed=5)
    regs[3] = 0
    s = np.arange(8)
    v = pairs_ref.pair_values(oracle, regs, s, s, (1, 0), 2, 31)
    rect = oracle.dist_rect(regs, regs, 2, 1, 31)
    assert pairs_ref.same_bits(v[0], np.diagonal(rect))
    assert (v[0][np.arange(8) != 3] == 1).all() and (v[1][np.arange(8) != 3] == 0).all()


def test_tri_index():
    n = 9
    lhs, rhs = pairs_ref.all_tri_pairs(n)
    assert np.array_equal(pairs_ref.tri_index(n, rhs, lhs), np.arange(n * (n - 1) // 2))
