"""The model of the union growth curve against itself, and dsh_curve_permutations against its Python restatement."""
import numpy as np
import pytest

import curve_ref
import dashing_amd
from dashing_amd import synth

P = 10


@pytest.fixture(scope="module")
def regs():
    r = synth.synthetic_sketches(20, P, seed=5)
    r[3] = 0
    return r


def test_every_model_histogram_sums_to_the_registers(regs):
    for order in (np.arange(20), np.arange(20)[::-1], [7], [3, 3, 4]):
        h = curve_ref.curve_hist(regs, order)
        assert h.dtype == np.uint32 and h.shape == (len(order), 64)
        assert (h.sum(axis=1) == 1 << P).all()
    assert curve_ref.curve_hist(regs, []).shape == (0, 64)


def test_a_repeated_member_repeats_the_previous_histogram(regs):
    h = curve_ref.curve_hist(regs, [5, 5, 2, 5, 2, 9, 9])
    for i in (1, 3, 4, 6):
        assert (h[i] == h[i - 1]).all()
    assert (h[2] != h[1]).any() and (h[5] != h[4]).any()


def test_the_last_prefix_of_a_permutation_is_the_union_of_all(regs):
    whole = np.bincount(regs.max(axis=0), minlength=64)
    for order in curve_ref.permutations(20, 4, 99):
        assert (curve_ref.curve_hist(regs, order)[-1] == whole).all()


@pytest.mark.parametrize("n", (0, 1, 2, 3, 64, 1000))
def test_permutations_equal_the_restatement(n):
    for seed in (0, 1, 11, 2**64 - 1, 0xDEADBEEF12345678):
        for n_perm in (0, 1, 5):
            got = dashing_amd.curve_permutations(n, n_perm, seed)
            assert got.dtype == np.uint32 and got.shape == (n_perm, n)
            assert (got == curve_ref.permutations(n, n_perm, seed)).all()
            for row in got:
                assert (np.sort(row) == np.arange(n)).all()
            if n >= 8:
                assert len({row.tobytes() for row in got}) == n_perm


def test_permutation_r_depends_on_seed_plus_r_alone():
    a = dashing_amd.curve_permutations(50, 5, 7)
    b = dashing_amd.curve_permutations(50, 3, 9)
    assert (a[2:] == b).all()
