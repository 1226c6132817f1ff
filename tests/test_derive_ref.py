"""CPU: the numpy model of the derived-sketch operations (tests/derive_ref.py) against the host's own fold
(fold_registers behind dshh_fold, the `fold` subcommand) and against the algebra a fold must keep."""
import ctypes as C
import os

import numpy as np
import pytest

import derive_ref
from dashing_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(p, q) for p in range(5, 17) for q in range(4, p)]


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    lib.dshh_fold.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def random_rows(p, seed):
    """four rows: the register law at a sparse and a dense cardinality, uniform values up to the cap, mostly empty"""
    m = 1 << p
    rng = np.random.default_rng(seed)
    rows = np.zeros((4, m), np.uint8)
    rows[0] = synth.hll_registers(seed, m // 8, p)
    rows[1] = synth.hll_registers(seed + 1, 6 * m, p)
    rows[2] = rng.integers(0, 64 - p + 2, m)
    rows[3] = np.where(rng.random(m) < 0.03, rng.integers(1, 64 - p + 2, m), 0)
    return rows


def test_model_equals_host_fold(host):
    for p, q in PAIRS:
        rows = random_rows(p, 1000 * p + q)
        want = np.zeros((rows.shape[0], 1 << q), np.uint8)
        for r in range(rows.shape[0]):
            assert host.dshh_fold(rows[r].ctypes.data, p, q, want[r].ctypes.data) == 0
        assert (derive_ref.fold(rows, q) == want).all(), (p, q)


def test_fold_commutes_with_union():
    for p, q in PAIRS:
        rows = random_rows(p, 77 * p + q)
        a, b = rows[:2], rows[2:]
        assert (derive_ref.fold(np.maximum(a, b), q) == np.maximum(derive_ref.fold(a, q), derive_ref.fold(b, q))).all(), (p, q)


def test_fold_to_the_same_p_is_a_copy_and_the_cap_maps_to_the_cap():
    rows = random_rows(9, 5)
    assert (derive_ref.fold(rows, 9) == rows).all()
    one = np.zeros((1, 1 << 12), np.uint8)
    one[0, 3 << 5] = 64 - 12 + 1  # low == 0 for d = 5
    got = derive_ref.fold(one, 7)
    assert got[0, 3] == 64 - 7 + 1 and got.sum() == 64 - 7 + 1


def test_union_groups_model():
    rows = random_rows(6, 9)
    got = derive_ref.union_groups(rows, [0, 0, 1, 4, 6], [2, 0, 1, 3, 1, 1])
    assert not got[0].any() and (got[1] == rows[2]).all() and (got[2] == rows[[0, 1, 3]].max(axis=0)).all() and (got[3] == rows[1]).all()
