"""k_finalize's tail join on collections where every match decision moves the float32 result (tests/join_cases.py; the
conditions and the margins are proved on the CPU by tests/test_join_cases.py: one wrong decision of a designated pair
is worth at least 16 tolerances).  Shapes: the smallest at which the join can go wrong -- one full and one ragged
column block (n = 129), three blocks (n = 260) up to p = 16, n = 129 at p = 17 .. 20, n = 20 at p = 22 and n = 6 at
p = 24 (sh = 0 .. 10, 32-bit positions from p = 16, position << 8 | value filling its word at p = 24).

Per collection (S, C, their crowded variants, and the mixed collections, which make no sensitivity claim): the full
triangle against the oracle within close() of tests/test_gpu_compare.py, and every other call form byte for byte
against that full call.  A collection is built once per module parameter, marked read-only, and dropped after it."""
import numpy as np
import pytest

import dashing_amd

import join_cases as jc
from test_gpu_compare import close

pytestmark = pytest.mark.gpu


class Loaded:
    def __init__(self, coll):
        self.coll = coll
        self.pairs = jc.designated_pairs(coll) if coll.tails else [(i, i + 1 + i % 3, "any") for i in range(0, coll.n - 3, 2)]
        self.full = None  # the device's full JI triangle under MLE, once computed


@pytest.fixture(scope="module", params=jc.KEYS, ids=jc.key_id)
def loaded(request):
    return Loaded(jc.build(request.param))


def full_triangle(ctx, ld):
    ctx.set_sketches(ld.coll.regs)
    if ld.full is None:
        ld.full = ctx.dist_rows()
        ld.full.setflags(write=False)
    return ld.full


@pytest.mark.parametrize("estim,rt", [(0, dashing_amd.JI), (1, dashing_amd.JI), (2, dashing_amd.JI), (2, dashing_amd.MASH_DIST),
                                      (2, dashing_amd.SIZES), (2, dashing_amd.CONTAINMENT_INDEX)])
def test_triangle_vs_oracle(ctx, oracle, loaded, estim, rt):
    regs = loaded.coll.regs
    want = oracle.dist_tri(regs, estim, rt, 31)
    ctx.set_sketches(regs)
    got = ctx.dist_rows(estim=estim, result_type=rt, k=31)
    close(got, want)
    if rt == dashing_amd.MASH_DIST:
        assert ((got == 1.0) == (want == 1.0)).all()
    if rt == dashing_amd.JI and loaded.coll.tails:  # the designated pairs are not blind
        n = loaded.coll.n
        at = np.array([dashing_amd.tri_index(n, i, j) for i, j, _ in loaded.pairs])
        assert (want[at] > 0).all() and np.isfinite(want[at]).all()


def test_call_forms_return_the_triangle_bytes(ctx, loaded):
    """a row range across the block boundary, the rectangle in both orientations, the explicit pairs (k_pairs_hist forms
    the histogram without the join: an independent device path) and the thresholded output"""
    n = loaded.coll.n
    full = full_triangle(ctx, loaded)
    sq = np.zeros((n, n), np.float32)
    iu = np.triu_indices(n, 1)
    sq[iu] = full
    sq.T[iu] = full
    rb, re = (100, 131) if n > 131 else (100, n - 1) if n > 128 else (1, n - 1)
    a, b = dashing_amd.tri_span(n, 0, rb), dashing_amd.tri_span(n, 0, re)
    assert ctx.dist_rows(rb, re).tobytes() == full[a:b].tobytes()
    h = n // 2
    assert ctx.dist_rect(1, h, h, n).tobytes() == np.ascontiguousarray(sq[1:h, h:n]).tobytes()          # rows before columns
    assert ctx.dist_rect(h + 1, n, 0, h + 1).tobytes() == np.ascontiguousarray(sq[h + 1 : n, 0 : h + 1]).tobytes()  # columns before rows
    pi = np.array([i for i, _, _ in loaded.pairs], np.uint32)
    pj = np.array([j for _, j, _ in loaded.pairs], np.uint32)
    at = np.array([dashing_amd.tri_index(n, int(i), int(j)) for i, j in zip(pi, pj)])
    assert ctx.dist_pairs(pj, pi)[0].tobytes() == full[at].tobytes()  # (lhs = j, rhs = i < j: dist_rows' orientation)
    vals = np.unique(full[at])
    assert len(vals) >= 2
    thr = float(np.float32((np.float64(vals[len(vals) // 2 - 1]) + np.float64(vals[len(vals) // 2])) / 2))  # between two designated values
    row_ptr, col, val = ctx.dist_threshold(thr)
    keep = sq >= np.float32(thr)
    keep[np.tril_indices(n)] = False
    assert row_ptr.tolist() == np.concatenate(([0], np.cumsum(keep.sum(1)))).tolist()
    wr, wc = np.nonzero(keep)
    assert col.tolist() == wc.tolist() and val.tobytes() == sq[wr, wc].tobytes()
    assert 0 < (full[at] >= np.float32(thr)).sum() < len(at)


def test_column_order_and_list_caps_return_the_triangle_bytes(ctx, loaded):
    """option sort = 0 and 1, and the list caps through set_option: with shorter lists the thresholds move and registers go
    from the join to the dense planes -- the result does not"""
    full = full_triangle(ctx, loaded)
    try:
        for sort in (0, 1):
            ctx.set_option("sort", sort)
            assert ctx.dist_rows().tobytes() == full.tobytes(), sort
    finally:
        ctx.set_option("sort", -1)
    try:
        for emax, elow in ((0, 0), (3, 0), (0, 3), (64, 200), (-1, -1)):
            ctx.set_option("emax", emax)
            ctx.set_option("elow", elow)
            assert ctx.dist_rows().tobytes() == full.tobytes(), (emax, elow)
    finally:
        ctx.set_option("emax", -1)
        ctx.set_option("elow", -1)
