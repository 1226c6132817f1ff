"""Table words per workgroup in the LDS placement of the sparse counting kernel (kernels_sparseplane.hip,
k_sparse_count_lds<CT, NW>; option and info sparse_words): with 2 a workgroup stages a word PAIR of the table slab, a lane
gathers 64 column bits per list entry and keeps two counter sets; either way a lane walks its list four steps of eight
entries at a time as a Harley-Seal tree over 32 entries, and what is left of the list step by step.

The route is FORCED (sparse_sided = 1).  For sparse_words in {1, 2} and sparse_run in {1, 4}: the output bytes of three
estimators x (JI, SIZES, CONTAINMENT_INDEX) equal the same context's run with every route off and its run with the table
gathered (sparse_lds = 0); one triangle per p is within the suite's 1e-6 of the oracle.

PLANTED collections make the list lengths exact: every register is B, and sketch g has k_g registers at B + 1, so that k_g
is the size of its set at the one plane of the call.  k runs through 0, 1, 7, 8, 9 (the partial last step), 31, 32, 33,
63, 64, 65, 255, 256, 257 (the tree's blocks of 32 entries a lane, at four and at eight lanes a row), cap - 1 and cap at
sparse_cap = 2040 (the counters at full width).  With `mixed`, sketches with all but k registers at B + 1 (their sets A(v)
are the short ones) and half-full ones stand between them: the blocks with a half-full sketch are no list side, and the
tiles of those rows against the last block are transposed items with lists in the A polarity.  The sided families
(tests/sparse_cases.py) add both polarities on both sides, transposed items in the U polarity and two bands.  What each
case routes is asserted on the host first, from the census model (tools/path_census.py) and `info`."""
import numpy as np
import pytest

import dashing_amd

from sparse_cases import pcs
from test_gpu_sparse_planes import close
from test_gpu_sparse_runs import runs_of
from test_gpu_sparse_sided import MEASURES, sided
from test_sparse_sided_model import case, kinds_of

pytestmark = pytest.mark.gpu
B = 5
CAP = pcs.SPARSE_CAP_MAX
LENGTHS = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257, CAP - 1, CAP)
WORDS, RUNS = (1, 2), (1, 4)
KEYS = [(e, m) for e in (0, 1, 2) for m in MEASURES]
_planted = {}


def planted(n, p, mixed=False):
    """(regs, k): k[g] registers of sketch g are B + 1, all others B; mixed: groups of 16 sketches take turns as k = a
    length, k = 2^p - a length, and k = 2^p / 2"""
    if (n, p, mixed) not in _planted:
        m = 1 << p
        rng = np.random.default_rng(0x5B0000 + 131 * p + n)
        regs, k = np.full((n, m), B, np.uint8), np.zeros(n, np.int64)
        for g in range(n):
            a, turn = LENGTHS[g % 16], (g // 16) % 3 if mixed else 0
            k[g] = (a, m - a, m // 2)[turn]
            regs[g, rng.choice(m, k[g], replace=False)] = B + 1
        _planted[(n, p, mixed)] = (regs, k)
    return _planted[(n, p, mixed)]


class words_of(runs_of):
    """test_gpu_sparse_runs.runs_of at a number of table words: set for a block, and put back behind it"""

    def __init__(self, ctx, words, run, **more):
        runs_of.__init__(self, ctx, run, sparse_words=words, **more)
        self.defaults["sparse_words"] = 0


def listed_lengths(c, k, m):
    """per polarity of the list side: the set sizes in the list blocks of the model's items, and how many are transposed"""
    got, transposed = {0: set(), 1: set()}, 0
    for t in c.tiles:
        for _, la, _, tr in t["sided"]:
            kk = k[c.blocks[t["bj"] if tr else t["bi"]]["cols"]]
            got[la] |= set((m - kk if la else kk).tolist())
            transposed += tr
    return got, transposed


def both_words(ctx, off, gathered, items, transposed, what, **more):
    for words in WORDS:
        for run in RUNS:
            with words_of(ctx, words, run, cap=CAP, **more):
                assert (ctx.info("sparse_words"), ctx.info("sparse_run")) == (words, run)
                for key in KEYS:
                    got = ctx.dist_rows(estim=key[0], result_type=key[1])
                    assert got.tobytes() == off[key].tobytes(), (what, words, run, key, "against the routes off")
                    assert got.tobytes() == gathered[key].tobytes(), (what, words, run, key, "against the gathered table")
                    assert (ctx.info("sparse_items"), ctx.info("sparse_transposed_items")) == (items, transposed), (what, words, run)
                assert ctx.info("sparse_table_fills") > 0


def references(ctx, items, cap):
    with sided(ctx, 0, cap=cap):
        off = {key: ctx.dist_rows(estim=key[0], result_type=key[1]) for key in KEYS}
        assert ctx.info("sparse_items") == 0
    with sided(ctx, 1, cap=cap, sparse_lds=0):
        gathered = {key: ctx.dist_rows(estim=key[0], result_type=key[1]) for key in KEYS}
        assert ctx.info("sparse_items") == items and ctx.info("sparse_words") == 0 and ctx.info("sparse_table_fills") == 0
    return off, gathered


@pytest.mark.parametrize("n,mixed", ((129, False), (257, False), (300, False), (300, True)))
@pytest.mark.parametrize("p", (13, 14))
def test_planted_lengths(ctx, oracle, n, p, mixed):
    regs, k = planted(n, p, mixed)
    c = pcs.census(regs, p, sparse_planes=0, sparse_cap=CAP, sparse_sided=1)
    items = c.plan["sparse_items"]
    lengths, transposed = listed_lengths(c, k, 1 << p)
    assert items > 0 and items % 8  # (a ragged run at either run length)
    if mixed:
        assert transposed == items and set(LENGTHS[:11]) <= lengths[1] and not lengths[0]
    else:
        assert transposed == 0 and lengths[0] == set(LENGTHS) and not lengths[1]
    ctx.set_option("sparse_cap", CAP)  # (before the matrix is attached: the per-sketch pass runs at this cap)
    try:
        ctx.set_sketches(regs)
        off, gathered = references(ctx, items, CAP)
        if n == 129:
            e, r = dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI
            close(off[(e, r)], oracle.dist_tri(regs, e, r, 31), (n, p, "off"))
        both_words(ctx, off, gathered, items, transposed, (n, p, mixed))
    finally:
        ctx.set_option("sparse_cap", pcs.SPARSE_CAP)


def test_a_word_pair_does_not_fit_at_p15(ctx, oracle):
    n, p = 129, 15
    regs, k = planted(n, p)
    c = pcs.census(regs, p, sparse_planes=0, sparse_cap=CAP, sparse_sided=1)
    items = c.plan["sparse_items"]
    assert items > 0 and listed_lengths(c, k, 1 << p)[0][0] == set(LENGTHS)
    ctx.set_option("sparse_cap", CAP)
    try:
        ctx.set_sketches(regs)
        off, gathered = references(ctx, items, CAP)
        e, r = dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI
        close(off[(e, r)], oracle.dist_tri(regs, e, r, 31), (n, p, "off"))
        for words in (0, 1):
            for run in RUNS:
                with words_of(ctx, words, run, cap=CAP):
                    assert ctx.info("sparse_words") == 1
                    for key in KEYS:
                        got = ctx.dist_rows(estim=key[0], result_type=key[1])
                        assert got.tobytes() == off[key].tobytes() == gathered[key].tobytes(), (words, run, key)
                    assert ctx.info("sparse_items") == items
        with words_of(ctx, 2, 4, cap=CAP):
            with pytest.raises(dashing_amd.DshError, match="sparse_words"):
                ctx.dist_rows(estim=e, result_type=r)
        with words_of(ctx, 2, 4, cap=CAP, sparse_lds=0):  # (gathered: no words are staged, nothing to refuse)
            assert ctx.info("sparse_words") == 0 and ctx.dist_rows(estim=e, result_type=r).tobytes() == off[(e, r)].tobytes()
    finally:
        ctx.set_option("sparse_cap", pcs.SPARSE_CAP)


@pytest.mark.parametrize("kind", ("mixed_thresholds", "survey", "near_duplicates"))
@pytest.mark.parametrize("p", (13, 14))
def test_sided_families(ctx, kind, p):
    n = 257
    regs = case(kind, n, p)[0]
    c = pcs.census(regs, p, sparse_planes=0, sparse_sided=1)
    items, transposed = c.plan["sparse_items"], c.plan["sparse_transposed_items"]
    held = kinds_of(c)
    assert items > 8  # (a residue of more than one item)
    if kind == "mixed_thresholds":
        assert transposed > 0 and held["aa"] + held["mixed"] > 0
    ctx.set_sketches(regs)
    off, gathered = references(ctx, items, pcs.SPARSE_CAP)
    for words in WORDS:
        for run in RUNS:
            with words_of(ctx, words, run):
                assert (ctx.info("sparse_words"), ctx.info("sparse_run")) == (words, run)
                for key in KEYS:
                    got = ctx.dist_rows(estim=key[0], result_type=key[1])
                    assert got.tobytes() == off[key].tobytes() == gathered[key].tobytes(), (kind, p, words, run, key)
                    assert (ctx.info("sparse_items"), ctx.info("sparse_transposed_items")) == (items, transposed)
        if kind == "mixed_thresholds":  # (a tile's C(v) is 32 KiB x planes: three tiles to a band)
            with words_of(ctx, words, 4, cum_budget_bytes=1 << 20):
                key = (dashing_amd.ESTIM_ERTL_MLE, dashing_amd.JI)
                assert ctx.dist_rows(estim=key[0], result_type=key[1]).tobytes() == off[key].tobytes() and ctx.info("bands") >= 2 and ctx.info("sparse_transposed_items") > 0
    assert ctx.info("sparse_words") == 1  # (option 0 again: the library's choice)
