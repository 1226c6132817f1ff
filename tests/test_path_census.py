"""CPU tests of the path census (tools/path_census.py): every condition on a hand-made collection of a few sketches on which
it holds by construction, and on a neighbouring collection on which it does not; agreement with the join's model
(tools/join_model.py) wherever both speak; and THE MATRIX -- every instance of tests/path_cases.py x every condition is
reached by some run of tests/test_gpu_paths.py, or is declared impossible with its arithmetic."""
import numpy as np
import pytest

from dashing_amd import synth

import path_cases as pc
import path_census as pcs
import join_model as jm


def const(p, v, n=1, **at):
    """n sketches of the value v; at: position -> value of single registers (pos_3=20 sets register 3 of every sketch)"""
    r = np.full((n, 1 << p), v, np.uint8)
    for k, x in at.items():
        r[:, int(k.split("_")[1])] = x
    return r


def cat(*parts):
    return np.concatenate(parts)


def two_valued(p, a, b):
    r = np.full((1, 1 << p), a, np.uint8)
    r[0, ::2] = b
    return r


# condition -> (p, collection on which it holds, the neighbour on which it does not), each (regs, emax, elow); identity
# column order.  One block, i.e. one (diagonal) tile, unless the condition needs two.
P = 6  # 64 registers, values <= 59, RK = 7
HAND = {
    "sketch.nothing_listed": (P, (const(P, 3), 1, 1), (const(P, 3, pos_0=7), 1, 1)),
    # two registers above the value 0 fit a list of two (the walk goes on down to lo) and not a list of one (it stops at hi)
    "sketch.T_at_lo": (P, (const(P, 0, pos_1=5, pos_2=5), 2, 0), (const(P, 0, pos_1=5, pos_2=5), 1, 0)),
    # one register above 5 (listed: T = 5), one below at 2: with a lower list of one L walks 2 -> 5 = T; without, L = lo
    "sketch.L_at_T_above_lo": (P, (const(P, 5, pos_1=9, pos_2=2), 1, 1), (const(P, 5, pos_1=9, pos_2=2), 1, 0)),
    "sketch.upper_list_full": (P, (const(P, 5, pos_1=9), 1, 0), (const(P, 5, pos_1=9), 2, 0)),
    "sketch.lower_list_full": (P, (const(P, 5, pos_2=2), 0, 1), (const(P, 5, pos_2=2), 0, 2)),
    # T = L = lo = 5 in the block; a sketch of 7 beside it raises the tile's T to 7 over Lp = 5
    "tile.no_dense_plane": (P, (const(P, 5, 2), 1, 1), (cat(const(P, 5), two_valued(P, 5, 7)), 1, 1)),
    # values from 0, threshold 20: 20 planes; threshold 16: one batch exactly
    "tile.planes_beyond_batch": (P, (cat(const(P, 0), const(P, 20)), 0, 0), (cat(const(P, 0), const(P, 16)), 0, 0)),
    # lo = 2, and L = 5 only where the register at 2 is listed
    "tile.bins_below_dense": (P, (const(P, 5, 2, pos_2=2), 0, 1), (const(P, 5, 2, pos_2=2), 0, 0)),
    # T = 5: x0 = 0, bins 0 .. 47 travel in the three words; a register at 48 is the 49th
    "tile.tail_bins_beyond_48": (P, (const(P, 5, 2, pos_1=48), 1, 0), (const(P, 5, 2, pos_1=47), 1, 0)),
    "tile.tail_words_cut": (P, (const(P, 31, 2), 0, 0), (const(P, 30, 2), 0, 0)),
    # the first sketch lists its 9 (T = 5); the second one's threshold is 12 -- or 8
    "tile.row_upper_in_dense": (P, (cat(const(P, 5, pos_1=9), const(P, 12)), 1, 0), (cat(const(P, 5, pos_1=9), const(P, 8)), 1, 0)),
    # the first sketch lists its 2 (L = 5); a sketch of 1 in the block brings Lp to 1, a sketch of 5 leaves it at 5
    "tile.row_lower_in_dense": (P, (cat(const(P, 5, pos_2=2), const(P, 1)), 0, 1), (cat(const(P, 5, pos_2=2), const(P, 5)), 0, 1)),
    # 20 and 9 listed at one position; a third sketch of 12 puts the tile's T between them
    "tile.column_entry_rejected": (P, (cat(const(P, 5, pos_3=20), const(P, 5, pos_3=9), const(P, 12)), 1, 0),
                                   (cat(const(P, 5, pos_3=20), const(P, 5, pos_3=9)), 1, 0)),
    "join.upper_equal_values": (P, (const(P, 5, 2, pos_3=20), 1, 0), (cat(const(P, 5, pos_3=20), const(P, 5, pos_3=21)), 1, 0)),
    "join.lower_equal_values": (P, (const(P, 5, 2, pos_3=2), 0, 1), (cat(const(P, 5, pos_3=2), const(P, 5, pos_3=1)), 0, 1)),
    # p = 15: positions 8 and 9 share bucket group 4, position 10 lies in group 5
    "join.group_entry_dropped": (15, (cat(const(15, 5, pos_8=20), const(15, 5, pos_9=20)), 1, 0),
                                 (cat(const(15, 5, pos_8=20), const(15, 5, pos_10=20)), 1, 0)),
    # a row finds its own entry in the diagonal tile; with empty lists it finds nothing
    "join.entry_for_lane_without_pair": (P, (cat(const(P, 5, pos_3=20), const(P, 5, pos_4=20)), 1, 0),
                                         (cat(const(P, 5, pos_3=20), const(P, 5, pos_4=20)), 0, 0)),
    # RK = 7: eight sketches list position 3, or seven
    "join.bucket_beyond_record": (P, (const(P, 5, 8, pos_3=20), 1, 0), (const(P, 5, 7, pos_3=20), 1, 0)),
    "join.bucket_beyond_wave_read": (P, (const(P, 5, 72, pos_3=20), 1, 0), (const(P, 5, 71, pos_3=20), 1, 0)),
    # three entries per row, each found in every column: 3 x 86 = 258 items, 3 x 85 = 255
    "join.queue_drained_early": (P, (const(P, 5, 86, pos_3=20, pos_4=20, pos_5=20), 3, 0), (const(P, 5, 85, pos_3=20, pos_4=20, pos_5=20), 3, 0)),
    "collection.no_planes": (P, (const(P, 5, 2), 1, 1), (cat(const(P, 5), const(P, 7)), 1, 1)),
    # a block of 128 sketches of 5 (no plane) and a second block with a sketch of 5 and 7 (planes 6 and 7 in its tiles)
    "collection.band_mixed_planes": (P, (cat(const(P, 5, 128), two_valued(P, 5, 7)), 0, 0), (const(P, 5, 129), 0, 0)),
}


def test_every_condition_has_a_hand_made_collection():
    assert set(HAND) == set(pcs.CONDITIONS)


@pytest.mark.parametrize("name", list(pcs.CONDITIONS))
def test_condition_on_a_hand_made_collection_and_not_on_its_neighbour(name):
    p, (regs, emax, elow), (nregs, nemax, nelow) = HAND[name]
    assert name in pcs.census(regs, p, emax, elow, sort=False), name
    assert name not in pcs.census(nregs, p, nemax, nelow, sort=False), name


def test_instances():
    for p, want in pc.INSTANCES.items():
        assert pcs.instance(p, jm.auto_list_cap(p, True), jm.auto_list_cap(p, False)) == want
    assert pcs.instance(8, 255, 255)["RK"] == 3 and pcs.instance(12, 128, 128)["RK"] == 7 and pcs.instance(13, 0, 0)["RK"] == 3
    assert pcs.instance(9, 3, 2)["tile_kernel"] == "lockstep" and pcs.instance(9, 3, 2, kc=32)["tile_kernel"] == "free"


def scalar_lookups(regs, s, T, L, Tt, Lp, cb, p):
    """the look-ups of one row, entry by entry and without lookup_matches: the independent statement both the census and
    jm.row_lookups are held to.  Per entry: the bucket's count (-1: not looked up), its entries of the same position, and
    those of them that pass the value filter"""
    sh = max(p - 14, 0)
    out = []
    for pos in range(regs.shape[1]):
        va = int(regs[s, pos])
        if not (va > T[s] or va < L[s]):
            continue  # not listed
        if not (va > Tt or va < Lp):
            out.append((-1, 0, 0))
            continue
        bucket = ((pos >> sh) << 1) | (0 if va > Tt else 1)
        found = [i for i in range(len(cb.bucket)) if cb.bucket[i] == bucket]
        same = [i for i in found if cb.pos[i] == pos]
        live = [i for i in same if (cb.vb[i] > Tt if va > Tt else cb.vb[i] < Lp)]
        out.append((len(found), len(same), len(live)))
    return out


@pytest.mark.parametrize("p,n,sort", [(8, 260, True), (10, 300, False), (14, 200, True), (16, 140, True)])
def test_census_agrees_with_the_join_model(p, n, sort):
    """thresholds, column order, blocks and the look-ups: what tools/join_model.py says row by row is what the census
    says tile by tile, and both are what an entry-by-entry loop of the test's own finds on sampled rows"""
    regs = np.concatenate((synth.related_sketches(n - 40, p, seed=3 * p)[0], pc.constant_outliers(40, p, seed=p)))
    emax, elow = jm.auto_list_cap(p, True), jm.auto_list_cap(p, False)
    c = pcs.census(regs, p, sort=sort)
    lo, hi, T, L = jm.thresholds(regs, emax, elow)
    order = jm.key_order(hi, T, L) if sort else np.arange(n)
    assert c.instance["RK"] == jm.record_inline(p, emax + elow)
    for b, blk in enumerate(c.blocks):
        cols = order[b * 128 : (b + 1) * 128]
        assert (blk["cols"] == cols).all()
        assert (blk["T"], blk["L"], blk["lo"]) == (int(T[cols].max()), int(L[cols].min()), int(lo[cols].min()))
    index = {}
    for t in c.tiles:
        bi, bj = c.blocks[t["bi"]], c.blocks[t["bj"]]
        assert t["T"] == max(bi["T"], bj["T"]) and t["Lp"] == max(max(bi["lo"], bj["lo"]), min(bi["L"], bj["L"]))
        cb = index.setdefault(t["bj"], jm.ColumnBlock(regs, bj["cols"], T, L, p))
        items = live = 0
        fullest = -1
        for k, s in enumerate(bi["cols"]):
            cnt, it, ap, _ = jm.row_lookups(regs, int(s), T, L, lo, bi, bj, cb, p)
            if k % 37 == 0:
                assert list(zip(cnt.tolist(), it.tolist(), ap.tolist())) == scalar_lookups(regs, int(s), T, L, t["T"], t["Lp"], cb, p), (t, s)
            items += int(it.sum())
            live += int(ap.sum())
            fullest = max(fullest, int(cnt.max()) if cnt.size else -1)
        assert (t["items"], t["live"], t["fullest"]) == (items, live, fullest), t


def test_plan_figures_of_a_known_collection():
    """pbase, P and the tiles' planes as plan::build_layout and plan::tile_planes make them, on numbers worked out by hand:
    128 sketches of 5 (T = L = 5), then 3 sketches of 0 and 9 by halves (T = 9, L = lo = 0)"""
    regs = np.concatenate((const(P, 5, 128), np.repeat(two_valued(P, 0, 9), 3, axis=0)))
    c = pcs.census(regs, P, 0, 0, sort=False)
    # pbase = the smallest L = 0, P = 9 - 0; tile (0, 0): lo_t = 5 = T: none; (0, 1): lo_t = max(max(5, 0), min(5, 0)) = 5, T = 9: 4;
    # (1, 1): lo_t = 0, T = 9: 9
    assert (c.plan["pbase"], c.plan["planes"], c.plan["tiles"], c.plan["sum_tile_planes"]) == (0, 9, 3, 13)
    assert [t["planes"] for t in c.tiles] == [0, 4, 9] and c.plan["avg_tile_planes_x100"] == 433
    assert c.plan["kpad"] == 32 and c.plan["cum_bytes"] == 2 and c.plan["lockstep"] == 0  # 9 planes x 2 words, stages of 16


def test_families_hold_what_they_are_named_for():
    """in both column orders, at every precision and size the GPU file uses them at"""
    for case in pc.CASES:
        for sort in (True, False):
            c = case.census(sort=sort)
            assert c.instance == pc.INSTANCES[case.p], case.id
            assert pc.NAMED_FOR[case.family] <= c.holds(), (case.id, sort, sorted(pc.NAMED_FOR[case.family] - c.holds()))


def test_the_matrix_every_instance_meets_every_condition():
    """the union of the census over every run of tests/test_gpu_paths.py (collection x list caps x column order), counted
    for the instance it really runs in: every cell of instance x condition is hit, but for the cells declared impossible
    -- and those are hit by nothing"""
    hit = {p: set() for p in pc.INSTANCES}
    for run in pc.census_runs():
        c = run.census()
        if c.instance == pc.INSTANCES[run.p]:  # (255 + 255 list entries turn RK = 7 into RK = 3: another instance)
            hit[run.p] |= c.holds()
    assert all(p in pc.INSTANCES and name in pcs.CONDITIONS for p, name in pc.IMPOSSIBLE)
    missing = sorted((p, name) for p in pc.INSTANCES for name in pcs.CONDITIONS if name not in hit[p] and (p, name) not in pc.IMPOSSIBLE)
    assert not missing, "cells no run reaches: %s" % missing
    wrongly = sorted((p, name) for p, name in pc.IMPOSSIBLE if name in hit[p])
    assert not wrongly, "cells declared impossible, yet reached: %s" % wrongly
