#!/usr/bin/env python3
"""CPU model (numpy) of the compare path's DATA-DEPENDENT branches: which of them a collection of sketches takes.

Where a SIZE decides the path (n around the tile, row ranges, parts, bands) a test can name the size.  Which arm of
finalize_block a tile takes is decided by the register values instead: by the thresholds T and L that k_selfhist_card
gives the tile's sketches.  This model says, from the registers, p, the two list caps and a column order alone,
  * the kernel INSTANCE the device runs (instance()): CT, the bytes of a C(v) count and of a histogram cell (2 for
    p <= 15, else 4), RK, the entries a bucket record holds inline (colindex_inline), and the tile kernel (free-running
    k_pair_counts where a plane is shorter than a stage of kc k-rows, i.e. below p = 9; lockstep from there);
  * the named CONDITIONS that hold (CONDITIONS below: per sketch, per tile, per tile's join, per collection), each with
    the lines of kernels_compare.hip / plan.cpp it stands for.
The rules it needs from the join's model are taken from there (tools/join_model.py: list_thresholds, key_order,
ColumnBlock, lookup_matches, auto_list_cap, record_inline, QUEUE_ITEMS); the layout rules are plan::build_layout's
(pbase, P, the blocks' statistics) and plan::tile_planes'.  It models the whole triangle in one band (sizes of a few
tiles) and, like the join's model, takes a bucket as a set.

As a tool it prints the census of the collections the existing GPU suite runs and of the collections of
tests/test_gpu_paths.py (tests/path_cases.py), one table of instance x condition each -- no device needed:

  python tools/path_census.py            # the tables (profiles/paths1/census.md)
  python tools/path_census.py --json     # one JSON line per replayed collection
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import join_model as jm  # noqa: E402

TILE = jm.TILE
CV_BATCH = 16    # kCvBatch of kernels_compare.hip: planes whose C(v) travel with the first round trip
TAIL_BINS = 48   # bins of a column's tail histogram that travel as three 16-byte words (tq[3])
PAIR_KC = 16     # k-rows of an LDS stage of the tile kernel with three items per workgroup (the default; engine.hip)
# sparse outer planes (plan.h, Tuning::sparse_planes): the defaults of the library
SPARSE_CAP = 1280        # kSparseCapDefault
SPARSE_CAP_MAX = 2040    # kSparseCapMax
SPARSE_AUTO_PLANES = 2   # kSparseAutoPlanes
SPARSE_SIDED_AUTO = True  # kSparseSidedAuto: the sided route is on where the automatic rule routes
SPARSE_MIN_BAND = 512    # the automatic rule: a band of more planes than this (Tuning::small_round_items under pair_groups = auto)

# name -> what it stands for in the code.  The order is the order of the report.
CONDITIONS = {
    # ---- per sketch: k_selfhist_card, lane 0's two walks
    "sketch.nothing_listed": "both walks stop at once (T == hi, L == lo): exc_n == 0, an all-kNone row of rl",
    "sketch.T_at_lo": "the first while runs to its bound `T > lo`: every register above the lowest bin is listed",
    "sketch.L_at_T_above_lo": "the second while runs to its bound `L < T` (L == T > lo): no dense value of its own",
    "sketch.upper_list_full": "`cnt + h[T] <= emax` held with equality: the upper list is filled exactly to its cap",
    "sketch.lower_list_full": "`cntl + h[L] <= elow` held with equality: the lower list is filled exactly to its cap",
    # ---- per tile: finalize_block
    "tile.no_dense_plane": "tile.w == tile.z (Lp == T): no item of the tile kernel, the `else prev = clow` arm",
    "tile.planes_beyond_batch": "more dense planes than kCvBatch: the `pl = tile.z + kCvBatch` loop reads C(v) itself",
    "tile.bins_below_dense": "Lp > vlo: the `x = vlo; x < Lp` loops (bins the lower join fills, clow)",
    "tile.tail_bins_beyond_48": "x0 + 48 <= vhi: the tail histogram's `x = x0 + 48` loop reads thS from global memory",
    "tile.tail_words_cut": "w0 >= 2: `w0 + k < 4` cuts the three tail words at the histogram's fourth",
    "tile.row_upper_in_dense": "a row entry its sketch lists above its own T lies at or below the tile's T: never joined",
    "tile.row_lower_in_dense": "a row entry its sketch lists below its own L lies at or above the tile's Lp: never joined",
    "tile.column_entry_rejected": "apply()'s value filter drops a found entry of the row entry's own position",
    # ---- per tile: join_tails
    "join.upper_equal_values": "an applied upper join with var == vb (`var < vb ? var : vb` takes vb)",
    "join.lower_equal_values": "an applied lower join with var == vb (`var > vb ? var : vb` takes vb)",
    "join.group_entry_dropped": "p > 14: same_position() drops an entry of another position of the bucket's group",
    "join.entry_for_lane_without_pair": "a live entry of a column whose lane owns no pair (`!all_own` and actm's bit clear)",
    "join.bucket_beyond_record": "a looked-up bucket holds more than RK entries: the wave expands it from ent[]",
    "join.bucket_beyond_wave_read": "... more than 64 + RK: rest() reads ent[] in further passes",
    "join.queue_drained_early": "a tile row queues more than 2 x kJoinQ items: one of its waves drains inside push()",
    # ---- per collection: plan::build_layout, engine.hip
    "collection.no_planes": "P == 0, Kpad == 0: no plane matrix, no transform, no tile-kernel launch (`if (c->Kpad)`)",
    "collection.band_mixed_planes": "one band holds tiles with dense planes and tiles without",
}


def instance(p, emax, elow, kc=PAIR_KC):
    """the kernel instance the device runs: k_finalize<CT, RK>, k_build_colindex<PT, RK> and the tile kernel"""
    E = max(1, emax + elow)
    W = max(1, (1 << p) // 32)  # 32-bit words of a plane (engine.hip; use_lockstep: W >= kc)
    return {"CT": 2 if p <= 15 else 4, "RK": jm.record_inline(p, E), "tile_kernel": "lockstep" if W >= kc else "free"}


class Census:
    """what census() found: .instance, .counts (condition -> sketches, tiles or 1 that hold it), .plan (the layout's
    and the tile list's figures, as dsh_get_info names them), .joins (applied upper and lower joins), .tiles (per tile:
    its blocks, Lp, T, value range, planes, queue items, live entries, fullest looked-up bucket) and .blocks"""

    def __init__(self, inst, counts, plan, joins, tiles, blocks):
        self.instance, self.counts, self.plan, self.joins, self.tiles, self.blocks = inst, counts, plan, joins, tiles, blocks

    def holds(self):
        return {k for k, v in self.counts.items() if v}

    def __contains__(self, name):
        assert name in CONDITIONS, name
        return self.counts[name] > 0


def sparse_sets(regs, v):
    """the complement sets of the plane (register < v): per sketch the positions whose register is >= v"""
    return [np.flatnonzero(r >= v) for r in np.asarray(regs)]


def sparse_plane_counts(rows, cols, v):
    """C(v) = #{t : a_t < v and b_t < v} of every (row sketch, column sketch) as the sparse route counts it
    (kernels_sparseplane.hip): the column block's table M[t] (bit j: column j has b_t >= v), every row's position list,
    and m - |U_i| - |U_j| + |U_i & U_j|"""
    rows, cols = np.asarray(rows), np.asarray(cols)
    m = rows.shape[1]
    table = cols.T >= v                      # [m positions][columns]
    len_j = table.sum(axis=0).astype(np.int64)
    out = np.empty((rows.shape[0], cols.shape[0]), np.int64)
    for i, u in enumerate(sparse_sets(rows, v)):
        out[i] = m - u.size - len_j + table[u].sum(axis=0)
    return out


def sparse_counts(regs, T):
    """k_selfhist_card's g0, g1: registers >= T_i and >= T_i - 1 per sketch, saturating 16-bit"""
    g0 = (regs >= T[:, None]).sum(axis=1)
    g1 = (regs.astype(np.int64) >= (T.astype(np.int64) - 1)[:, None]).sum(axis=1)
    return np.minimum(g0, 65535), np.minimum(g1, 65535)


def sided_thresholds(regs, cap):
    """k_selfhist_card's thresholds of the sided route at `cap`, per sketch: vU = the smallest v with #{a >= v} <= cap,
    vA = the largest v with #{a < v} <= cap (v in 0 .. 64)"""
    regs = np.asarray(regs)
    h = np.stack([np.bincount(r, minlength=64)[:64] for r in regs]).astype(np.int64)
    below = np.concatenate([np.zeros((len(regs), 1), np.int64), np.cumsum(h, axis=1)], axis=1)  # [:, v] = #{a < v}, v = 0 .. 64
    at_or_above = below[:, -1:] - below                                                          # [:, v] = #{a >= v}
    vU = (at_or_above <= cap).argmax(axis=1)
    vA = 64 - (below <= cap)[:, ::-1].argmax(axis=1)
    return vU, vA


def sided_plane_counts(lists, tables, v, list_a, table_a):
    """C(v) = #{t : a_t < v and b_t < v} of every (list sketch, table sketch) as the sided route counts it
    (kernels_sparseplane.hip, sp_values): the list side's position lists R, the table side's table S -- each U(v) = {a >= v}
    or, with its flag, A(v) = {a < v} -- cnt = |R & S| read off the table, and one of the four formulas"""
    lists, tables = np.asarray(lists), np.asarray(tables)
    m = lists.shape[1]
    table = (tables.T < v) if table_a else (tables.T >= v)  # [m positions][table sketches]
    lt = table.sum(axis=0).astype(np.int64)
    out = np.empty((lists.shape[0], tables.shape[0]), np.int64)
    for i, r in enumerate(lists):
        pos = np.flatnonzero(r < v if list_a else r >= v)
        ll, cnt = pos.size, table[pos].sum(axis=0)
        if not list_a and not table_a:
            out[i] = m - ll - lt + cnt
        elif list_a and table_a:
            out[i] = cnt
        elif not list_a and table_a:
            out[i] = lt - cnt
        else:
            out[i] = ll - cnt
    return out


def census(regs, p, emax=None, elow=None, sort=True, kc=PAIR_KC, sparse_planes=-1, sparse_cap=SPARSE_CAP, sparse_sided=0):
    """regs: [n, 2^p] uint8 (legal registers, <= 64 - p + 1); emax / elow: the list caps (None: plan::auto_list_cap);
    sort: the key-ordered column layout (True) or the identity (False); the whole triangle; sparse_planes / sparse_cap:
    the two options of the sparse outer planes (-1: the automatic rule); sparse_sided: the sided route (plan.h,
    Tuning::sparse_sided: -1 automatic, 0 off, 1 forced) -- every tile then has "below" and "sided", its items as
    (plane, list A, table A, transposed), and the plan "sparse_sided_items", "sparse_transposed_items", "sparse_table_slabs" """
    regs = np.ascontiguousarray(regs, np.uint8)
    n = regs.shape[0]
    assert n >= 1 and regs.shape[1] == 1 << p and int(regs.max()) <= 64 - p + 1
    emax = jm.auto_list_cap(p, True) if emax is None else emax
    elow = jm.auto_list_cap(p, False) if elow is None else elow
    inst = instance(p, emax, elow, kc)
    RK = inst["RK"]
    lo, hi, T, L, cnt, cntl = jm.list_thresholds(regs, emax, elow)
    counts = dict.fromkeys(CONDITIONS, 0)
    counts["sketch.nothing_listed"] = int((cnt + cntl == 0).sum())
    counts["sketch.T_at_lo"] = int(((T == lo) & (hi > lo)).sum())
    counts["sketch.L_at_T_above_lo"] = int(((L == T) & (T > lo)).sum())
    counts["sketch.upper_list_full"] = int(((cnt == emax) & (cnt > 0)).sum())
    counts["sketch.lower_list_full"] = int(((cntl == elow) & (cntl > 0)).sum())
    # plan::build_layout: the column order, the blocks' statistics, pbase (the smallest low threshold) and P
    order = jm.key_order(hi, T, L) if sort else np.arange(n)
    nblk = (n + TILE - 1) // TILE
    blk = []
    for b in range(nblk):
        cols = order[b * TILE : (b + 1) * TILE]
        blk.append({"cols": cols, "T": int(T[cols].max()), "L": int(L[cols].min()), "lo": int(lo[cols].min()), "hi": int(hi[cols].max())})
    # sparse outer planes: the blocks' bounds (plan::build_layout) and which calls route at all (plan::build_tiles)
    g0, g1 = sparse_counts(regs, T)
    for b in blk:
        b["g0"] = int(g0[b["cols"]].max())
        b["g1"] = int(np.where(T[b["cols"]] == b["T"], g1[b["cols"]], g0[b["cols"]]).max())

    def sparse_bound(b, v):
        return b["g0"] if v >= b["T"] else b["g1"] if v == b["T"] - 1 else 65535

    sp_can = (sparse_planes != 0 and sort and inst["tile_kernel"] == "lockstep" and 9 <= p <= 16 and (sparse_planes > 0 or p >= 13))
    sp_planes = 0 if not sp_can else SPARSE_AUTO_PLANES if sparse_planes < 0 else min(sparse_planes, 2)
    sp_cap = min(sparse_cap, SPARSE_CAP_MAX)
    pbase = min(int(T.max()), min(b["L"] for b in blk))
    P = int(T.max()) - pbase
    index = [jm.ColumnBlock(regs, b["cols"], T, L, p) for b in blk]  # a block's listed registers: as columns and as rows
    own_T = [T[b["cols"]][ix.jl] for b, ix in zip(blk, index)]       # per entry: its sketch's own thresholds
    own_L = [L[b["cols"]][ix.jl] for b, ix in zip(blk, index)]
    planes, joins, tiles = [], {"upper": 0, "lower": 0}, []
    for bi in range(nblk):
        for bj in range(bi, nblk):
            # plan::tile_planes and tile_vrange
            lo_t = max(max(blk[bi]["lo"], blk[bj]["lo"]), min(blk[bi]["L"], blk[bj]["L"]))
            pb = max(0, lo_t - pbase)
            pe = max(pb, max(blk[bi]["T"], blk[bj]["T"]) - pbase)
            Lp, Tt = pbase + pb, pbase + pe
            vlo, vhi = min(blk[bi]["lo"], blk[bj]["lo"]), max(blk[bi]["hi"], blk[bj]["hi"])
            planes.append(pe - pb)
            sp = 0  # planes routed sparse, from the top of the range (plan.cpp, tile_route: the two-plane route)
            while sp < sp_planes and pe - sp > pb and max(sparse_bound(blk[bi], Tt - sp), sparse_bound(blk[bj], Tt - sp)) <= sp_cap:
                sp += 1
            w0 = (Tt + 1) >> 4
            rows, cb = index[bi], index[bj]
            tile = {
                "tile.no_dense_plane": pe == pb,
                "tile.planes_beyond_batch": pe - pb > CV_BATCH,
                "tile.bins_below_dense": Lp > vlo,
                "tile.tail_bins_beyond_48": w0 * 16 + TAIL_BINS <= vhi,
                "tile.tail_words_cut": w0 >= 2,
                "tile.row_upper_in_dense": bool(((rows.vb > own_T[bi]) & (rows.vb <= Tt)).any()),
                "tile.row_lower_in_dense": bool(((rows.vb < own_L[bi]) & (rows.vb >= Lp)).any()),
            }
            # the join: every row's entries looked up in the column block's index
            c, up, e, k = jm.lookup_matches(rows.pos, rows.vb, cb, Tt, Lp, p)
            same = cb.pos[k] == rows.pos[e]
            live = same & np.where(up[e], cb.vb[k] > Tt, cb.vb[k] < Lp)
            owns = np.full(e.size, True) if bi < bj else cb.jl[k] > rows.jl[e]  # (full triangle: si < sj)
            applied = live & owns
            equal = applied & (cb.vb[k] == rows.vb[e])
            items = np.bincount(rows.jl[e[same]], minlength=1)
            tile.update({
                "tile.column_entry_rejected": bool((same & ~live).any()),
                "join.upper_equal_values": bool((equal & up[e]).any()),
                "join.lower_equal_values": bool((equal & ~up[e]).any()),
                "join.group_entry_dropped": bool((~same).any()),
                "join.entry_for_lane_without_pair": bool((live & ~owns).any()),
                "join.bucket_beyond_record": bool((c > RK).any()),
                "join.bucket_beyond_wave_read": bool((c > 64 + RK).any()),
                "join.queue_drained_early": bool((items > 2 * jm.QUEUE_ITEMS).any()),
            })
            tiles.append({"bi": bi, "bj": bj, "Lp": Lp, "T": Tt, "vlo": vlo, "vhi": vhi, "planes": pe - pb, "sparse": sp, "items": int(same.sum()),
                          "live": int(live.sum()), "fullest": int(c.max()) if c.size else -1})
            joins["upper"] += int((applied & up[e]).sum())
            joins["lower"] += int((applied & ~up[e]).sum())
            for name, holds in tile.items():
                counts[name] += int(bool(holds))
    counts["collection.no_planes"] = int(P == 0)
    counts["collection.band_mixed_planes"] = int(min(planes) == 0 < max(planes))
    W = max(1, (1 << p) // 32)
    if sparse_planes < 0 and sum(planes) <= SPARSE_MIN_BAND:  # (the automatic rule: one band here)
        for t in tiles:
            t["sparse"] = 0
    # the sided route (plan.cpp, tile_route and route_sparse): per block the largest vU and the smallest vA
    for t in tiles:
        t["below"], t["sided"] = 0, []
    sided_items = transposed = table_slabs = 0
    sd_can = sort and inst["tile_kernel"] == "lockstep" and 13 <= p <= 16
    if sd_can and (sparse_sided > 0 or (sparse_sided < 0 and sparse_planes < 0 and SPARSE_SIDED_AUTO and sum(planes) > SPARSE_MIN_BAND)):
        vU, vA = sided_thresholds(regs, sp_cap)
        for b in blk:
            b["vU"], b["vA"] = int(vU[b["cols"]].max()), int(vA[b["cols"]].min())

        def depth(b, v):
            return max(v - b["vU"], b["vA"] - v)

        def polarity(b, v):
            return 0 if v >= b["vU"] else 1 if v <= b["vA"] else 0

        listed = {}  # (block, plane) -> an item reads lists from it
        for t in tiles:
            bi, bj = blk[t["bi"]], blk[t["bj"]]
            pb, pe = t["Lp"] - pbase, t["T"] - pbase
            routed = [depth(bi, pbase + 1 + pl) >= 0 or depth(bj, pbase + 1 + pl) >= 0 for pl in range(pb, pe)]
            above = below = 0
            while above < pe - pb and routed[pe - pb - 1 - above]:
                above += 1
            while below + above < pe - pb and routed[below]:
                below += 1
            t["sparse"], t["below"] = above, below
            for pl in [pe - 1 - x for x in range(above)] + [pb + x for x in range(below)]:
                v = pbase + 1 + pl
                tr = t["bi"] != t["bj"] and depth(bj, v) > depth(bi, v)
                lb, tb = (bj, bi) if tr else (bi, bj)
                t["sided"].append((pl, polarity(lb, v), polarity(tb, v), int(tr)))
                for key, lists in (((t["bi"], pl), not tr), ((t["bj"], pl), tr or t["bi"] == t["bj"])):
                    listed[key] = listed.get(key, False) or lists
                sided_items += 1
                transposed += int(tr)
        table_slabs = sum(1 for x in listed.values() if not x)
    sparse_items = sum(t["sparse"] + t["below"] for t in tiles)
    plan = {"planes": P, "pbase": pbase, "kpad": (P * W + kc - 1) // kc * kc, "tiles": len(planes), "sum_tile_planes": int(sum(planes)),
            "avg_tile_planes_x100": int(sum(planes)) * 100 // len(planes), "cum_bytes": inst["CT"],
            "lockstep": int(inst["tile_kernel"] == "lockstep"), "sorted": int(bool(sort)),
            "sparse_items": sparse_items, "dense_planes": int(sum(planes)) - sparse_items, "sparse_sided_items": sided_items,
            "sparse_transposed_items": transposed, "sparse_table_slabs": table_slabs}
    return Census(inst, counts, plan, joins, tiles, blk)


# ---- the census of what the GPU suite runs (a report, not a test) ------------------------------------------------------
def instance_name(p, inst):
    return "p=%d CT=%d RK=%d %s" % (p, inst["CT"], inst["RK"], inst["tile_kernel"])


def fuzz_random_case(case):
    """the collection and list caps of tests/test_gpu_fuzz.py::test_random_case(case): the same draws in the same order (a
    comment there points here: change both together)"""
    import test_gpu_fuzz as tf

    rng = np.random.default_rng(1000 + case)
    p = int(rng.choice([4, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20]))
    n = int(rng.integers(2, 420 if p <= 12 else (180 if p <= 16 else 24)))
    kind = str(rng.choice(["law", "related", "uniform", "narrow"]))
    rng.integers(0, 3), rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8]), rng.choice([15, 21, 31, 32])  # estim, rt, k
    regs = tf._regs(rng, n, p, kind)
    if n > 4 and rng.random() < 0.5:
        regs[int(rng.integers(n))] = 0
        a, b = rng.choice(n, 2, replace=False)
        regs[a] = regs[b]
    emax = int(rng.choice([-1, -1, 0, 3, 17, 255]))
    elow = int(rng.choice([-1, -1, 0, 2, 40, 255]))
    return p, regs, (None if emax < 0 else emax), (None if elow < 0 else elow)


def suite_collections():
    """(source, p, regs, emax, elow, column orders) of the existing GPU suite's collections that need only the random
    streams and dashing_amd.synth"""
    from dashing_amd import synth
    import test_gpu_finalize_join as fj

    for case in range(100):
        p, regs, emax, elow = fuzz_random_case(case)
        yield "test_gpu_fuzz::test_random_case", p, regs, emax, elow, (True,)
    for k in range(40):
        p, regs = fj.fuzz_case(k)
        yield "test_gpu_finalize_join::fuzz_case", p, regs, None, None, (True,)
    for p in (10, 14, 16):
        for n in (129, 257, 300):
            yield "test_gpu_finalize_join::test_crowded_buckets", p, fj.near_duplicates(n, p, seed=1000 * p + n), None, None, (True,)
    for p, n in ((10, 127), (10, 128), (10, 129), (10, 300), (14, 130), (14, 260), (15, 40), (12, 97), (7, 70), (4, 33), (5, 40), (16, 20), (16, 140)):
        regs = synth.synthetic_sketches(n, p, seed=0x1234 + p * 131 + n)
        regs[n // 2] = regs[0]
        regs[n - 1] = 0
        yield "test_gpu_compare::test_tri_vs_oracle", p, regs, None, None, (True,)
    for p in (8, 11, 15):
        q = 64 - p
        rng = np.random.default_rng(p)
        m = 1 << p
        regs = rng.integers(0, q + 2, size=(140, m)).astype(np.uint8)
        regs[0], regs[1], regs[2] = q + 1, 7, 0
        regs[2, 5] = 9
        regs[3] = rng.integers(0, 3, size=m)
        regs[4] = rng.integers(q - 2, q + 2, size=m)
        yield "test_gpu_compare::test_adversarial_registers", p, regs, None, None, (True, False)


def new_file_collections():
    import path_cases as pc

    for run in pc.census_runs():
        yield "test_gpu_paths", run.p, run.regs(), run.emax, run.elow, (run.sort,)


def tally(collections):
    """instance name -> condition -> collections (x column order) that hold it; and the JSON records"""
    table, records = {}, []
    for source, p, regs, emax, elow, orders in collections:
        for sort in orders:
            c = census(regs, p, emax, elow, sort)
            row = table.setdefault((p, instance_name(p, c.instance)), dict.fromkeys(CONDITIONS, 0))
            row["_collections"] = row.get("_collections", 0) + 1
            for name in c.holds():
                row[name] += 1
            records.append({"source": source, "p": p, "n": int(regs.shape[0]), "emax": emax, "elow": elow, "sorted": bool(sort),
                            "instance": c.instance, "holds": sorted(c.holds()), "plan": c.plan, "joins": c.joins})
    return table, records


def markdown(title, table):
    insts = sorted(table)
    out = ["### " + title, "", "collections (x column order) that hold the condition, per instance; `.` = none", "",
           "| condition | " + " | ".join(name for _, name in insts) + " |", "|---|" + "---|" * len(insts),
           "| *collections replayed* | " + " | ".join(str(table[i]["_collections"]) for i in insts) + " |"]
    for name in CONDITIONS:
        out.append("| `%s` | " % name + " | ".join(str(table[i][name]) if table[i][name] else "." for i in insts) + " |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", action="store_true", help="one JSON line per replayed collection instead of the tables")
    ap.add_argument("--only", choices=("suite", "new"), help="one of the two tables")
    a = ap.parse_args()
    for title, gen in (("the existing GPU suite (fuzz streams, crowded buckets, the fixed collections of test_gpu_compare.py)", suite_collections),
                       ("tests/test_gpu_paths.py (tests/path_cases.py)", new_file_collections)):
        if a.only and (a.only == "suite") != (gen is suite_collections):
            continue
        table, records = tally(gen())
        if a.json:
            for r in records:
                print(json.dumps(r))
        else:
            print(markdown(title, table))


if __name__ == "__main__":
    main()
