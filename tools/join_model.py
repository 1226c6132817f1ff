#!/usr/bin/env python3
"""CPU model (numpy) of k_finalize's tail join for a collection of sketches: what a tile row looks up in its column
block's position index and what the look-ups find, counted per WAVE -- the unit that pays.

It rebuilds, from the registers and the two list caps alone,
  * the thresholds of k_selfhist_card (T: the largest upper tail of at most emax registers, L: the largest lower tail
    of at most elow registers below T) and the listed registers of every sketch,
  * the column order of plan::sort_rows_by_key (stable, by T, L, largest value) and the 128-column blocks,
  * the buckets of k_build_colindex ((position >> sh) * 2 + lower tail, the tail by the COLUMN's own thresholds),
  * the tile's dense range (plan::tile_planes) and, for sampled (row, column block) pairs, the look-ups of the row:
    lane e of round r holds entry 128 r + e of the row's list.
The rules are stated once, as functions (list_thresholds, key_order, listed, ColumnBlock, lookup_matches, row_lookups);
tools/path_census.py builds the census of the compare path's data-dependent branches on them.
Two things the device does not fix are assumptions here: the ORDER of a row's list (k_selfhist_card writes it lane by
lane, this model takes it in position order) and therefore which entries share a wave-round; the order inside a bucket
plays no part (a bucket is a set).

Prints one JSON line: the load per row, the per-lane walk that k_finalize had before the work queue ("walk": a wave
applies its RK inline entries and then as many further entries as its fullest bucket holds) and the queue form
("queue": every entry is one item, the lanes apply 64 items per pass).

  python tools/join_model.py --n 10000 --p 14            # bench.py's collection (synth.survey_sketches, seed 0x5EED0000)
  python tools/join_model.py --n 100000 --p 10 --rows 320
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TILE = 128
QUEUE_ITEMS = 128  # kJoinQ of kernels_compare.hip: items of a wave's queue


def auto_list_cap(p, upper):
    """plan::auto_list_cap"""
    return min(255 if upper else 200, (1 << p) >> 5)


def record_inline(p, E):
    """colindex_inline (kernels.h): entries a bucket's record holds inline"""
    return 7 if p <= 12 and E <= 256 else 3


def list_thresholds(regs, emax, elow):
    """per sketch: lo, hi, T, L as k_selfhist_card finds them, and the registers it lists above T and below L
    (regs: [n, 2^p] uint8)"""
    n = regs.shape[0]
    out = np.zeros((6, n), np.int64)
    for s in range(n):
        h = np.bincount(regs[s], minlength=64)[:64]
        nz = np.flatnonzero(h)
        a, b = int(nz[0]), int(nz[-1])
        t, cnt = b, 0
        while t > a and cnt + h[t] <= emax:
            cnt += h[t]
            t -= 1
        l, cntl = a, 0
        while l < t and cntl + h[l] <= elow:
            cntl += h[l]
            l += 1
        out[:, s] = a, b, t, l, cnt, cntl
    return tuple(out)


def thresholds(regs, emax, elow):
    """per sketch: lo, hi, T, L as k_selfhist_card finds them (regs: [n, 2^p] uint8)"""
    return list_thresholds(regs, emax, elow)[:4]


def key_order(hi, T, L):
    """plan::sort_rows_by_key: stable, by (T, L, largest value)"""
    return np.argsort((T << 12) | (L << 6) | hi, kind="stable")


def listed(row, T, L):
    """(positions, values) of a sketch's listed registers, in position order"""
    pos = np.flatnonzero((row > T) | (row < L))
    return pos, row[pos].astype(np.int64)


class ColumnBlock:
    """the position index of up to 128 sketches (k_build_colindex): entries sorted by bucket"""

    def __init__(self, regs, cols, T, L, p):
        sh = max(p - 14, 0)
        bk, jl, vb, pos = [], [], [], []
        for k, s in enumerate(cols):
            ps, vs = listed(regs[s], T[s], L[s])
            bk.append(((ps >> sh) << 1) | (vs <= T[s]))
            jl.append(np.full(len(ps), k, np.int64))
            vb.append(vs)
            pos.append(ps)
        self.bucket = np.concatenate(bk) if bk else np.zeros(0, np.int64)
        o = np.argsort(self.bucket, kind="stable")
        self.bucket = self.bucket[o]
        self.jl = np.concatenate(jl)[o]
        self.vb = np.concatenate(vb)[o]
        self.pos = np.concatenate(pos)[o]
        self.nbuckets = (1 << (p - sh)) * 2
        self.count = np.bincount(self.bucket, minlength=self.nbuckets)
        self.first = np.concatenate(([0], np.cumsum(self.count)))[:-1]
        self.T = int(T[cols].max())
        self.L = int(L[cols].min())


def lookup_matches(ps, vs, cb, Tt, Lp, p):
    """list entries (positions ps, values vs: of one row or of many) looked up in column block cb by a tile with the
    thresholds Tt and Lp.  Per entry: the bucket's entry count (-1: the entry is not looked up -- Tt itself and the dense
    range are never joined) and whether it is one of the upper tail; per (entry, entry of its bucket): e, the index into
    ps, and k, the index into cb's arrays"""
    sh = max(p - 14, 0)
    up = vs > Tt
    look = up | (vs < Lp)
    b = ((ps >> sh) << 1) | (~up).astype(np.int64)
    cnt = np.where(look, cb.count[b], -1).astype(np.int64)
    c = np.maximum(cnt, 0)
    e = np.repeat(np.arange(len(ps)), c)
    k = cb.first[b][e] + (np.arange(e.size) - np.repeat(np.cumsum(c) - c, c))
    return cnt, up, e, k.astype(np.int64)


def row_lookups(regs, s, T, L, lo, blk_row, blk_col, cb, p):
    """the look-ups of row sketch s in column block cb: per list entry (in list order) the bucket's entry count (-1: the
    entry is not looked up), the entries of its own position (the queue's items), those that pass the value filter, and
    whether the look-up is one of the upper tail"""
    Tt = max(blk_row["T"], blk_col["T"])
    Lp = max(max(blk_row["lo"], blk_col["lo"]), min(blk_row["L"], blk_col["L"]))
    ps, vs = listed(regs[s], T[s], L[s])
    cnt, up, e, k = lookup_matches(ps, vs, cb, Tt, Lp, p)
    same = cb.pos[k] == ps[e]
    live = same & np.where(up[e], cb.vb[k] > Tt, cb.vb[k] < Lp)
    items = np.bincount(e[same], minlength=len(ps)).astype(np.int64)
    applied = np.bincount(e[live], minlength=len(ps)).astype(np.int64)
    return cnt, items, applied, up


def model(regs, p, emax=None, elow=None, rows=320, seed=1, sort=True):
    n = regs.shape[0]
    emax = auto_list_cap(p, True) if emax is None else emax
    elow = auto_list_cap(p, False) if elow is None else elow
    E = max(1, emax + elow)
    RK = record_inline(p, E)
    lo, hi, T, L = thresholds(regs, emax, elow)
    order = key_order(hi, T, L) if sort else np.arange(n)
    nblk = (n + TILE - 1) // TILE
    blk = []
    for b in range(nblk):
        cols = order[b * TILE : (b + 1) * TILE]
        blk.append({"T": int(T[cols].max()), "L": int(L[cols].min()), "lo": int(lo[cols].min()), "cols": cols})
    rng = np.random.default_rng(seed)
    index = {}
    nlist, nlook, counts = [], [], []
    rounds_work, rounds_ovf, trips, lanes_busy, lane_slots = 0, 0, [], 0, 0
    applied_row, items_row, walk_exec, queue_passes, expansions, drains = [], [], 0, 0, 0, 0
    for _ in range(rows):
        bi = int(rng.integers(nblk))
        bj = int(rng.integers(bi, nblk))
        s = int(blk[bi]["cols"][int(rng.integers(len(blk[bi]["cols"])))])
        if bj not in index:
            index[bj] = ColumnBlock(regs, blk[bj]["cols"], T, L, p)
        cnt, items, applied, _ = row_lookups(regs, s, T, L, lo, blk[bi], blk[bj], index[bj], p)
        nlist.append(len(cnt))
        nlook.append(int((cnt >= 0).sum()))
        counts.append(cnt[cnt >= 0])
        applied_row.append(int(applied.sum()))
        items_row.append(int(items.sum()))
        for wave in (0, 1):
            queued = 0
            for r in range((E + 127) // 128):
                e0 = 128 * r + 64 * wave
                c = np.maximum(cnt[e0 : e0 + 64], 0)
                if len(c) == 0 or c.max() == 0:
                    continue
                rounds_work += 1
                over = np.maximum(c - RK, 0)
                rounds_ovf += int(over.max() > 0)
                trips.append(int(over.max()))
                ex = RK + int(over.max())
                walk_exec += ex
                lane_slots += 64 * ex
                lanes_busy += int(c.sum())
                expansions += int((over > 0).sum())
                queued += int(items[e0 : e0 + 64].sum())
            queue_passes += (queued + 63) // 64
            drains += max((queued + QUEUE_ITEMS - 1) // QUEUE_ITEMS, 1 if queued else 0)
    allc = np.concatenate(counts) if counts else np.zeros(0, np.int64)
    tr = np.array(trips if trips else [0])
    share = lambda m: round(float(m.mean()), 4) if len(allc) else 0.0
    return {
        "n": n, "p": p, "emax": emax, "elow": elow, "E": E, "RK": RK, "sorted": bool(sort), "rows_sampled": rows, "seed": seed,
        "listed_per_row": round(float(np.mean(nlist)), 2),
        "lookups_per_row": round(float(np.mean(nlook)), 2),
        "bucket_count_share": {"0": share(allc == 0), "1": share(allc == 1), "2": share(allc == 2), "3": share(allc == 3),
                               "gt3": share(allc > 3), "ge7": share(allc >= 7), "gt_RK": share(allc > RK)},
        "entries_applied_per_row": round(float(np.mean(applied_row)), 2),
        "items_per_row": round(float(np.mean(items_row)), 2),
        "walk": {
            "wave_rounds_with_work_per_row": round(rounds_work / rows, 3),
            "wave_rounds_entering_overflow": round(rounds_ovf / max(rounds_work, 1), 4),
            "overflow_trips_per_wave_round": {"mean": round(float(tr.mean()), 2), "median": float(np.median(tr)),
                                              "p90": float(np.percentile(tr, 90)), "max": int(tr.max())},
            "apply_per_wave_round": round(walk_exec / max(rounds_work, 1), 2),
            "apply_per_row": round(walk_exec / rows, 2),
            "lane_slots_busy": round(lanes_busy / max(lane_slots, 1), 4),
        },
        "queue": {
            "capacity": QUEUE_ITEMS,
            "apply_per_row": round(queue_passes / rows, 2),
            "bucket_expansions_per_row": round(expansions / rows, 2),
            "drains_per_row": round(drains / rows, 2),
        },
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--p", type=int, default=14)
    ap.add_argument("--seed", type=lambda x: int(x, 0), default=0x5EED0000, help="seed of synth.survey_sketches")
    ap.add_argument("--emax", type=int, default=None)
    ap.add_argument("--elow", type=int, default=None)
    ap.add_argument("--rows", type=int, default=320, help="sampled (row, column block) pairs")
    ap.add_argument("--sample-seed", type=int, default=1)
    ap.add_argument("--registers", help=".npy of [n, 2^p] uint8 registers instead of the synthetic collection")
    a = ap.parse_args()
    if a.registers:
        regs = np.load(a.registers)
        p = int(regs.shape[1]).bit_length() - 1
    else:
        from dashing_amd import synth

        regs = synth.survey_sketches(a.n, a.p, seed=a.seed)[0]
        p = a.p
    print(json.dumps(model(np.ascontiguousarray(regs, np.uint8), p, a.emax, a.elow, a.rows, a.sample_seed)))


if __name__ == "__main__":
    main()
