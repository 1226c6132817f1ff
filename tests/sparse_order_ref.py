"""The launch order of the sparse items restated in numpy, and the host hook that returns the planner's
(tests/test_sparse_order.py, tests/test_sparse_emit.py, tests/test_gpu_sparse_schedule.py).

plan.cpp, order_sparse_items: the items of a band read the table of their TABLE BLOCK (the column block of their tile, the
row block of a transposed item).  Table blocks by item count descending (stable in block order); each to the least loaded
of eight lists (the lowest index on a tie); inside a list by (table block ascending, plane descending, ti + tj ascending),
stable in emission order; the eight lists interleaved one item at a time.  Emission order: the tiles of the band in launch
order, per tile the planes routed from the top of its range downwards, then those routed from the bottom upwards."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSPOSED = 1 << 10  # plan.h, kSpItemTransposed (flags sit above the plane in an item's second word)
NX = 8


def load():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    u64, i32, u32, vp = C.c_uint64, C.c_int, C.c_uint32, C.c_void_p
    lib.dshh_plan_sparse_items.argtypes = [u64, vp, vp, vp, u32, u64, u64, u32, i32, i32, u64, u32, i32, i32, u32, u32, i32, vp, vp, u64, vp, u64,
                                           vp, u64, vp, u64, vp, C.c_char_p, C.c_size_t]
    lib.dshh_plan_sparse_items.restype = i32
    return lib


def plan(lib, keys, gcnt, thr, p, thr_cap=1280, rb=0, re=None, nparts=1, want_parts=0, budget=8 << 30, ri=768, sp=-1, sd=-1, cap=None,
         max_slabs=0, two_step=0):
    """the plan of a triangle job as dshh_plan_sparse_items returns it: dict of tiles (nt, 6), bands (nb, 4), items (ni, 4),
    slabs (ns, 2), chunks (nt, 2) and the counts"""
    keys = np.ascontiguousarray(keys, np.uint32)
    n = len(keys)
    gcnt = None if gcnt is None else np.ascontiguousarray(gcnt, np.uint32)
    thr = None if thr is None else np.ascontiguousarray(thr, np.uint32)
    nt = (n + 127) // 128
    ntiles = nt * (nt + 1) // 2 + 1
    tiles = np.zeros((ntiles, 6), np.uint32)
    chunks = np.zeros((ntiles, 2), np.uint32)
    bands = np.zeros((ntiles, 4), np.uint64)
    items = np.zeros((64 * ntiles, 4), np.uint32)
    slabs = np.zeros((64 * nt + 1, 2), np.uint32)
    counts = np.zeros(9, np.uint64)
    err = C.create_string_buffer(512)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = lib.dshh_plan_sparse_items(n, ptr(keys), ptr(gcnt), ptr(thr), thr_cap, rb, n if re is None else re, nparts, want_parts, p, budget, ri, sp, sd,
                                    thr_cap if cap is None else cap, max_slabs, two_step, ptr(counts), ptr(tiles), len(tiles), ptr(bands), len(bands),
                                    ptr(items), len(items), ptr(slabs), len(slabs), ptr(chunks), err, 512)
    assert rc == 0, err.value.decode()
    c = [int(x) for x in counts]
    return {"tiles": tiles[: c[0]].copy(), "chunks": chunks[: c[0]].copy(), "bands": bands[: c[1]].astype(np.int64), "items": items[: c[2]].copy(),
            "slabs": slabs[: c[3]].copy(), "sided_items": c[4], "transposed_items": c[5], "table_slabs": c[6], "dense_items": c[7], "NT": c[8]}


def emission_order(tiles, band):
    """the items of one band as (tile in band, plane) in emission order, from the tiles' routed planes alone"""
    out = []
    for t in range(int(band[0]), int(band[1])):
        _, _, pb, pe, below, above = (int(x) for x in tiles[t])
        out += [(t - int(band[0]), pe - 1 - x) for x in range(above)] + [(t - int(band[0]), pb + x) for x in range(below)]
    return out


def launch_order(tiles, band, items):
    """the rule above applied to the items of one band GIVEN IN EMISSION ORDER (an (k, 4) array of the planner's words):
    the permutation that puts them into launch order"""
    k = len(items)
    if k <= 1:
        return np.arange(k)
    T = tiles[int(band[0]) + items[:, 0].astype(np.int64)]
    tblock = np.where(items[:, 1] & TRANSPOSED, T[:, 0], T[:, 1]).astype(np.int64)
    plane = (items[:, 1] & 0xFF).astype(np.int64)
    s = T[:, 0].astype(np.int64) + T[:, 1].astype(np.int64)
    blocks, per_block = np.unique(tblock, return_counts=True)  # (ascending)
    by_count = blocks[np.argsort(-per_block, kind="stable")]
    count_of = dict(zip(blocks.tolist(), per_block.tolist()))
    load, list_of = [0] * NX, {}
    for b in by_count.tolist():
        x = min(range(NX), key=lambda y: (load[y], y))
        list_of[b] = x
        load[x] += count_of[b]
    lst = np.array([list_of[b] for b in tblock.tolist()])
    lists = []
    for x in range(NX):
        idx = np.flatnonzero(lst == x)
        o = np.lexsort((s[idx], -plane[idx], tblock[idx]))  # (stable; the last key is the first compared)
        lists.append(idx[o])
    order = []
    for r in range(max(len(l) for l in lists)):
        order += [int(l[r]) for l in lists if r < len(l)]
    return np.array(order, np.int64)


def emission_sorted(tiles, band, items):
    """the items of a band put back into emission order (every (tile, plane) of a band has one item): the input of
    launch_order"""
    pos = {tp: i for i, tp in enumerate(emission_order(tiles, band))}
    got = [pos[(int(it[0]), int(it[1]) & 0xFF)] for it in items]
    assert sorted(got) == list(range(len(pos))), "the band's items are not one per routed (tile, plane)"
    return items[np.argsort(np.array(got, np.int64), kind="stable")] if len(items) else items
