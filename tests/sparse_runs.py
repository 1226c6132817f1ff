"""The runs of the LDS placement of the sparse counting kernel (dashing_amd/csrc/kernels_sparseplane.hip,
k_sparse_count_lds; plan.h, sparse_table_fills), restated in numpy for tests/test_sparse_runs_model.py and
tests/test_gpu_sparse_runs.py.  Items are the rows of test_sparse_sided_model.plan: (tile, plane, flags, slab of the row
block, slab of the column block), flags = list A | table A << 1 | transposed << 2, in launch order, of ONE launch (a band)."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSPOSED = 4
RUNS = (1, 2, 3, 8, 64)


def table_slab(items):
    items = np.asarray(items, np.int64).reshape(-1, 5)
    return np.where(items[:, 2] & TRANSPOSED, items[:, 3], items[:, 4])


def runs(n, run):
    """the item indices of every workgroup run: residue x of 8, `run` of its items one behind the other"""
    return [np.arange(x, n, 8)[a : a + run] for x in range(min(n, 8)) for a in range(0, len(range(x, n, 8)), run)]


def fills(items, run):
    """a table word is staged at the start of a run and wherever the table slab changes inside it; four words a table"""
    ts = table_slab(items)
    return 4 * sum(1 + int((ts[r][1:] != ts[r][:-1]).sum()) for r in runs(len(ts), run))


def conditions(items, run):
    """what the runs of these items at `run` hold, by name"""
    items = np.asarray(items, np.int64).reshape(-1, 5)
    ts, tr = table_slab(items), (items[:, 2] & TRANSPOSED) != 0
    got = dict.fromkeys(("slab_change", "transposed_then_plain", "plain_then_transposed", "ragged", "single", "whole_residue"), False)
    rs = runs(len(items), run)
    got["whole_residue"] = len(rs) == min(len(items), 8) and len(items) > 8
    for r in rs:
        same = ts[r][1:] == ts[r][:-1]
        got["slab_change"] |= bool((~same).any())
        got["transposed_then_plain"] |= bool((same & tr[r][:-1] & ~tr[r][1:]).any())
        got["plain_then_transposed"] |= bool((same & ~tr[r][:-1] & tr[r][1:]).any())
        got["ragged"] |= 1 < len(r) < run  # (the launch ends inside the run: the kernel's loop leaves at the item count)
        got["single"] |= len(r) == 1
    return got


def words(items):
    """the four words of every item as the device list holds them: {tile, plane | flags << 8, slab, slab}"""
    items = np.asarray(items, np.uint32).reshape(-1, 5)
    return np.ascontiguousarray(np.stack([items[:, 0], items[:, 1] | (items[:, 2] << 8), items[:, 3], items[:, 4]], axis=1), np.uint32)


def host_fills(host, items, run):
    """plan::sparse_table_fills through the C interface of the host library"""
    w = words(items)
    host.dshh_sparse_table_fills.restype = C.c_uint64
    host.dshh_sparse_table_fills.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
    return int(host.dshh_sparse_table_fills(w.ctypes.data if len(w) else None, len(w), run))
