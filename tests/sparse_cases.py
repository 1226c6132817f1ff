"""Collections of tests/test_sparse_plane_model.py and tests/test_gpu_sparse_planes.py: the sparse outer planes of the
compare path (dashing_amd/csrc/plan.h, Tuning::sparse_planes; kernels_sparseplane.hip), and the model's view of them
(tools/path_census.py, tools/join_model.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import join_model as jm  # noqa: E402
import path_census as pcs  # noqa: E402
from dashing_amd import synth  # noqa: E402

KINDS = ("survey", "near_duplicates", "mixed_thresholds", "cap_boundary", "constant")


def thresholds(regs, p):
    """lo, hi, T, L and the counts g0, g1 of every sketch, as k_selfhist_card finds them under the default list caps"""
    lo, hi, T, L, _, _ = jm.list_thresholds(regs, jm.auto_list_cap(p, True), jm.auto_list_cap(p, False))
    g0, g1 = pcs.sparse_counts(regs, T)
    return lo, hi, T, L, g0, g1


def keys_and_counts(regs, p):
    """the per-sketch keys and the word next to them (g0 | g1 << 16), as the planner reads them"""
    lo, hi, T, L, g0, g1 = thresholds(regs, p)
    keys = (hi.astype(np.uint32) << 18) | (T.astype(np.uint32) << 12) | (L.astype(np.uint32) << 6) | lo.astype(np.uint32)
    return np.ascontiguousarray(keys, np.uint32), np.ascontiguousarray(g0.astype(np.uint32) | (g1.astype(np.uint32) << 16), np.uint32)


def near_duplicates(n, p, seed, changed=5):
    """one base sketch; copy g differs from it in `changed` registers: the sets of a pair are nearly the same set, the
    counters of the route run to the sets' full size"""
    base = synth.hll_registers(seed, 3_000_000, p)
    regs = np.repeat(base[None, :], n, axis=0)
    rng = np.random.default_rng(seed)
    top = 64 - p + 1
    for g in range(1, n):
        pos = rng.choice(1 << p, changed, replace=False)
        v = regs[g, pos].astype(np.int64) + rng.choice((-1, 1), changed)
        regs[g, pos] = np.clip(v, 0, top).astype(np.uint8)
    return regs


def mixed_thresholds(n, p, seed):
    """sketches of four cardinalities, a factor of two to thirty apart: thresholds one, two and many below the largest, so
    that the blocks at the borders of the key order mix sketches at the tile's T with sketches whose own T is below it --
    their sets come from the range of their lists, and those of the small ones are empty"""
    cards = (9_000_000, 4_500_000, 2_200_000, 300_000)
    return np.stack([synth.hll_registers(seed + 977 * g, cards[g % 4], p) for g in range(n)])


def cap_boundary(n, p, seed):
    """(regs, cap, odd): every sketch has exactly `cap` registers >= its T -- copies of one sketch that differ below T - 1
    only -- except sketch `odd`, which has cap + 1: with sparse_cap = cap its blocks' planes stay dense, the others' go"""
    base = synth.hll_registers(seed, 4_000_000, p)
    T = int(thresholds(base[None, :], p)[2][0])
    regs = np.repeat(base[None, :], n, axis=0)
    rng = np.random.default_rng(seed)
    low = np.flatnonzero((base < T - 1) & (base > 1))
    for g in range(1, n):
        pos = rng.choice(low, 7, replace=False)
        regs[g, pos] -= 1
    odd = n // 2
    regs[odd, np.flatnonzero(regs[odd] == T - 1)[0]] = T  # one more register at T: the same T, one more position
    _, _, Ts, _, g0, _ = thresholds(regs, p)
    cap = int(g0[0])
    assert (Ts == T).all() and int(g0[odd]) == cap + 1 and (np.delete(g0, odd) == cap).all(), (T, cap, g0[odd])
    return regs, cap, odd


def collection(kind, n, p):
    """(regs, sparse_cap or None for the default)"""
    seed = 0x5A0000 + 131 * p + n
    if kind == "survey":
        return synth.survey_sketches(n, p, seed=seed)[0], None
    if kind == "near_duplicates":
        return near_duplicates(n, p, seed), None
    if kind == "mixed_thresholds":
        return mixed_thresholds(n, p, seed), None
    if kind == "cap_boundary":
        regs, cap, _ = cap_boundary(n, p, seed)
        return regs, cap
    if kind == "constant":
        return np.full((n, 1 << p), 7, np.uint8), None
    raise ValueError(kind)
