"""k_finalize's tail join through the wave's work queue (kernels_compare.hip, join_tails of finalize_block): crowded buckets -- more
entries than a record holds inline, more than one wave-wide read of ent[], more items than the queue holds -- both
tails, empty lists, and every call form, against the oracle (|d| <= 1e-6 * max(|ref|, 1e-9)) and byte for byte against
the full call of the same context.  The conditions a collection is chosen for are asserted on the host first, with
the numpy model of the join (tools/join_model.py), for the key-ordered and for the identity column order."""
import os
import sys

import numpy as np
import pytest

import dashing_amd
from dashing_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import join_model as jm  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-6


def close(got, ref):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all()
    err = np.abs(got[fin] - ref[fin])
    tol = RTOL * np.maximum(np.abs(ref[fin]), 1e-9)
    bad = err > tol
    assert not bad.any(), "max rel err %.3g at %d of %d" % (
        (err / np.maximum(np.abs(ref[fin]), 1e-9)).max(), int(bad.sum()), err.size)


def near_duplicates(n, p, seed, changed=5):
    """one base sketch; copy g differs from it in `changed` registers (a legal value one off the base's)"""
    base = synth.hll_registers(seed, 3_000_000, p)
    regs = np.repeat(base[None, :], n, axis=0)
    rng = np.random.default_rng(seed)
    top = 64 - p + 1
    for g in range(1, n):
        pos = rng.choice(1 << p, changed, replace=False)
        v = regs[g, pos].astype(np.int64) + rng.choice((-1, 1), changed)
        regs[g, pos] = np.clip(v, 0, top).astype(np.uint8)
    return regs


def join_load(regs, p, emax=None, elow=None):
    """What the join meets in this collection, for the key-ordered and the identity column order (the smaller of the two
    where they differ): the fullest bucket of a column block, the largest number of queue items one tile row brings per
    wave-round (items / (2 waves x rounds): some wave-round holds at least that many, whatever the order of the list),
    and the entries applied per tail."""
    n = regs.shape[0]
    emax = jm.auto_list_cap(p, True) if emax is None else emax
    elow = jm.auto_list_cap(p, False) if elow is None else elow
    E = max(1, emax + elow)
    lo, hi, T, L = jm.thresholds(regs, emax, elow)
    out = None
    for order in (jm.key_order(hi, T, L), np.arange(n)):
        blk = []
        for b in range((n + 127) // 128):
            cols = order[b * 128 : (b + 1) * 128]
            blk.append({"T": int(T[cols].max()), "L": int(L[cols].min()), "lo": int(lo[cols].min()), "cols": cols})
        idx = [jm.ColumnBlock(regs, b["cols"], T, L, p) for b in blk]
        fullest = max(int(ix.count.max()) for ix in idx)
        per_round, upper, lower = 0.0, 0, 0
        for bi in range(len(blk)):
            for s in blk[bi]["cols"][:: max(len(blk[bi]["cols"]) // 4, 1)]:  # a few rows of every block
                for bj in range(bi, len(blk)):
                    cnt, items, applied, up = jm.row_lookups(regs, int(s), T, L, lo, blk[bi], blk[bj], idx[bj], p)
                    per_round = max(per_round, items.sum() / (2.0 * ((E + 127) // 128)))
                    upper += int(applied[up].sum())
                    lower += int(applied[~up].sum())
        cur = {"fullest": fullest, "per_round": per_round, "upper": upper, "lower": lower, "RK": jm.record_inline(p, E)}
        out = cur if out is None else {k: min(out[k], cur[k]) for k in cur}
    return out


_crowded = {}


def crowded(n, p):
    """the near-duplicate collection of a shape, its join load and the oracle's triangle: computed once, never changed"""
    if (n, p) not in _crowded:
        from oracle import oracle_c

        regs = near_duplicates(n, p, seed=1000 * p + n)
        regs.setflags(write=False)
        ref = oracle_c.dist_tri(regs)
        ref.setflags(write=False)
        _crowded[(n, p)] = (regs, join_load(regs, p), ref)
    return _crowded[(n, p)]


@pytest.mark.parametrize("p", [10, 14, 16])  # RK = 7; RK = 3; the position-group check (sh = 2) and 32-bit counts
@pytest.mark.parametrize("n", [129, 257, 300])  # a diagonal tile, ragged last blocks, lanes without a pair
def test_crowded_buckets(ctx, oracle, n, p):
    regs, load, ref = crowded(n, p)
    assert load["fullest"] > load["RK"], load            # a bucket beyond its record: the wave expands it
    assert load["fullest"] > 64 + load["RK"], load       # beyond one wave-wide read of ent[]: further passes
    assert load["per_round"] > jm.QUEUE_ITEMS, load      # some wave-round brings more than the queue holds: drains mid-round
    assert load["upper"] > 0 and (p > 14 or load["lower"] > 0), load  # (p = 16: near-duplicates share no register below Lp)
    ctx.set_sketches(regs)
    got = ctx.dist_rows()
    close(got, ref)
    # the same rows as a range (its own layout) and with the dense-only histogram: byte for byte
    lo_, hi_ = dashing_amd.tri_span(n, 0, 5), dashing_amd.tri_span(n, 0, n - 2)
    assert ctx.dist_rows(5, n - 2).tobytes() == got[lo_:hi_].tobytes()
    try:
        ctx.set_option("emax", 0)
        ctx.set_option("elow", 0)
        assert ctx.dist_rows().tobytes() == got.tobytes()
    finally:
        ctx.set_option("emax", -1)
        ctx.set_option("elow", -1)


def test_both_tails_and_empty_lists(ctx, oracle):
    """rows that join in the upper tail only, in the lower tail only, in both, and not at all (empty lists): the list
    caps through set_option, 0 and small values, on related sketches and on near-duplicates"""
    p = 14
    for regs in (synth.related_sketches(140, p, seed=77)[0], np.concatenate((near_duplicates(100, p, seed=5), synth.synthetic_sketches(40, p, seed=6)))):
        ref = oracle.dist_tri(regs)
        both = join_load(regs, p)
        assert both["upper"] > 0 and both["lower"] > 0, both
        only_up, only_low = join_load(regs, p, 255, 0), join_load(regs, p, 0, 200)
        assert only_up["upper"] > 0 and only_up["lower"] == 0 and only_low["lower"] > 0 and only_low["upper"] == 0
        none = join_load(regs, p, 0, 0)
        assert none["upper"] == 0 and none["lower"] == 0 and none["fullest"] == 0
        ctx.set_sketches(regs)
        base = ctx.dist_rows()
        close(base, ref)
        try:
            for elow, emax in ((0, 0), (0, -1), (-1, 0), (0, 3), (3, 0), (7, 3), (1, 64), (200, 1), (-1, -1)):
                ctx.set_option("elow", elow)
                ctx.set_option("emax", emax)
                assert ctx.dist_rows().tobytes() == base.tobytes(), (elow, emax)
        finally:
            ctx.set_option("elow", -1)
            ctx.set_option("emax", -1)


@pytest.mark.parametrize("p", [10, 14])
def test_call_forms_agree_byte_for_byte(ctx, oracle, p):
    """the instances of k_finalize at one crowded collection: the plain triangle (full, a row range), GENERAL (a
    rectangle, the square and the banded nearest-neighbour call, row-sorted parts) and the signalling instance
    (dsh_dist_rows_parts_device_async), each against the full call of the same context"""
    import torch

    n = 300
    regs, load, _ = crowded(n, p)
    assert load["fullest"] > 64 + load["RK"] and load["per_round"] > jm.QUEUE_ITEMS, load
    ctx.set_sketches(regs)
    full = ctx.dist_rows()
    sq = np.zeros((n, n), np.float32)
    iu = np.triu_indices(n, 1)
    sq[iu] = full
    sq.T[iu] = full
    for rb, re in ((0, 130), (37, 211), (129, n)):
        a, b = dashing_amd.tri_span(n, 0, rb), dashing_amd.tri_span(n, 0, re)
        assert ctx.dist_rows(rb, re).tobytes() == full[a:b].tobytes(), (rb, re)
    rect = ctx.dist_rect(3, 140, 150, n)
    assert rect.tobytes() == np.ascontiguousarray(sq[3:140, 150:n]).tobytes()
    rect = ctx.dist_rect(131, n, 0, 129)
    assert rect.tobytes() == np.ascontiguousarray(sq[131:n, 0:129]).tobytes()
    for budget in (96 << 30, 0):  # the square, then bands of query rows
        ctx.set_option("knn_square_budget_bytes", budget)
        try:
            gi, gv = ctx.knn(9)
        finally:
            ctx.set_option("knn_square_budget_bytes", 96 << 30)
        assert (gi < n).all() and (gi != np.arange(n)[:, None]).all()
        assert gv.tobytes() == np.ascontiguousarray(sq[np.arange(n)[:, None], gi]).tobytes(), budget
    dev = torch.device("cuda", 0)
    for sort_min in (1024, 1):  # (1: the parts of a short range come row-sorted -- the sorted-output form)
        ctx.set_option("range_sort_min_rows", sort_min)
        try:
            for rb, re, nparts in ((0, n, 1), (0, n, 3), (37, 290, 2)):
                a, span = dashing_amd.tri_span(n, 0, rb), dashing_amd.tri_span(n, rb, re)
                out = torch.full((span,), -3.0, dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                ctx.dist_rows_parts_device_async(out.data_ptr(), rb, re, nparts)
                ctx.wait()
                assert out.cpu().numpy().tobytes() == full[a : a + span].tobytes(), (sort_min, rb, re, nparts)
        finally:
            ctx.set_option("range_sort_min_rows", 1024)


@pytest.mark.parametrize("p", [10, 14])  # bucket records with 7 inline entries; with 3
def test_timed_instance_returns_the_same_bytes(ctx, oracle, p):
    """the stamped instance (option finalize_timing under profiling, as tools/finalize_probe.py sets it) at a crowded
    collection with a diagonal tile, off-diagonal tiles and a padded last block: the same bytes as the plain instance,
    and some wave reported its phases"""
    n = 300
    regs, load, _ = crowded(n, p)
    assert load["RK"] == (7 if p == 10 else 3), load
    ctx.set_sketches(regs)
    plain = ctx.dist_rows()
    ctx.set_profiling(True)
    try:
        ctx.set_option("finalize_timing", 1)
        timed = ctx.dist_rows()
        cycles = ctx.finalize_phase_cycles()
    finally:
        ctx.set_option("finalize_timing", 0)
        ctx.set_profiling(False)
    assert timed.tobytes() == plain.tobytes()
    assert cycles[6] > 0, cycles  # waves counted


def fuzz_case(k):
    rng = np.random.default_rng(0xF00D + k)
    p = (8, 10, 12, 14, 16)[k % 5]
    n = int(rng.integers(2, 301 if p < 16 else 161))
    kind = int(rng.integers(4))
    if kind == 0:
        regs = synth.synthetic_sketches(n, p, seed=900 + k)
    elif kind == 1:
        regs = synth.related_sketches(n, p, seed=900 + k)[0]
    elif kind == 2:
        regs = near_duplicates(n, p, seed=900 + k, changed=int(rng.integers(1, 40)))
    else:  # a few groups of near-duplicates of different size
        parts, left, g = [], n, 0
        while left:
            c = int(min(left, rng.integers(1, 140)))
            parts.append(near_duplicates(c, p, seed=7000 + 31 * k + g, changed=int(rng.integers(1, 12))))
            left -= c
            g += 1
        regs = np.concatenate(parts)[rng.permutation(n)]
    return p, np.ascontiguousarray(regs)


@pytest.mark.parametrize("chunk", range(4))
def test_seeded_fuzz_against_the_oracle(ctx, oracle, chunk):
    """40 small cases (n <= 300, p in 8 .. 16; ten per test): independent, related and near-duplicate sketches"""
    for k in range(10 * chunk, 10 * chunk + 10):
        p, regs = fuzz_case(k)
        ctx.set_sketches(regs)
        got = ctx.dist_rows()
        close(got, oracle.dist_tri(regs))
        n = regs.shape[0]
        if n > 4:
            a, b = dashing_amd.tri_span(n, 0, 1), dashing_amd.tri_span(n, 0, n - 1)
            assert ctx.dist_rows(1, n - 1).tobytes() == got[a:b].tobytes(), (k, n, p)
