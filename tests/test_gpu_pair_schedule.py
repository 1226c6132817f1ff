"""GPU: the lockstep tile kernel (k_pair_counts_ls<KC, CT, FRAG, GROUPS>) computes the same integers with three work items
per 768-thread workgroup (the default) as with two per 512-thread workgroup (the reference arm, option pair_groups = 2).

"pair_groups" only changes how the AND + popcount work is scheduled: how many groups of four waves share a workgroup, its
barriers and a CU.  For every case the reference arm is held once to the CPU oracle (1e-6 relative, the `close` rule of
test_gpu_compare.py); three groups must then give the reference arm's bytes at the same k-rows per LDS stage (kc = 16:
three groups do not exist at kc = 32), and the reference arm at kc = 32 the same bytes again.

What each shape is for:
  (9, 16), (10, 32)    a plane is ONE chunk (a flush after every chunk);  (10, 16): two chunks per plane
  n = 2, 129, 300      one pair; a ragged last block; 1, 3 and 6 tiles: item counts 1, 2 and 0 modulo 3 (and 0, 1 modulo 2)
                       leave groups of the last workgroup without an item, idling at the barriers
  n = 257              6 tiles at another plane count
  (14, 130)            W = 512: several chunks per plane at both kc; nsplit = 3: unequal item lengths inside a workgroup
  (16, 20)             32-bit counts (store8 / add8 of eight words)
  overflow_frag_permille = 0 | 1000   whole items only | the FRAG instance as well: info("frag_items") says which ran
                       (a plane of one chunk cannot be cut, and nsplit switches fragments off: plan.cpp, plan_fragments)
"""
import numpy as np
import pytest

import dashing_amd
from dashing_amd import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-6
REF = 2         # pair_groups of the reference arm
ARMS = [3]      # every other arm the library has (three groups: kc = 16 only)


def close(got, ref):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all()
    err = np.abs(got[fin] - ref[fin])
    tol = RTOL * np.maximum(np.abs(ref[fin]), 1e-9)
    bad = err > tol
    assert not bad.any(), "max rel err %.3g at %d of %d" % ((err / np.maximum(np.abs(ref[fin]), 1e-9)).max(), int(bad.sum()), err.size)


def set_arm(ctx, groups, kc):
    ctx.set_option("kc", kc)
    ctx.set_option("pair_groups", groups)


def restore(ctx):
    for name, v in (("pair_groups", 0), ("kc", 0), ("nsplit", 0), ("overflow_frag_permille", 500),
                    ("cum_budget_bytes", 8 << 30)):
        ctx.set_option(name, v)


CASES = [  # p, n, kcs, nsplit
    (9, 129, (16,), 0),
    (10, 2, (16, 32), 0),
    (10, 129, (16, 32), 0),
    (10, 257, (16, 32), 0),
    (10, 300, (16, 32), 0),
    (14, 130, (16, 32), 0),
    (14, 130, (16, 32), 3),
    (16, 20, (16, 32), 0),
]


@pytest.mark.parametrize("p,n,kcs,nsplit", CASES)
def test_every_schedule_gives_the_reference_arms_bytes(ctx, oracle, p, n, kcs, nsplit):
    regs = synth.synthetic_sketches(n, p, seed=7100 + 17 * p + n)
    ctx.set_sketches(regs)
    want = oracle.dist_tri(regs)
    W = (1 << p) // 32
    try:
        ctx.set_option("nsplit", nsplit)
        first = None
        for kc in kcs:
            for permille in (0, 1000):
                ctx.set_option("overflow_frag_permille", permille)
                set_arm(ctx, REF, kc)
                base = ctx.dist_rows()
                assert (ctx.info("pair_groups"), ctx.info("kc"), ctx.info("lockstep")) == (2, kc, 1)
                # neither instance may be skipped silently: fragments exist exactly where a plane can be cut
                frags_possible = permille == 1000 and W // kc >= 2 and nsplit == 0
                assert (ctx.info("frag_items") > 0) == frags_possible, (kc, permille, ctx.info("frag_items"))
                if first is None:
                    close(base, want)
                    first = base
                assert base.tobytes() == first.tobytes(), (kc, permille)
                for arm in ARMS:
                    if arm == 3 and kc != 16:
                        continue
                    set_arm(ctx, arm, kc)
                    got = ctx.dist_rows()
                    assert (ctx.info("pair_groups"), ctx.info("kc"), ctx.info("lockstep")) == (arm, kc, 1)
                    assert (ctx.info("frag_items") > 0) == frags_possible, (arm, kc, permille)
                    assert got.tobytes() == base.tobytes(), (arm, kc, permille)
    finally:
        restore(ctx)


def test_several_bands_and_a_row_range_through_every_schedule(ctx, oracle):
    p, n = 10, 300
    regs = synth.synthetic_sketches(n, p, seed=7100 + 17 * p + n)
    ctx.set_sketches(regs)
    try:
        for kc in (16, 32):
            set_arm(ctx, REF, kc)
            full = ctx.dist_rows()
            lo = dashing_amd.tri_span(n, 0, 5)
            ctx.set_option("cum_budget_bytes", 1 << 21)
            for arm in [REF] + ARMS:
                if arm == 3 and kc != 16:
                    continue
                set_arm(ctx, arm, kc)
                assert ctx.dist_rows().tobytes() == full.tobytes(), (arm, kc)
                assert ctx.info("bands") > 1
                part = ctx.dist_rows(5, n - 3)
                assert part.tobytes() == full[lo : lo + part.size].tobytes(), (arm, kc)
            ctx.set_option("cum_budget_bytes", 8 << 30)
        close(full, oracle.dist_tri(regs))
    finally:
        restore(ctx)


def test_auto_runs_three_groups_on_large_bands_and_two_on_small_ones(ctx):
    """the default: bands of more than 1 024 work items run three per workgroup in rounds of 768, smaller ones keep two
    in rounds of 512 (plan.h, Tuning::small_round_items) -- the reference arm's bytes either way, and overflow fragments
    planned at the round the band runs in"""
    p = 10
    try:
        for n, large in ((300, False), (2000, True)):
            regs = synth.synthetic_sketches(n, p, seed=7100 + 17 * p + n)
            ctx.set_sketches(regs)
            set_arm(ctx, REF, 16)
            base = ctx.dist_rows()
            assert ctx.info("pair_round") == 512
            set_arm(ctx, 3, 16)
            assert ctx.dist_rows().tobytes() == base.tobytes() and ctx.info("pair_round") == 768
            set_arm(ctx, 0, 0)
            for permille in (0, 1000):
                ctx.set_option("overflow_frag_permille", permille)
                got = ctx.dist_rows()
                assert (ctx.info("pair_groups"), ctx.info("kc"), ctx.info("bands")) == (3, 16, 1)
                items, frags = ctx.info("items"), ctx.info("frag_items")
                assert (items - frags // 2 > 1024) == large, (items, frags)
                assert ctx.info("pair_round") == (768 if large else 512)
                if permille == 0:
                    assert frags == 0
                elif not large:
                    assert 0 < frags == items <= 512, (items, frags)   # a band below a round of two is all fragments
                elif frags:
                    assert (items - frags) % 768 == 0 and frags <= 768, (items, frags)
                assert got.tobytes() == base.tobytes(), (n, permille)
    finally:
        restore(ctx)


def test_option_values_are_checked(ctx):
    try:
        for name, bad in (("pair_groups", 1), ("pair_groups", 4), ("pair_groups", -1), ("pair_rows", 2)):
            with pytest.raises(dashing_amd.DshError):
                ctx.set_option(name, bad)
    finally:
        restore(ctx)


def test_three_groups_refuse_long_stages_and_auto_follows_kc(ctx):
    """three groups exist at 16-row stages only: asked for together with kc = 32 the call fails.  Left to auto, the
    library runs three groups at kc = 16 -- and two where the caller asks for kc = 32."""
    regs = synth.synthetic_sketches(140, 12, seed=7)
    ctx.set_sketches(regs)
    try:
        set_arm(ctx, REF, 0)
        base = ctx.dist_rows()
        assert (ctx.info("pair_groups"), ctx.info("kc")) == (2, 32)
        set_arm(ctx, 3, 32)
        with pytest.raises(dashing_amd.DshError):
            ctx.dist_rows()
        for groups, kc, want in ((3, 0, (3, 16)), (0, 0, (3, 16)), (0, 16, (3, 16)), (0, 32, (2, 32)), (3, 16, (3, 16))):
            set_arm(ctx, groups, kc)
            assert ctx.dist_rows().tobytes() == base.tobytes(), (groups, kc)
            assert (ctx.info("pair_groups"), ctx.info("kc")) == want, (groups, kc)
    finally:
        restore(ctx)
