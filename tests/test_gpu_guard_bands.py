"""GPU: every entry point that stores through a caller's pointer writes the caller's span and nothing else.  Each buffer
is a guard.Guarded -- canaries in front and behind, sized by the whole packed triangle plus one tile row so that a store at
a full-triangle position of a range call lands in a guard and not outside the allocation --, each case runs at a 16-byte
aligned start and at one moved by 1..3 items, and asserts (a) guards intact, (b) no span element left unwritten, (c) the
span's bytes equal the context's own dense result (which is held to the oracle once per precision here).  What the helper
detects is proven on the CPU (tests/test_guard.py); on the device only by a torch write of the test's own into a guard."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import ctx_model
import dashing_amd
import knn_ref
from dashing_amd import synth
from guard import Guarded, GuardError, guard_items
from test_gpu_compare import close  # (the 1e-6 relative rule between GPU and oracle values)

pytestmark = pytest.mark.gpu

D = dashing_amd
DEV = "cuda:0"
NS = (1, 2, 127, 128, 129, 257, 300)
PS = (8, 10, 14, 16)  # free-running k_pair_counts | lock-step, 32-byte records | 16-byte records | uint32 cum
SHAPES = [(n, p) for p in PS for n in NS if p < 16 or n <= 140]
ORACLE_SHAPES = {(300, 8), (300, 10), (300, 14), (129, 16)}  # one (n, p) per p also meets the oracle
ALL_TYPES = (0, 1, 2, 3, 4, 5, 6, 7, 8)
F32, U32, U8 = np.float32, np.uint32, np.uint8


@functools.lru_cache(maxsize=None)
def collection(n, p):
    """the collection of test_tri_vs_oracle: one duplicated and one all-zero row"""
    regs = synth.synthetic_sketches(n, p, seed=0x1234 + p * 131 + n)
    if n > 3:
        regs[n // 2] = regs[0]
        regs[n - 1] = 0
    regs.setflags(write=False)
    return regs


def fbuf(items, n, mis, dtype=F32, device=DEV):
    g = guard_items(n)
    return Guarded(items, dtype, g, g, mis, device)


def verify(g, want, what):
    """the three checks of every case"""
    g.check(str(what))
    assert g.unwritten() == 0, (what, "span elements never written", g.unwritten(), g.n_items)
    want = np.ascontiguousarray(want).reshape(-1)
    got = g.host()
    assert got.size == want.size, what
    ne = np.flatnonzero(got.view(g.itype) != want.view(g.itype))
    assert ne.size == 0, (what, "%d of %d differ, first at %d" % (ne.size, got.size, ne[0] if ne.size else -1))


def untouched(g, want, what):
    """an input buffer: guards intact and the bytes it was given"""
    g.check(str(what))
    assert g.host().tobytes() == np.ascontiguousarray(want).tobytes(), (what, "an input was modified")


def ranges_of(n):
    """first row, last row (no pair: nothing may be written), a middle range, one that ends inside a tile row"""
    r = [(0, 1), (n - 1, n)]
    if n > 8:
        r.append((5, n - 3))
    if n > 4:
        r.append((2, n // 2 + 1) if n <= 130 else (2, 130))
    return r


def run_rows(ctx, n, full, rb, re, mis, asyn, what, **kw):
    lo, span = D.tri_span(n, 0, rb), D.tri_span(n, rb, re)
    g = fbuf(span, n, mis)
    if asyn:
        ctx.dist_rows_device_async(g.ptr, rb, re, **kw)
        ctx.wait()
    else:
        ctx.dist_rows_device(g.ptr, rb, re, **kw)
    verify(g, full[lo : lo + span], ("rows", what, n, rb, re, mis, asyn))


# ---- the detection itself, once, by the harness's own in-bounds action ----------------------------------------------
def test_a_torch_write_into_a_guard_is_reported(ctx):
    import torch

    for dtype in (F32, U32, U8):
        g = Guarded(100, dtype, 256, 256, 1, DEV)
        g.check()
        assert g.unwritten() == 100
        g.buf[g.front + 100 + 7] = 1  # the 8th element behind the span
        g.buf[g.front - 2] = 1
        torch.cuda.synchronize()
        with pytest.raises(GuardError) as e:
            g.check("self-check")
        assert (e.value.first, e.value.last, e.value.count) == (-2, 107, 2)
    g = Guarded(10, F32, 64, 64, 3, DEV)
    g.span()[4] = 1.0  # one float into the SPAN: no guard hit, one element fewer unwritten
    g.check()
    assert g.unwritten() == 9
    g.buf.view(torch.float32)[g.front + 10] = 2.5  # one float into the guard
    with pytest.raises(GuardError) as e:
        g.check()
    assert (e.value.first, e.value.count) == (10, 1)


# ---- dist_rows_device / dist_rows_device_async -------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", SHAPES)
def test_rows_full_triangle_and_ranges(ctx, oracle, n, p):
    regs = collection(n, p)
    ctx.set_sketches(regs)
    full = ctx.dist_rows()
    assert full.size == n * (n - 1) // 2
    if (n, p) in ORACLE_SHAPES:  # the reference of every case below meets the oracle here
        close(full, oracle.dist_tri(np.array(regs), 2, D.JI, 31))
    case = 0
    for asyn in (False, True):
        for mis in (0, 1 + (n + asyn) % 3):
            run_rows(ctx, n, full, 0, n, mis, asyn, "full")
    try:
        for min_rows in (1024, 1):  # identity layout | the layout built for the range (key-ordered)
            ctx.set_option("range_sort_min_rows", min_rows)
            for rb, re in ranges_of(n):
                for mis in (0, 1 + case % 3):
                    run_rows(ctx, n, full, rb, re, mis, bool(case & 1), "min_rows=%d" % min_rows)
                case += 1
    finally:
        ctx.set_option("range_sort_min_rows", 1024)


@pytest.mark.parametrize("p", PS)
def test_rows_in_several_bands(ctx, p):
    n = 300 if p < 16 else 129
    ctx.set_sketches(collection(n, p))
    full = ctx.dist_rows()
    try:
        ctx.set_option("cum_budget_bytes", 1 << 21)
        for mis, asyn in ((0, False), (1 + p % 3, True)):
            run_rows(ctx, n, full, 0, n, mis, asyn, "bands")
            run_rows(ctx, n, full, 5, n - 3, mis, not asyn, "bands")
        print("p=%d n=%d: %d bands" % (p, n, ctx.info("bands")))
    finally:
        ctx.set_option("cum_budget_bytes", 8 << 30)


# ---- dist_rows_parts_device_async ------------------------------------------------------------------------------------
def run_parts(ctx, n, full, rb, re, nparts, mis, what, **kw):
    lo, span = D.tri_span(n, 0, rb), D.tri_span(n, rb, re)
    g = fbuf(span, n, mis)
    ctx.dist_rows_parts_device_async(g.ptr, rb, re, nparts, **kw)
    ctx.wait()
    verify(g, full[lo : lo + span], ("parts", what, n, rb, re, nparts, mis))


@pytest.mark.parametrize("n,p", [(n, p) for n, p in SHAPES if n >= 127])
def test_rows_in_parts(ctx, n, p):
    ctx.set_sketches(collection(n, p))
    full = ctx.dist_rows()
    case = 0
    try:
        ctx.set_option("range_sort_min_rows", 1)
        for band_tiles in (1, 2048):
            ctx.set_option("part_band_tiles", band_tiles)
            for nparts in (2, 3, 5):
                for rb, re in ((0, n), (5, n - 3)):
                    for mis in (0, 1 + case % 3):
                        run_parts(ctx, n, full, rb, re, nparts, mis, "part_band_tiles=%d" % band_tiles)
                    case += 1
    finally:
        ctx.set_option("range_sort_min_rows", 1024)
        ctx.set_option("part_band_tiles", 2048)


# ---- shards of the sorted order, the three un-permutes ------------------------------------------------------------------
def run_shards(ctx, n, full, G, mis, what, estim=2, rt=D.JI, k=31):
    total = n * (n - 1) // 2
    off = ctx.shard_plan(G, estim)
    assert off[0] == 0 and off[-1] == total and all(off[r] <= off[r + 1] for r in range(G))
    spans = []
    for r in range(G):  # every shard on its own (empty spans included)
        g = fbuf(off[r + 1] - off[r], n, (mis + r) % 4 if mis else 0)
        ctx.dist_shard_device(g.ptr, r, G, estim, rt, k)
        ctx.synchronize()
        g.check(str(("shard", what, n, G, r)))
        assert g.unwritten() == 0, ("shard", what, n, G, r)
        spans.append(g.host().copy())
    sorted_want = np.concatenate(spans) if spans else np.zeros(0, F32)
    # back to back in ONE buffer: any alignment per shard, the neighbours as guards
    btb = fbuf(total, n, mis)
    for r in range(G):
        ctx.dist_shard_device(btb.ptr + 4 * off[r], r, G, estim, rt, k)
        ctx.synchronize()
    verify(btb, sorted_want, ("shards back to back", what, n, G, mis))
    out = fbuf(total, n, mis)
    ctx.unpermute_device(btb.ptr, out.ptr)
    ctx.synchronize()
    verify(out, full, ("unpermute", what, n, G, mis))
    untouched(btb, sorted_want, ("unpermute input", what, n, G))
    # padded blocks of a gather: shard r at r * stride
    stride = max(max(off[r + 1] - off[r] for r in range(G)), 1) + 5
    blocks = np.full(G * stride, -4.0, F32)
    for r in range(G):
        blocks[r * stride : r * stride + spans[r].size] = spans[r]
    stage = fbuf(G * stride, n, (mis + 1) % 4 if mis else 0)
    stage.fill(blocks)
    out = fbuf(total, n, mis)
    ctx.unpermute_staged_device(stage.ptr, stride, G, out.ptr)
    ctx.synchronize()
    verify(out, full, ("unpermute_staged", what, n, G, mis))
    untouched(stage, blocks, ("unpermute_staged input", what, n, G))
    # any arrangement of the blocks: the shards in reverse order, 3 floats between them
    boff, pos = [0] * G, 0
    for r in reversed(range(G)):
        boff[r] = pos
        pos += spans[r].size + 3
    blocks = np.full(pos, -5.0, F32)
    for r in range(G):
        blocks[boff[r] : boff[r] + spans[r].size] = spans[r]
    stage = fbuf(pos, n, (mis + 2) % 4 if mis else 0)
    stage.fill(blocks)
    out = fbuf(total, n, mis)
    ctx.unpermute_blocks_device(stage.ptr, boff, out.ptr)
    ctx.synchronize()
    verify(out, full, ("unpermute_blocks", what, n, G, mis))
    untouched(stage, blocks, ("unpermute_blocks input", what, n, G))


@pytest.mark.parametrize("n,p", [(n, p) for n, p in SHAPES if p == 10 or n in (129, 300)])
def test_shards_and_unpermutes(ctx, n, p):
    ctx.set_sketches(collection(n, p))
    full = ctx.dist_rows()
    for G in (1, 2, 3, 5):
        for mis in (0, 1 + (G + n) % 3):
            run_shards(ctx, n, full, G, mis, "p=%d" % p)


# ---- the exchange pair on virtual ranks -----------------------------------------------------------------------------------
def attach_guarded(ctx, regs):
    """the register matrix in a Guarded under dsh_attach_device_sketches: an input of every call on it.  Its start is not
    moved: the library takes an attached matrix at a 16-byte boundary only (anything else is DSH_EINVAL), so the guards
    begin directly in front of the first and behind the last register"""
    n, m = regs.shape
    g = Guarded(regs.size, U8, 2 * m + 128, 2 * m + 128, 0, DEV)
    g.fill(regs)
    ctx.attach_device(g.ptr, n, int(m).bit_length() - 1)
    return g


def run_exchange(ctx, regs, full, rows, world, dst, nparts, mis, what):
    """virtual ranks on one context as tests/test_gpu_multirank.py sets them up: `rows` contiguous bounds (row-sorted parts
    for short ranges) or a RowSets table (ranges + top-up tile rows)"""
    n = regs.shape[0]
    total = n * (n - 1) // 2
    final = fbuf(total, n, mis)
    dregs = attach_guarded(ctx, regs)
    order = [dst] + [r for r in range(world) if r != dst]  # (the destination's per-sketch pass comes first, as in a real run)
    for r in order:
        rs, k, floats = D.exchange_mode(n, rows, r, nparts, dst, want_floats=True)
        if isinstance(rows, D.RowSets):
            segs = rows.rows(r)
            if not segs:
                continue
            first, size = segs[0][0], (floats if r != dst else 0)
            if r != dst:
                assert floats == rows.pairs(r)
        else:
            first, size = rows[r], D.tri_span(n, rows[r], rows[r + 1])
        local = None if r == dst else fbuf(size, n, (mis + r) % 4 if mis else 0)
        ptr = final.ptr + 4 * D.tri_span(n, 0, first) if r == dst else local.ptr  # the destination computes in place
        ctx.attach_device(dregs.ptr, n, ctx.p)  # a rank starts from the registers alone
        ctx.exchange_rows_device_async(ptr, rows, r, nparts, dst)
        ctx.synchronize()
        if r != dst:
            local.check(str(("exchange local", what, world, dst, nparts, r)))
            assert local.unwritten() == 0, ("exchange local", what, world, dst, nparts, r, local.unwritten())
            mine = local.host().copy()
            ctx.exchange_place_device(rows, r, nparts, local.ptr, final.ptr, dst)
            ctx.synchronize()
            untouched(local, mine, ("exchange_place input", what, world, dst, nparts, r))
        final.check(str(("exchange final", what, world, dst, nparts, r)))
    verify(final, full, ("exchange", what, world, dst, nparts, mis))
    untouched(dregs, regs, ("exchange registers", what))


@pytest.mark.parametrize("table", ["bounds", "rowsets"])
@pytest.mark.parametrize("n,p", [(700, 10), (301, 12)])
def test_exchange_virtual_ranks(ctx, n, p, table):
    regs = synth.survey_sketches(n, p, seed=13 + (table == "rowsets"))[0]
    ctx.set_sketches(regs)
    full = ctx.dist_rows()
    case = 0
    try:
        for signal in (1, 0):
            ctx.set_option("finalize_signal", signal)
            for world in (3, 4):
                for dst in (0, world - 2):
                    for nparts in (1, 3):
                        rows = D.balance_rows(n, world) if table == "bounds" else D.balance_rowsets(n, world)
                        for mis in (0, 1 + case % 3):
                            run_exchange(ctx, regs, full, rows, world, dst, nparts, mis, "signal=%d" % signal)
                        case += 1
    finally:
        ctx.set_option("finalize_signal", -1)
        ctx.alloc(2, 10)  # the shared context must not keep a pointer into a tensor that is about to go


# ---- dist_pairs_device ----------------------------------------------------------------------------------------------------
def run_pairs(ctx, n, lhs, rhs, types, mis, what, **kw):
    npairs = lhs.size
    want = ctx.dist_pairs(lhs, rhs, types, **kw)
    gl = Guarded(npairs, U32, 512, 512, mis, DEV)
    gr = Guarded(npairs, U32, 512, 512, (mis + 1) % 4, DEV)
    gl.fill(lhs)
    gr.fill(rhs)
    side = guard_items(n) + 9 * npairs  # (a row stored at another row's position stays inside)
    out = Guarded(len(types) * npairs, F32, side, side, mis, DEV)
    ctx.dist_pairs_device(gl.ptr, gr.ptr, npairs, out.ptr, types, **kw)
    verify(out, want, ("pairs", what, n, npairs, len(types), mis))
    untouched(gl, lhs, ("pairs lhs", what))
    untouched(gr, rhs, ("pairs rhs", what))


@pytest.mark.parametrize("n,p", [(129, 10), (40, 16)])
def test_pairs_device(ctx, n, p):
    ctx.set_sketches(collection(n, p))
    rng = np.random.default_rng(n + p)
    case = 0
    try:
        for chunk in (1, 64, 1 << 18):
            ctx.set_option("pairs_chunk", chunk)
            for npairs in (0, 1, 63, 64, 65, 257):
                lhs, rhs = rng.integers(0, n, npairs).astype(U32), rng.integers(0, n, npairs).astype(U32)
                for types in ((D.JI,), (8, 1, 1, 0), ALL_TYPES):  # an odd count: every row after the first is misaligned
                    for mis in (0, 1 + case % 3):
                        run_pairs(ctx, n, lhs, rhs, types, mis, "chunk=%d" % chunk, estim=case % 3, k=21)
                    case += 1
    finally:
        ctx.set_option("pairs_chunk", 1 << 18)


# ---- copy_sketches_device ---------------------------------------------------------------------------------------------
def run_copy(ctx, regs, first, cnt, mis, what):
    n, m = regs.shape
    g = Guarded(cnt * m, U8, regs.size + 128, regs.size + 128, mis, DEV)  # (the whole matrix fits on either side)
    ctx.copy_sketches_device(g.ptr, first, cnt)
    verify(g, regs[first : first + cnt], ("copy_sketches", what, n, m, first, cnt, mis))


@pytest.mark.parametrize("p", [4, 14])
def test_copy_sketches_device(ctx, p):
    n = 129
    regs = collection(n, p)
    ctx.set_sketches(regs)
    for i, (first, cnt) in enumerate(((0, n), (1, 1), (n - 1, 1), (3, n - 5))):
        for mis in (0, 1 + i % 3):
            run_copy(ctx, regs, first, cnt, mis, "uploaded")


# ---- dist_threshold_device (its capacity edge is guarded in tests/test_gpu_threshold.py) ----------------------------------
def run_threshold(ctx, n, rb, re, t, mis, what, **kw):
    want = ctx.dist_threshold(t, rb, re, **kw)
    hits = want[1].size
    rows = max(min(re, n) - rb, 0)
    rp = Guarded(rows + 1, np.uint64, n + 64, n + 64, mis % 2, DEV)
    col = fbuf(hits, n, mis, U32)
    val = fbuf(hits, n, (mis + 1) % 4 if mis else 0)
    got = ctx.dist_threshold_device(rp.ptr, col.ptr, val.ptr, hits, t, rb, re, **kw)
    assert got == hits
    verify(rp, want[0], ("threshold row_ptr", what, n, rb, re, t, mis))
    verify(col, want[1], ("threshold col", what, n, rb, re, t, mis))
    verify(val, want[2], ("threshold val", what, n, rb, re, t, mis))
    return hits


# ---- host-pointer forms ---------------------------------------------------------------------------------------------------
def hbuf(items, dtype, mis, side=4096, device=None):
    return Guarded(items, dtype, side, side, mis, device)


def test_host_pointer_forms(ctx):
    n, p = 129, 10
    regs = collection(n, p)
    ctx.set_sketches(regs)
    m = 1 << p
    lib, h = ctx._lib, ctx._h
    full = ctx.dist_rows()
    side = guard_items(n)
    for mis in (0, 1, 2, 3):
        for rb, re in ((0, n), (5, n - 3), (n - 1, n)):
            lo, span = D.tri_span(n, 0, rb), D.tri_span(n, rb, re)
            g = hbuf(span, F32, mis, side)
            if span:
                ret = ctx.dist_rows(rb, re, out=g.span())
                assert ret.size == span
            else:  # (a numpy view of no element has no address of its own)
                ctx._ck(lib.dsh_dist_rows(h, 2, D.JI, 31, rb, re, C.c_void_p(g.ptr)))
            verify(g, full[lo : lo + span], ("dist_rows(out=)", rb, re, mis))
            for kind in ("pinned", None):
                g = hbuf(span, F32, mis, side, kind)
                ctx._ck(lib.dsh_dist_rows_async(h, 2, D.JI, 31, rb, re, C.c_void_p(g.ptr)))
                ctx.wait()
                verify(g, full[lo : lo + span], ("dist_rows_async", kind, rb, re, mis))
        # download
        for first, cnt in ((0, n), (1, 1), (n - 1, 1), (3, n - 5)):
            g = hbuf(cnt * m, U8, mis, regs.size + 64)
            ctx._ck(lib.dsh_download_sketches(h, first, cnt, C.c_void_p(g.ptr)))
            verify(g, regs[first : first + cnt], ("download", first, cnt, mis))
        # cardinalities
        for estim in (0, 1, 2):
            g = hbuf(n, np.float64, mis, 2 * n)
            ctx._ck(lib.dsh_cardinalities(h, estim, C.c_void_p(g.ptr)))
            verify(g, ctx.cardinalities(estim), ("cardinalities", estim, mis))
        # dist_pairs' out
        rng = np.random.default_rng(mis)
        for npairs in (0, 1, 65, 257):
            lhs, rhs = rng.integers(0, n, npairs).astype(U32), rng.integers(0, n, npairs).astype(U32)
            for types in ((D.JI,), (8, 1, 0), ALL_TYPES):
                ty = np.asarray(types, np.int32)
                gl, gr = hbuf(npairs, U32, mis), hbuf(npairs, U32, (mis + 1) % 4)
                gl.fill(lhs)
                gr.fill(rhs)
                g = hbuf(len(types) * npairs, F32, mis, side)
                ctx._ck(lib.dsh_dist_pairs(h, 2, ty.ctypes.data, ty.size, 31, C.c_void_p(gl.ptr), C.c_void_p(gr.ptr), npairs, C.c_void_p(g.ptr)))
                verify(g, ctx.dist_pairs(lhs, rhs, types), ("dist_pairs out", npairs, len(types), mis))
                untouched(gl, lhs, "dist_pairs lhs")
                untouched(gr, rhs, "dist_pairs rhs")
        # knn: nn around the 64 lanes; a rectangle with fewer references than nn writes its filler entries too
        for nn in (1, 64, 65):
            for q0, q1, r0, r1 in ((0, n, 0, n), (3, 20, 10, 40), (100, n, 0, 7)):
                nq = q1 - q0
                gi, gv = hbuf(nq * nn, U32, mis, n * nn + 64), hbuf(nq * nn, F32, (mis + 2) % 4, n * nn + 64)
                ctx._ck(lib.dsh_knn(h, 2, D.JI, 31, q0, q1, r0, r1, nn, C.c_void_p(gi.ptr), C.c_void_p(gv.ptr)))
                want = ctx.knn(nn, q0, q1, r0, r1)
                verify(gi, want[0], ("knn idx", nn, q0, q1, r0, r1, mis))
                verify(gv, want[1], ("knn val", nn, q0, q1, r0, r1, mis))
                model = knn_ref.select(ctx.dist_rect(q0, q1, r0, r1), nn, q0, r0, True, D.JI)
                assert knn_ref.same((gi.host().reshape(nq, nn), gv.host().reshape(nq, nn)), model), (nn, q0, q1, r0, r1)
                if r1 - r0 < nn:
                    assert (gi.host().reshape(nq, nn)[:, -1] == knn_ref.FILL).all()


def test_host_regs_out_of_the_sketch_calls(ctx, oracle):
    p, k = 10, 21
    m = 1 << p
    gs = synth.synthetic_genomes(5, 3000, seed=3)
    seq, off = synth.concat_for_device(gs)
    seq = np.ascontiguousarray(seq, U8)
    off = np.ascontiguousarray(off, np.uint64)
    ng = off.size - 1
    lib, h = ctx._lib, ctx._h
    for mis in (0, 1, 2, 3):
        for first in (0, 2):
            ctx.alloc(ng + 3, p)
            want = ctx.sketch_batch(seq, off, first, k, True)
            assert (want == oracle.sketch_batch(seq, off, k, p, True)).all()
            ctx.alloc(ng + 3, p)
            g = hbuf(ng * m, U8, mis, (ng + 3) * m)
            ctx._ck(lib.dsh_sketch_batch(h, seq.ctypes.data, off.ctypes.data, ng, first, k, 1, C.c_void_p(g.ptr)))
            verify(g, want, ("sketch_batch regs_out", first, mis))
            assert (ctx.download(first, ng) == want).all()
            # records: the same bytes cut at other places, rows overwritten
            rec = np.array([0, 40, 40, 1500, 1519, int(off[-1])], np.uint64)
            nr = rec.size - 1
            wantr = ctx.sketch_records(seq, rec, first, k, True)
            ctx.clear()
            g = hbuf(nr * m, U8, mis, (ng + 3) * m)
            ctx._ck(lib.dsh_sketch_records(h, seq.ctypes.data, rec.ctypes.data, nr, first, k, 1, C.c_void_p(g.ptr)))
            verify(g, wantr, ("sketch_records regs_out", first, mis))
            assert wantr.any() and not wantr[1].any()  # (an empty record has an all-zero row, which IS written)


# ---- inputs stay inputs -------------------------------------------------------------------------------------------------
def test_attached_matrix_is_never_written(ctx):
    import hashlib

    try:
        for i, (n, p) in enumerate(((129, 10), (300, 8), (130, 14), (40, 16))):
            regs = collection(n, p)
            mis = (0, 1, 2, 3)[i]
            dregs = attach_guarded(ctx, regs)
            before = hashlib.sha256(dregs.host().tobytes()).hexdigest()
            assert before == hashlib.sha256(regs.tobytes()).hexdigest()
            if mis:  # a matrix off the 16-byte boundary is refused, not read from a rounded address
                with pytest.raises(D.DshError):
                    ctx.attach_device(dregs.ptr + mis, n - 1, p)
                ctx.attach_device(dregs.ptr, n, p)

            def same(what):
                dregs.check(str(("attached registers", what, n, p)))
                assert hashlib.sha256(dregs.host().tobytes()).hexdigest() == before, (what, n, p)

            ctx.cardinalities()
            same("cardinalities")
            full = ctx.dist_rows()
            same("dist_rows")
            run_rows(ctx, n, full, 0, n, mis, False, "attached")
            run_rows(ctx, n, full, 5, n - 3, (mis + 1) % 4, True, "attached")
            same("dist_rows_device")
            ctx.dist_rect(3, n - 2, 1, n)
            same("dist_rect")
            ctx.knn(5)
            ctx.knn(3, 2, 30, 1, n - 1)
            same("knn")
            hits = run_threshold(ctx, n, 0, n, 0.02, mis, "attached")
            run_threshold(ctx, n, 5, n - 3, 1.0, (mis + 1) % 4, "attached")  # (t = 1.0: the duplicated pair alone)
            assert 0 < hits < full.size
            same("dist_threshold_device")
            rng = np.random.default_rng(n)
            lhs, rhs = rng.integers(0, n, 257).astype(U32), rng.integers(0, n, 257).astype(U32)
            run_pairs(ctx, n, lhs, rhs, ALL_TYPES, mis, "attached")
            same("dist_pairs_device")
            run_copy(ctx, regs, 3, n - 5, (mis + 2) % 4, "attached")
            same("copy_sketches_device")
    finally:
        ctx.alloc(2, 10)  # the shared context must not keep a pointer into a tensor that is about to go


# ---- a short seeded fuzz ------------------------------------------------------------------------------------------------
_FIRST = int(os.environ.get("DSH_GUARD_FIRST", "0"))
ENTRY_POINTS = ["rows", "rows_async", "parts", "shards", "exchange", "pairs", "threshold", "copy"]


@pytest.mark.parametrize("case", range(_FIRST, _FIRST + int(os.environ.get("DSH_GUARD_CASES", "40"))))
def test_random_case(ctx, case):
    rng = np.random.default_rng(0x6A2D0000 + case)
    p = int(rng.choice([6, 8, 9, 10, 12, 14, 16]))
    n = int(rng.integers(1, 141 if p >= 14 else 421))
    what = ENTRY_POINTS[(case + int(rng.integers(0, 2)) * 3) % len(ENTRY_POINTS)]
    mis = int(rng.integers(0, 4))
    estim = int(rng.integers(0, 3))
    rt = int(rng.choice(ALL_TYPES))
    k = int(rng.choice([15, 21, 31, 32]))
    emax = int(rng.choice(ctx_model.OPTION_VALUES["emax"]))
    elow = int(rng.choice(ctx_model.OPTION_VALUES["elow"]))
    regs = synth.synthetic_sketches(n, p, seed=int(rng.integers(1 << 30)))
    if n > 4:
        regs[int(rng.integers(n))] = 0
        a, b = rng.choice(n, 2, replace=False)
        regs[a] = regs[b]
    rb = int(rng.integers(0, n))
    re = int(rng.integers(rb, n + 1))
    kw = dict(estim=estim, result_type=rt, k=k)
    note = "case %d: %s n=%d p=%d mis=%d estim=%d rt=%d k=%d emax=%d elow=%d rows [%d, %d)" % (case, what, n, p, mis, estim, rt, k, emax, elow, rb, re)
    print(note)
    try:
        ctx.set_option("emax", emax)
        ctx.set_option("elow", elow)
        ctx.set_sketches(regs)
        full = ctx.dist_rows(**kw)
        if what in ("rows", "rows_async"):
            ctx.set_option("range_sort_min_rows", int(rng.choice(ctx_model.OPTION_VALUES["range_sort_min_rows"])))
            run_rows(ctx, n, full, rb, re, mis, what == "rows_async", note, **kw)
            run_rows(ctx, n, full, 0, n, mis, what == "rows_async", note, **kw)
        elif what == "parts":
            ctx.set_option("range_sort_min_rows", 1)
            ctx.set_option("part_band_tiles", int(rng.choice(ctx_model.OPTION_VALUES["part_band_tiles"])))
            run_parts(ctx, n, full, rb, re, int(rng.integers(1, 7)), mis, note, **kw)
        elif what == "shards":
            run_shards(ctx, n, full, int(rng.integers(1, 6)), mis, note, estim, rt, k)
        elif what == "exchange":
            if n >= 2:
                world = int(rng.integers(1, 6))
                ctx.set_option("finalize_signal", int(rng.choice([0, 1])))
                rows = D.balance_rows(n, world) if rng.random() < 0.5 else D.balance_rowsets(n, world)
                full = ctx.dist_rows()  # (the exchange runs under the defaults of the tests it is modelled on)
                run_exchange(ctx, regs, full, rows, world, int(rng.integers(0, world)), int(rng.integers(1, 5)), mis, note)
        elif what == "pairs":
            npairs = int(rng.choice([0, 1, 63, 64, 65, 257, int(rng.integers(1, 600))]))
            ctx.set_option("pairs_chunk", int(rng.choice([1, 64, 100, 1 << 18])))
            types = tuple(int(x) for x in rng.choice(ALL_TYPES, int(rng.integers(1, 10))))
            lhs, rhs = rng.integers(0, n, npairs).astype(U32), rng.integers(0, n, npairs).astype(U32)
            run_pairs(ctx, n, lhs, rhs, types, mis, note, estim=estim, k=k)
        elif what == "threshold":
            fin = full[np.isfinite(full)]
            t = float(np.median(fin)) if fin.size else 0.5
            run_threshold(ctx, n, rb, re, t, mis, note, **kw)
        elif what == "copy":
            run_copy(ctx, regs, rb, re - rb, mis, note)
    finally:
        for name in ("emax", "elow", "range_sort_min_rows", "part_band_tiles", "finalize_signal"):
            ctx.set_option(name, ctx_model.OPTION_DEFAULTS[name])
        ctx.set_option("pairs_chunk", 1 << 18)
        ctx.alloc(2, 10)
