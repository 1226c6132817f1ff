"""dsh_dist_pairs / dsh_dist_pairs_device / dsh_dist_pairs_csr on the device: equal to the dense path bit for bit (no
tolerance, no pair left out), within 1e-6 of the oracle, independent of order, grouping and chunking, and without a trace
in the context's derived state."""
import numpy as np
import pytest

import dashing_amd
import pairs_ref
import thr_ref
from dashing_amd import synth

pytestmark = pytest.mark.gpu

D = dashing_amd
ALL = pairs_ref.ALL_TYPES
RTOL = 1e-6  # the rule of tests/test_gpu_compare.py::close, restated: |d| <= 1e-6 * max(|ref|, 1e-9)


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    ne = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert ne.size == 0, (what, "first mismatch at %d of %d (%d differ): %r != %r" % (
        ne[0], g.size, ne.size, np.asarray(got).reshape(-1)[ne[0]], np.asarray(want).reshape(-1)[ne[0]]))


@pytest.fixture(autouse=True)
def default_chunk(ctx):
    yield
    ctx.set_option("pairs_chunk", 1 << 18)
    ctx.set_option("sort", -1)


def check_against_dense(ctx, n, lhs, rhs, estims=(0, 1, 2), k=31, oracle=None, regs=None):
    """lhs > rhs everywhere: the pairs as given against dist_rows, reversed and with themselves against dist_rect"""
    slots = np.unique(np.concatenate([lhs, rhs]))[:64]
    for estim in estims:
        got = ctx.dist_pairs(lhs, rhs, ALL, estim=estim, k=k)
        rev = ctx.dist_pairs(rhs, lhs, ALL, estim=estim, k=k)
        selfp = ctx.dist_pairs(slots, slots, ALL, estim=estim, k=k)
        assert got.dtype == np.float32 and got.shape == (9, lhs.size)
        for t, rt in enumerate(ALL):
            tri = ctx.dist_rows(estim=estim, result_type=rt, k=k)
            assert_bits(got[t], pairs_ref.pick_tri(tri, n, lhs, rhs), ("tri", n, estim, rt))
            rect = ctx.dist_rect(0, n, 0, n, estim=estim, result_type=rt, k=k)
            assert_bits(got[t], pairs_ref.pick_rect(rect, lhs, rhs), ("rect", n, estim, rt))
            assert_bits(rev[t], pairs_ref.pick_rect(rect, rhs, lhs), ("rect reversed", n, estim, rt))
            assert_bits(selfp[t], pairs_ref.pick_rect(rect, slots, slots), ("self", n, estim, rt))
            if oracle is not None:
                otri = oracle.dist_tri(regs, estim, rt, k)
                want = pairs_ref.pick_tri(otri, n, lhs, rhs)
                close(got[t], want)
                if rt == D.MASH_DIST:
                    oj = pairs_ref.pick_tri(oracle.dist_tri(regs, estim, D.JI, k), n, lhs, rhs)
                    assert (got[t][oj == 0] == 1).all()


# ---- 1, 2: equal to the dense path bit for bit, within 1e-6 of the oracle ---------------------------------------------
@pytest.mark.parametrize("n,p,seed", [(300, 10, 91), (700, 12, 91)])
def test_all_pairs_equal_dense_and_oracle(ctx, oracle, n, p, seed):
    regs = synth.related_sketches(n, p, seed=seed)[0]
    ctx.set_sketches(regs)
    lhs, rhs = pairs_ref.all_tri_pairs(n)
    check_against_dense(ctx, n, lhs, rhs, oracle=oracle, regs=regs)


def test_random_pairs_of_survey_equal_dense_and_oracle(ctx, oracle):
    n = 3000
    regs = synth.survey_sketches(n, 12)[0]
    ctx.set_sketches(regs)
    rng = np.random.default_rng(12)
    a = rng.integers(0, n, 3000)
    b = (a + rng.integers(1, n, 3000)) % n
    lhs, rhs = np.maximum(a, b).astype(np.uint32), np.minimum(a, b).astype(np.uint32)
    check_against_dense(ctx, n, lhs, rhs)
    for estim in (0, 1, 2):
        got = ctx.dist_pairs(lhs, rhs, ALL, estim=estim)
        want = pairs_ref.pair_values(oracle, regs, lhs, rhs, ALL, estim, 31)
        for t, rt in enumerate(ALL):
            close(got[t], want[t])
        assert (got[0][want[1] == 0] == 1).all()  # oracle J exactly 0: Mash distance exactly 1


@pytest.mark.parametrize("p,n", [(4, 40), (8, 40), (9, 40), (13, 30), (14, 24), (15, 12), (16, 10), (18, 6)])
def test_other_precisions(ctx, oracle, p, n):
    regs = synth.synthetic_sketches(n, p, seed=p)
    ctx.set_sketches(regs)
    lhs, rhs = pairs_ref.all_tri_pairs(n)
    check_against_dense(ctx, n, lhs, rhs, oracle=oracle, regs=regs)


# ---- 3: CSR round trip ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(thr_ref.oracle_cases())))
def test_csr_round_trip(ctx, case):
    name, make, rt, k, ts = thr_ref.oracle_cases()[case]
    regs = make()
    n = regs.shape[0]
    ctx.set_sketches(regs)
    other = D.JI if rt != D.JI else D.MASH_DIST
    dense_other = ctx.dist_rows(result_type=other, k=k)
    for t in ts:
        for rb, re in ((0, n), (n // 3, n // 2)):
            row_ptr, col, val = ctx.dist_threshold(t, rb, re, result_type=rt, k=k)
            got = ctx.dist_pairs_csr(row_ptr, col, rb, (rt, other), k=k)
            assert got.shape == (2, col.size)
            assert_bits(got[0], val, (name, rt, t, rb, re))
            rows = np.repeat(np.arange(rb, re), np.diff(row_ptr.astype(np.int64)))
            assert_bits(got[1], pairs_ref.pick_tri(dense_other, n, col, rows), (name, other, t, rb, re))
    # rectangle form, queries and references overlapping
    q0, q1, r0, r1 = n // 4, n // 2, n // 3, n
    rect_other = ctx.dist_rect(q0, q1, r0, r1, result_type=other, k=k)
    for t in ts[:2]:
        row_ptr, col, val = ctx.dist_rect_threshold(t, q0, q1, r0, r1, result_type=rt, k=k)
        got = ctx.dist_pairs_csr(row_ptr, col, q0, (rt, other), k=k)
        assert_bits(got[0], val, (name, "rect", rt, t))
        rows = np.repeat(np.arange(q0, q1), np.diff(row_ptr.astype(np.int64)))
        assert_bits(got[1], pairs_ref.pick_rect(rect_other, col, rows, q0, r0), (name, "rect", other, t))


# ---- 4: multi-measure -------------------------------------------------------------------------------------------------
def test_one_call_with_nine_types_equals_nine_calls(ctx):
    n = 200
    ctx.set_sketches(synth.synthetic_sketches(n, 11, seed=4))
    rng = np.random.default_rng(4)
    lhs, rhs = rng.integers(0, n, 5000), rng.integers(0, n, 5000)
    for estim in (0, 1, 2):
        nine = ctx.dist_pairs(lhs, rhs, ALL, estim=estim)
        for t, rt in enumerate(ALL):
            assert_bits(nine[t], ctx.dist_pairs(lhs, rhs, (rt,), estim=estim)[0], (estim, rt))
        perm = (8, 1, 1, 0, 5)
        some = ctx.dist_pairs(lhs, rhs, perm, estim=estim)
        for t, rt in enumerate(perm):
            assert_bits(some[t], nine[rt], (estim, perm, t))


# ---- 5: order, grouping, chunking -------------------------------------------------------------------------------------
def test_order_and_grouping(ctx):
    n = 500
    ctx.set_sketches(synth.related_sketches(n, 10, seed=8)[0])
    rng = np.random.default_rng(8)
    lhs, rhs = rng.integers(0, n, 20000).astype(np.uint32), rng.integers(0, n, 20000).astype(np.uint32)
    types = (D.JI, D.MASH_DIST, 5)
    base = ctx.dist_pairs(lhs, rhs, types)
    sh = rng.permutation(lhs.size)
    assert_bits(ctx.dist_pairs(lhs[sh], rhs[sh], types), base[:, sh], "shuffled")
    so = np.argsort(rhs, kind="stable")
    assert_bits(ctx.dist_pairs(lhs[so], rhs[so], types), base[:, so], "sorted by rhs")
    assert_bits(ctx.dist_pairs(np.repeat(lhs, 3), np.repeat(rhs, 3), types), np.repeat(base, 3, axis=1), "repeated")
    # 1 000 000 pairs over the 500 sketches: every pair equals the value of its (lhs, rhs) in the n x n table
    table = ctx.dist_pairs(np.tile(np.arange(n), n), np.repeat(np.arange(n), n), types).reshape(len(types), n, n)
    big_l, big_r = rng.integers(0, n, 1_000_000), rng.integers(0, n, 1_000_000)
    assert_bits(ctx.dist_pairs(big_l, big_r, types), table[:, big_r, big_l], "one million pairs")


def test_every_chunk_size_gives_the_same_bytes(ctx):
    n = 60
    ctx.set_sketches(synth.synthetic_sketches(n, 10, seed=2))
    rng = np.random.default_rng(2)
    lhs, rhs = rng.integers(0, n, 37), rng.integers(0, n, 37)
    base = ctx.dist_pairs(lhs, rhs, ALL)
    import torch

    dl = torch.tensor(lhs.astype(np.int64), device="cuda").to(torch.int32)
    dr = torch.tensor(rhs.astype(np.int64), device="cuda").to(torch.int32)
    for chunk in list(range(1, 40)) + [64, 1000, 1 << 24]:
        ctx.set_option("pairs_chunk", chunk)
        assert_bits(ctx.dist_pairs(lhs, rhs, ALL), base, chunk)
        out = torch.full((9, 37), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
        ctx.dist_pairs_device(dl.data_ptr(), dr.data_ptr(), 37, out.data_ptr(), ALL)
        assert_bits(out.cpu().numpy(), base, ("device", chunk))
    ctx.set_option("pairs_chunk", 1 << 18)
    # a list longer than the default chunk, with a ragged tail
    big_l, big_r = rng.integers(0, n, (1 << 18) + 77), rng.integers(0, n, (1 << 18) + 77)
    want = ctx.dist_pairs(big_l, big_r, (1, 0))
    ctx.set_option("pairs_chunk", 50000)
    assert_bits(ctx.dist_pairs(big_l, big_r, (1, 0)), want, "ragged")
    for bad in (0, -1, (1 << 24) + 1):
        with pytest.raises(D.DshError):
            ctx.set_option("pairs_chunk", bad)


# ---- 6: edges ---------------------------------------------------------------------------------------------------------
def test_edges(ctx, oracle):
    n, p = 50, 10
    regs = synth.synthetic_sketches(n, p, seed=6)
    ctx.set_sketches(regs)
    assert ctx.dist_pairs([], [], ALL).shape == (9, 0)
    assert ctx.dist_pairs([1, 2], [0, 0], ()).shape == (0, 2)
    one = ctx.dist_pairs([n - 1], [0], ALL)
    tri_last = [ctx.dist_rows(result_type=rt)[n - 2] for rt in ALL]  # pair (0, n - 1) closes row 0
    assert_bits(one[:, 0], np.array(tri_last, np.float32), "slots 0 and n - 1")
    # all-zero sketches, constant sketches at the largest legal register, the sketch with itself
    q = 64 - p
    regs[3] = 0
    regs[4] = 0
    regs[5] = q + 1
    regs[6] = q + 1
    regs[7] = 7
    ctx.set_sketches(regs)
    lhs, rhs = pairs_ref.all_tri_pairs(n)
    check_against_dense(ctx, n, lhs, rhs, oracle=oracle, regs=regs)
    s = np.array([0, 1, 7, n - 1])
    selfv = ctx.dist_pairs(s, s, (D.JI, D.MASH_DIST))
    assert (selfv[0] == 1).all() and (selfv[1] == 0).all()


@pytest.mark.parametrize("p", (8, 12))
def test_adversarial_uniform_registers(ctx, oracle, p):
    """the generator of tests/test_gpu_compare.py::test_adversarial_registers, restated: registers that do not follow the
    HLL law"""
    q = 64 - p
    rng = np.random.default_rng(p)
    n, m = 140, 1 << p
    regs = rng.integers(0, q + 2, size=(n, m)).astype(np.uint8)
    regs[0] = q + 1
    regs[1] = 7
    regs[2] = 0
    regs[2, 5] = 9
    regs[3] = rng.integers(0, 3, size=m)
    regs[4] = rng.integers(q - 2, q + 2, size=m)
    ctx.set_sketches(regs)
    lhs, rhs = pairs_ref.all_tri_pairs(n)
    for sm in (1, 0):
        ctx.set_option("sort", sm)
        check_against_dense(ctx, n, lhs, rhs)
    for estim in (0, 1, 2):
        want = oracle.dist_tri(regs, estim, D.JI, 31)
        got = ctx.dist_pairs(lhs, rhs, (D.JI,), estim=estim)[0]
        fin = np.isfinite(want)
        assert (np.isfinite(got) == fin).all()
        assert np.allclose(got[fin], want[fin], rtol=1e-6, atol=1e-12)


# ---- 7: errors --------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    with D.Context(0) as fresh:
        with pytest.raises(D.DshError) as e:
            fresh.dist_pairs([0], [0])
        assert e.value.code == -11  # DSH_ESTATE
        with pytest.raises(D.DshError) as e:
            fresh.dist_pairs_csr([0, 0], [], 0)
        assert e.value.code == -11
    n = 20
    ctx.set_sketches(synth.synthetic_sketches(n, 10, seed=1))
    for lhs, rhs in (([n], [0]), ([0], [n]), ([1, 2, 0xFFFFFFFF], [0, 0, 0])):
        with pytest.raises(D.DshError) as e:
            ctx.dist_pairs(lhs, rhs)
        assert e.value.code == -22
    for types in ((9,), (-1,), (1, 2, 77), (1,) * 10):
        with pytest.raises(D.DshError) as e:
            ctx.dist_pairs([1], [0], types)
        assert e.value.code == -22
    with pytest.raises(D.DshError) as e:
        ctx.dist_pairs([1], [0], estim=3)
    assert e.value.code == -22
    for row_ptr, col, rb in (([0, 2, 1], [1, 2], 0), ([0, 1], [n], 0), ([0, 1, 1], [3], n - 1), ([0, 0], [], n)):
        with pytest.raises(D.DshError) as e:
            ctx.dist_pairs_csr(row_ptr, col, rb)
        assert e.value.code == -22, (row_ptr, col, rb)
    assert ctx.dist_pairs_csr([0], [], 0).shape == (1, 0)
    assert ctx.dist_pairs_csr([0, 0, 0], [], 3).shape == (1, 0)
    assert ctx.dist_pairs([1], [0]).shape == (1, 1)  # the context is still good


def test_out_of_range_registers_in_a_named_sketch_are_refused(ctx):
    p = 12
    regs = synth.synthetic_sketches(40, p, seed=3)
    good = None
    for badval in (64 - p + 2, 100, 200, 255):
        r = regs.copy()
        r[17, 1234] = badval
        ctx.set_sketches(r)
        for lhs, rhs in (([3, 17, 5], [1, 2, 4]), ([3, 20], [1, 17]), ([17], [17])):
            with pytest.raises(D.DshError) as e:
                ctx.dist_pairs(lhs, rhs)
            assert e.value.code == -22 and "sketch 17" in str(e.value)
        # the same matrix with that sketch not named
        lhs, rhs = pairs_ref.all_tri_pairs(40)
        keep = (lhs != 17) & (rhs != 17)
        got = ctx.dist_pairs(lhs[keep], rhs[keep], ALL)
        if good is None:
            ctx.set_sketches(regs)
            good = ctx.dist_pairs(lhs[keep], rhs[keep], ALL)
        assert_bits(got, good, badval)
    # the device form: the same refusal, found on the device
    import torch

    r = regs.copy()
    r[17, 1234] = 200
    r[30, 7] = 99
    ctx.set_sketches(r)
    out = torch.zeros((9, 3), dtype=torch.float32, device="cuda")
    for lhs, rhs, who in (([3, 30, 17], [1, 2, 4], "sketch 17"), ([3, 5, 6], [1, 30, 4], "sketch 30")):
        dl = torch.tensor(lhs, dtype=torch.int32, device="cuda")
        dr = torch.tensor(rhs, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
        with pytest.raises(D.DshError) as e:
            ctx.dist_pairs_device(dl.data_ptr(), dr.data_ptr(), 3, out.data_ptr(), ALL)
        assert e.value.code == -22 and who in str(e.value)
    dl = torch.tensor([3, 5, 6], dtype=torch.int32, device="cuda")
    dr = torch.tensor([1, 2, 4], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
    ctx.dist_pairs_device(dl.data_ptr(), dr.data_ptr(), 3, out.data_ptr(), ALL)  # neither is named: fine
    assert_bits(out.cpu().numpy(), ctx.dist_pairs([3, 5, 6], [1, 2, 4], ALL), "device form beside unnamed bad sketches")
    regs[17, 1234] = 64 - p + 1  # the largest legal value is fine
    ctx.set_sketches(regs)
    assert np.isfinite(ctx.dist_pairs([17], [3])).all()


# ---- 8: device form ---------------------------------------------------------------------------------------------------
def test_device_form(ctx):
    import torch

    n = 300
    ctx.set_sketches(synth.related_sketches(n, 12, seed=21)[0])
    rng = np.random.default_rng(21)
    lhs, rhs = rng.integers(0, n, 10000), rng.integers(0, n, 10000)
    want = ctx.dist_pairs(lhs, rhs, ALL, estim=1, k=21)
    dl = torch.tensor(lhs, device="cuda").to(torch.int32)
    dr = torch.tensor(rhs, device="cuda").to(torch.int32)
    out = torch.zeros((9, lhs.size), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
    ctx.dist_pairs_device(dl.data_ptr(), dr.data_ptr(), lhs.size, out.data_ptr(), ALL, estim=1, k=21)
    assert_bits(out.cpu().numpy(), want, "device form")
    torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
    ctx.dist_pairs_device(0, 0, 0, 0, ALL)  # an empty list needs no buffers
    dl[777] = n  # a slot out of range fails the call (checked on the device)
    torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
    with pytest.raises(D.DshError) as e:
        ctx.dist_pairs_device(dl.data_ptr(), dr.data_ptr(), lhs.size, out.data_ptr(), ALL)
    assert e.value.code == -22 and "pair 777" in str(e.value)
    dl[777] = int(lhs[777])
    torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
    ctx.dist_pairs_device(dl.data_ptr(), dr.data_ptr(), lhs.size, out.data_ptr(), ALL, estim=1, k=21)
    assert_bits(out.cpu().numpy(), want, "device form after the failed call")


# ---- 9: the context's derived state -----------------------------------------------------------------------------------
def test_dense_calls_do_not_see_pairs_calls(ctx):
    n = 400
    regs = synth.related_sketches(n, 10, seed=33)[0]
    rng = np.random.default_rng(33)
    lhs, rhs = rng.integers(0, n, 3000), rng.integers(0, n, 3000)

    def dense():
        return (ctx.dist_rows(estim=2, result_type=D.MASH_DIST).tobytes(),
                b"".join(np.asarray(x).tobytes() for x in ctx.dist_threshold(0.1, 20, 300, result_type=D.JI)),
                b"".join(np.asarray(x).tobytes() for x in ctx.knn(5)))

    ctx.set_sketches(regs)
    before = dense()
    ctx.set_sketches(regs)
    first = ctx.dist_pairs(lhs, rhs, ALL, estim=0)  # before any dense call: nothing of the dense path exists yet
    a = ctx.dist_rows(estim=2, result_type=D.MASH_DIST).tobytes()
    ctx.dist_pairs(lhs, rhs, ALL, estim=1)
    b = b"".join(np.asarray(x).tobytes() for x in ctx.dist_threshold(0.1, 20, 300, result_type=D.JI))
    ctx.dist_pairs_csr([0, 2, 3], [5, 6, 7], 1, (0,), estim=2)
    c = b"".join(np.asarray(x).tobytes() for x in ctx.knn(5))
    assert (a, b, c) == before
    assert_bits(ctx.dist_pairs(lhs, rhs, ALL, estim=0), first, "pairs after dense calls")
    assert dense() == before
