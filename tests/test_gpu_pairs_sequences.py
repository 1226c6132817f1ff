"""The explicit pair list as one more call kind of a context that is being mutated (in the manner of
tests/test_gpu_ctx_sequences.py): every pairs call sees the registers as they are at that moment, whatever was called
before -- checked against tests/pairs_ref.py (oracle) and, bit for bit, against the dense path.  And a fuzz of random
collections, measure sets, estimators and list shapes against the dense path."""
import numpy as np
import pytest

import dashing_amd
import pairs_ref
from dashing_amd import synth

pytestmark = pytest.mark.gpu

D = dashing_amd
RTOL = 1e-6


def close(got, ref):  # the rule of tests/test_gpu_compare.py::close, restated
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all()
    err = np.abs(got[fin] - ref[fin])
    assert (err <= RTOL * np.maximum(np.abs(ref[fin]), 1e-9)).all()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("seed", range(4))
def test_pairs_calls_see_every_mutation(ctx, oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    p, k = 10, 21
    gs = synth.synthetic_genomes(12, 20000, seed=seed + 1)
    n = 40
    model = synth.synthetic_sketches(n, p, seed=seed)
    ctx.set_sketches(model)
    trace = []

    def pairs_call():
        m = int(rng.integers(1, 200))
        lhs, rhs = rng.integers(0, n, m), rng.integers(0, n, m)
        estim = int(rng.integers(0, 3))
        types = tuple(int(x) for x in rng.integers(0, 9, int(rng.integers(1, 5))))
        form = int(rng.integers(0, 2))
        if form == 0:
            got = ctx.dist_pairs(lhs, rhs, types, estim=estim, k=k)
        else:  # as CSR: rows = sorted rhs
            order = np.argsort(rhs, kind="stable")
            lhs, rhs = lhs[order], rhs[order]
            row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rhs, minlength=n))]).astype(np.uint64)
            got = ctx.dist_pairs_csr(row_ptr, lhs.astype(np.uint32), 0, types, estim=estim, k=k)
        want = pairs_ref.pair_values(oracle, model, lhs, rhs, types, estim, k)
        for t in range(len(types)):
            try:
                close(got[t], want[t])
            except AssertionError:
                ne = np.flatnonzero(~np.isclose(got[t], want[t], rtol=1e-5, atol=0))
                raise AssertionError("steps %r, form %d, estim %d, types %r, measure %d: pairs %r give %r, the oracle %r" % (
                    trace, form, estim, types, types[t], [(int(lhs[x]), int(rhs[x])) for x in ne[:8]], got[t][ne[:8]], want[t][ne[:8]]))
        rect = {rt: ctx.dist_rect(0, n, 0, n, estim=estim, result_type=rt, k=k) for rt in set(types)} if rng.integers(0, 2) else {}
        for t, rt in enumerate(types):
            if rt in rect:
                assert np.array_equal(bits(got[t]), bits(pairs_ref.pick_rect(rect[rt], lhs, rhs))), (trace, rt)

    for step in range(14):
        kind = int(rng.integers(0, 6))
        trace.append(kind)
        if kind == 0:
            model = synth.synthetic_sketches(n, p, seed=100 * seed + step)
            ctx.set_sketches(model)
        elif kind == 1:
            s = int(rng.integers(0, n))
            row = synth.synthetic_sketches(1, p, seed=7 * step + 3)
            ctx.upload(row, s)
            model = model.copy()
            model[s] = row[0]
        elif kind == 2:
            s, c = int(rng.integers(0, n - 3)), int(rng.integers(1, 4))
            ctx.clear(s, c)
            model = model.copy()
            model[s:s + c] = 0
        elif kind == 3:
            take = [gs[int(x)] for x in rng.integers(0, len(gs), 3)]
            seq, off = synth.concat_for_device(take)
            s = int(rng.integers(0, n - 3))
            if rng.integers(0, 2):  # onto cleared rows: the genomes' own sketches
                ctx.clear(s, 3)
                model = model.copy()
                model[s:s + 3] = 0
            ctx.sketch_batch(seq, off, s, 31, True)
            model = model.copy()
            model[s:s + 3] = np.maximum(model[s:s + 3], oracle.sketch_batch(seq, off, 31, p, True))  # (sketching max-merges)
        elif kind == 4:
            ctx.dist_rows(estim=int(rng.integers(0, 3)))
        pairs_call()
    assert np.array_equal(ctx.download(), model)


FUZZ_CASES = 2000
FUZZ_SEED = 20240607


def test_fuzz_against_the_dense_path(ctx):
    import torch

    rng = np.random.default_rng(FUZZ_SEED)
    for case in range(FUZZ_CASES):
        p = int(rng.integers(4, 17))
        n = int(rng.integers(2, 401))
        n = max(2, min(n, (1 << 22) >> p))  # (registers of a case: at most 4 MiB)
        estim = int(rng.integers(0, 3))
        k = int(rng.integers(1, 33))
        types = tuple(int(x) for x in rng.integers(0, 9, int(rng.integers(1, 10))))
        regs = synth.synthetic_sketches(n, p, seed=int(rng.integers(0, 1 << 30)), cluster=int(rng.integers(1, 12)))
        if rng.integers(0, 4) == 0:
            regs[int(rng.integers(0, n))] = 0
        ctx.set_sketches(regs)
        shape = int(rng.integers(0, 4))
        m = int(rng.integers(1, 600))
        if shape == 0:    # random
            lhs, rhs = rng.integers(0, n, m), rng.integers(0, n, m)
        elif shape == 1:  # runs of equal rhs (a CSR row, a kNN list)
            rhs = np.sort(rng.integers(0, n, m))
            lhs = rng.integers(0, n, m)
        elif shape == 2:  # one pair over and over, the sketch with itself
            lhs = np.full(m, int(rng.integers(0, n)))
            rhs = np.where(rng.integers(0, 2, m) == 1, lhs, int(rng.integers(0, n)))
        else:             # the whole triangle
            lhs, rhs = pairs_ref.all_tri_pairs(n)
        if rng.integers(0, 3) == 0:
            ctx.set_option("pairs_chunk", int(rng.integers(1, 300)))
        lhs, rhs = np.asarray(lhs, np.uint32), np.asarray(rhs, np.uint32)
        form = int(rng.integers(0, 3))
        if form == 0:
            got = ctx.dist_pairs(lhs, rhs, types, estim=estim, k=k)
        elif form == 1:  # the device form
            dl, dr = torch.from_numpy(lhs.astype(np.int32)).cuda(), torch.from_numpy(rhs.astype(np.int32)).cuda()
            dout = torch.full((len(types), lhs.size), -1.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
            ctx.dist_pairs_device(dl.data_ptr(), dr.data_ptr(), lhs.size, dout.data_ptr(), types, estim=estim, k=k)
            got = dout.cpu().numpy()
        else:            # as CSR: rows = the rhs slots from row_begin on
            order = np.argsort(rhs, kind="stable")
            lhs, rhs = lhs[order], rhs[order]
            rb = int(rhs.min())
            row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rhs - rb, minlength=int(rhs.max()) - rb + 1))]).astype(np.uint64)
            got = ctx.dist_pairs_csr(row_ptr, lhs, rb, types, estim=estim, k=k)
        ctx.set_option("pairs_chunk", 1 << 18)
        for t, rt in enumerate(types):
            rect = ctx.dist_rect(0, n, 0, n, estim=estim, result_type=rt, k=k)
            want = pairs_ref.pick_rect(rect, lhs, rhs)
            hi = np.asarray(lhs) > np.asarray(rhs)
            if hi.any():
                tri = ctx.dist_rows(estim=estim, result_type=rt, k=k)
                assert np.array_equal(bits(got[t][hi]), bits(pairs_ref.pick_tri(tri, n, np.asarray(lhs)[hi], np.asarray(rhs)[hi]))), \
                    "fuzz seed %d, case %d of %d: n=%d p=%d estim=%d k=%d type %d against dist_rows, form %d" % (FUZZ_SEED, case, FUZZ_CASES, n, p, estim, k, rt, form)
            assert np.array_equal(bits(got[t]), bits(want)), \
                "fuzz seed %d, case %d of %d: n=%d p=%d estim=%d k=%d type %d against dist_rect, form %d" % (FUZZ_SEED, case, FUZZ_CASES, n, p, estim, k, rt, form)
