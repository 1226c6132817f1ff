"""GPU: the life of a context.  Everything a context holds on the device and in page-locked memory is released by its
owners when it is destroyed (csrc/ctx.h), and dsh_destroy waits for what the context has enqueued first
(include/dashing_hip.h).  Contexts are made, put through one smallest call of every module that owns state, and closed,
three times over: the third cycle must give bit for bit what the first gave, and the dense values those of the session
context.  A context closed right behind asynchronous calls must have delivered their results.

n = 130 sketches at p = 10: one full 128-row tile and a partial one, the smallest shape that crosses a tile boundary
(nothing under test depends on size beyond that)."""
import numpy as np
import pytest

import dashing_amd
from dashing_amd import synth

pytestmark = pytest.mark.gpu

D = dashing_amd
N, P, K = 130, 10, 31
REGS = synth.synthetic_sketches(N, P, seed=0x11FEC7C1)
GENOME = synth.concat_for_device(synth.synthetic_genomes(1, 300, seed=0x11FE, decorate=False))
RECORDS = synth.concat_for_device(synth.synthetic_genomes(3, 90, seed=0x11FF, decorate=False))


@pytest.fixture(scope="module")
def base(ctx):
    """the session context's dense values of REGS (computed once), and a threshold taken from them that selects the top
    twentieth of the pairs: neither none nor all"""
    ctx.set_sketches(REGS)
    dense = ctx.dist_rows(k=K).copy()
    t = float(np.sort(dense)[dense.size - dense.size // 20])
    assert 0 < int((dense >= t).sum()) < dense.size
    return dense, t


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def one_cycle(t):
    """a fresh context through one smallest call of every module that owns state, then closed: {name: arrays}"""
    out = {}
    with D.Context(0) as c:
        c.set_sketches(REGS)
        out["sketch_batch"] = [c.sketch_batch(GENOME[0], GENOME[1], 0, K, True)]
        out["sketch_records"] = [c.sketch_records(RECORDS[0], RECORDS[1], 1, K, True)]
        c.upload(REGS[:4], 0)  # (the rows the sketch calls wrote: the compare calls below see REGS again)
        out["dist_rows"] = [c.dist_rows(k=K).copy()]
        out["dist_rect"] = [c.dist_rect(0, 7, 100, N, k=K)]
        out["knn"] = list(c.knn(3, k=K))
        out["dist_threshold"] = list(c.dist_threshold(t, k=K))
        lhs, rhs = np.array([5, 129, 64, 128, 9], np.uint32), np.array([0, 1, 63, 127, 8], np.uint32)
        out["dist_pairs"] = [c.dist_pairs(lhs, rhs, k=K)]
        labels, nc = c.cluster_threshold(t, k=K)
        out["cluster_threshold"] = [labels, nc]
        out["cluster_pairs"] = list(c.cluster_pairs(10, [1, 2, 7, 9], [0, 1, 8, 9]))
        out["greedy_threshold"] = list(c.greedy_threshold(t, k=K))
        out["greedy_extend"] = list(c.greedy_extend(t, assign="best", k=K))
        out["group_stats"] = list(c.group_stats(labels, k=K))
        out["dist_histogram"] = [c.dist_histogram([t / 2, t], k=K)]
        out["linkage_threshold"] = list(c.linkage_threshold(t, "complete", k=K))
        out["fold"] = [c.fold(9)]
        out["union_groups"] = [c.union_groups([0, 2, 5], [0, 1, 2, 3, 4])]
    return out


def test_three_cycles_give_the_same(ctx, base):
    dense, t = base
    cycles = [one_cycle(t) for _ in range(3)]
    for cyc in cycles:
        assert same_bits(cyc["dist_rows"][0], dense)
    first, third = cycles[0], cycles[2]
    assert first.keys() == third.keys()
    for name in first:
        assert len(first[name]) == len(third[name])
        for a, b in zip(first[name], third[name]):
            assert same_bits(a, b), name
    # the selections were neither empty nor everything
    row_ptr = first["dist_threshold"][0]
    assert 0 < int(row_ptr[-1]) < dense.size
    assert 1 < first["cluster_threshold"][1] < N and 1 < first["greedy_threshold"][1] < N


def test_close_right_behind_async_calls(ctx, base):
    """dsh_destroy waits for everything the context has enqueued before it releases anything: the rows asked for with
    dsh_dist_rows_async are in the caller's page-locked array when close() returns, with no wait in between"""
    dense, _ = base
    pin = D.PinnedArray(dense.size, np.float32)
    pin.array[:] = np.nan
    seq = D.PinnedArray(GENOME[0].size, np.uint8)
    seq.array[:] = GENOME[0]
    c = D.Context(0)
    c.set_sketches(REGS)
    c.dist_rows_async(pin.array, k=K)
    c.sketch_batch_async(seq.array, GENOME[1], 0, K, True)  # (behind the rows on the stream: they do not see it)
    c.close()
    assert same_bits(pin.array[: dense.size], dense)
