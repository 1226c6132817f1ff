"""CPU: the numpy reference of the value histograms (tests/hist_ref.py) against a brute-force loop, np.histogram and the
threshold predicate of tests/thr_ref.py; dashing_amd.histogram_hits; and the grid rule of k_hist (plan::hist_grid through
dshh_hist_grid of csrc/host/plan_capi.cpp)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import dashing_amd
import hist_ref as H
import thr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 0.5, np.nextafter(F(0.5), F(1)), np.nextafter(F(0.5), F(0))], F)


def brute_class(v, edges, descending):
    if math.isnan(v):
        return len(edges) + 1
    return sum(1 for e in edges if (e <= v if descending else e < v))


def cases():
    rng = np.random.default_rng(7)
    out = []
    for ne in (1, 2, 5, 33):
        pool = np.unique(np.concatenate([rng.random(ne * 2).astype(F), np.array([0.0, 0.5, 1.0, -np.inf, np.inf], F)]))
        edges = np.sort(rng.choice(pool, size=min(ne, pool.size), replace=False)).astype(F)
        vals = np.concatenate([rng.random(200).astype(F), SPECIAL, edges, rng.choice(edges, 40)]).astype(F)
        rng.shuffle(vals)
        out.append((edges, vals))
    out.append((np.array([-np.inf, 0.0, np.inf], F), np.concatenate([SPECIAL, F(rng.standard_normal(50))]).astype(F)))
    return out


@pytest.mark.parametrize("descending", [True, False])
def test_reference_equals_a_brute_force_loop(descending):
    for edges, vals in cases():
        want = np.array([brute_class(float(v), [float(e) for e in edges], descending) for v in vals], np.int64)
        got = H.classes(vals, edges, descending)
        assert np.array_equal(got, want), (edges, descending)
        same = np.arange(vals.size) % 3 == 0
        hist = H.histogram(vals, edges, descending, same)
        assert hist.dtype == np.uint64 and hist.shape == (2, edges.size + 2)
        for plane, mask in ((0, same), (1, ~same)):
            assert np.array_equal(hist[plane], np.bincount(want[mask], minlength=edges.size + 2))
        one = H.histogram(vals, edges, descending)
        assert one.shape == (1, edges.size + 2) and np.array_equal(one[0], hist[0] + hist[1]) and int(one.sum()) == vals.size
        assert int(one[0, -1]) == int(np.isnan(vals).sum())


def test_both_zeros_are_one_value_and_sit_on_the_closed_side():
    edges = np.array([0.0], F)
    z = np.array([0.0, -0.0], F)
    assert H.classes(z, edges, True).tolist() == [1, 1]   # e <= v: a threshold of 0 passes both
    assert H.classes(z, edges, False).tolist() == [0, 0]  # e < v: neither is above 0; v <= 0 passes
    assert H.classes(z, np.array([-0.0], F), True).tolist() == [1, 1]


def test_similarity_closure_is_np_histogram_on_interior_bins():
    rng = np.random.default_rng(11)
    edges = np.linspace(0, 1, 21).astype(F)
    vals = np.concatenate([rng.random(5000).astype(F), edges[:-1]])  # (np.histogram closes its LAST bin on both sides)
    want, _ = np.histogram(vals, bins=edges)
    got = H.histogram(vals, edges, True)[0]
    assert np.array_equal(got[1:-2], want) and got[0] == 0 and got[-2] == 0 and got[-1] == 0


@pytest.mark.parametrize("rt", range(9))
def test_cumulative_sums_are_the_hit_counts_of_the_threshold_predicate(rt):
    descending = rt in thr_ref.SIMILARITY
    assert descending == (rt in H.SIMILARITY)
    for edges, vals in cases():
        counts = H.histogram(vals, edges, descending, np.arange(vals.size) % 2 == 0)
        want = np.array([int(thr_ref.passes(vals, e, rt).sum()) for e in edges], np.uint64)
        got = H.hits(counts, descending)
        assert got.shape == (2, edges.size) and np.array_equal(got.sum(axis=0), want)
        mine = dashing_amd.histogram_hits(counts, rt)
        assert mine.dtype == np.uint64 and np.array_equal(mine, got)
        flat = dashing_amd.histogram_hits(counts.sum(axis=0), rt)
        assert flat.shape == (edges.size,) and np.array_equal(flat, want)


def test_histogram_hits_takes_the_direction_of_the_library():
    """SIZES is no *_DIST form: the library ranks it descending and passes a threshold with v >= t"""
    assert sorted(dashing_amd.DISTANCE_TYPES) == sorted(thr_ref.DISTANCE) and dashing_amd.SIZES in thr_ref.SIMILARITY
    counts = np.array([[1, 2, 4, 8, 16]], np.uint64)  # three edges; 16 NaN
    for rt in range(9):
        want = [2 + 4 + 8, 4 + 8, 8] if rt in thr_ref.SIMILARITY else [1, 1 + 2, 1 + 2 + 4]
        assert dashing_amd.histogram_hits(counts, rt).tolist() == [want], rt
    for bad in (-1, 9, True):
        with pytest.raises(ValueError):
            dashing_amd.histogram_hits(counts, bad)


def test_histogram_hits_refuses_what_is_no_histogram():
    with pytest.raises(ValueError):
        dashing_amd.histogram_hits(np.zeros(2, np.uint64), 1)
    with pytest.raises(ValueError):
        dashing_amd.histogram_hits(np.zeros((1, 1, 5), np.uint64), 1)


def test_position_helpers():
    n = 7
    i, j = H.tri_ij(n)
    assert i.size == n * (n - 1) // 2 and (j > i).all()
    assert [(int(a), int(b)) for a, b in zip(i, j)] == [(a, b) for a in range(n) for b in range(a + 1, n)]
    i, j = H.tri_ij(n, 2, 5)
    assert [(int(a), int(b)) for a, b in zip(i, j)] == [(a, b) for a in range(2, 5) for b in range(a + 1, n)]
    assert H.tri_ij(n, 5, 3)[0].size == 0 and H.tri_ij(1)[0].size == 0
    i, j = H.rect_ij(1, 3, 0, 4)
    assert [(int(a), int(b)) for a, b in zip(i, j)] == [(a, b) for a in (1, 2) for b in range(4)]
    lab = np.array([5, 5, 9, 5, 9, 1, 1])
    assert H.tri_same(lab, n).sum() == 3 + 1 + 1 and H.rect_same(lab, 0, 7, 0, 7).sum() == 9 + 4 + 4


# ---- the grid rule ---------------------------------------------------------------------------------------------------
MAX_ITERS = (1 << 18) - 1


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    lib.dshh_hist_grid.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.dshh_hist_grid.restype = C.c_uint64
    return lib


def model_grid(units, lds, cus):
    per_cu = min(max((160 << 10) // max(lds, 1), 1), 8)
    need = -(-units // 4)
    least = -(-units // (4 * MAX_ITERS))
    return max(min(need, max(cus, 1) * per_cu), least, 1)


def test_grid_rule(host):
    ldss = (12, 816, 20 << 10, 49168, 160 << 10, 1 << 20)
    for units in (0, 1, 3, 4, 5, 1023, 8192, 8193, 10**6, 4 * MAX_ITERS * 768, 4 * MAX_ITERS * 768 + 1, 1 << 38):
        for lds in ldss:
            for cus in (1, 256):
                it = C.c_uint64()
                g = host.dshh_hist_grid(units, lds, cus, C.byref(it))
                assert g == model_grid(units, lds, cus), (units, lds, cus)
                assert 1 <= g < 1 << 31
                # every unit is taken: four waves a workgroup, `it` trips each
                assert 4 * g * it.value >= units and it.value == -(-units // (4 * g))
                # a workgroup's share stays inside its 32-bit counters whatever the band holds
                assert it.value <= MAX_ITERS and 4 * it.value * 4096 < 1 << 32
                # never more workgroups than units need, and bounded by the device unless the counters force more
                assert g <= max(-(-units // 4), 1)
                if -(-units // (4 * MAX_ITERS)) <= cus * 8:
                    assert g <= cus * 8
    # small histograms keep occupancy, the largest still fits three to a compute unit
    assert host.dshh_hist_grid(1 << 24, 816, 256, None) == 256 * 8
    assert host.dshh_hist_grid(1 << 24, 49168, 256, None) == 256 * 3
