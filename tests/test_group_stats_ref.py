"""The two forms of the reference of dsh_group_stats* (tests/group_stats_ref.py) held to each other and to examples worked
out by hand.  CPU only."""
import numpy as np
import pytest

import group_stats_ref as R


def random_matrix(rng, n):
    V = rng.random((n, n)).astype(np.float32) * np.float32(1.5) - np.float32(0.25)
    V = np.triu(V, 1)
    V = V + V.T
    i, j = np.triu_indices(n, 1)
    special = [np.nan, 0.0, -0.0, np.inf, -np.inf, 2.0, -2.0, 2.5, 1e9, np.nextafter(np.float32(2), np.float32(0)), 0.5, 0.5, 0.25]
    for x in rng.choice(i.size, size=min(i.size, max(4 * len(special), i.size // 3)), replace=False):
        V[i[x], j[x]] = V[j[x], i[x]] = np.float32(special[int(rng.integers(len(special)))])
    return V


def labellings(rng, n):
    ar = np.arange(n, dtype=np.uint32)
    yield ar
    yield np.zeros(n, np.uint32)
    yield (ar % 2) % max(n, 1)
    ids = rng.choice(n, size=max(n // 5, 1), replace=False).astype(np.uint32)
    yield ids[rng.integers(ids.size, size=n)]  # not idempotent: a label need not be a member of its group


@pytest.mark.parametrize("descending", [True, False])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64])
def test_fast_form_equals_brute_force(n, descending):
    rng = np.random.default_rng(1000 * n + descending)
    for rep in range(3):
        V = random_matrix(rng, n)
        ref = R.Ref(V, descending)
        for lab in labellings(rng, n):
            got, want = ref.stats(lab), R.brute(V, lab, descending)
            assert R.same(got, want), (n, descending, rep, lab.tolist())
            assert [a.dtype for a in got] == [np.uint32, np.uint32, np.int64, np.float32]
            # what the definition implies
            med, cnt, sm, worst = got
            assert (lab[med] == lab).all() and (med[med] == med).all()
            assert (np.isnan(worst) == (cnt == 0)).all()
            assert np.array_equal(R.diameter(lab, worst, descending)[med], R.diameter(lab, worst, descending), equal_nan=True)


def test_hand_written_example():
    """slots 0..3 one group, slot 4 alone.  v01 is NaN, so cnt = 2, 2, 3, 3: the medoid is among {2, 3} whatever the sums
    of 0 and 1 are.  sum[2] = sum[3] = 1.25: the tie goes to the smaller slot, under both orders."""
    V = np.full((5, 5), np.nan, np.float32)

    def put(x, y, v):
        V[x, y] = V[y, x] = v

    put(0, 2, 0.5), put(1, 2, 0.25), put(0, 3, 0.25), put(1, 3, 0.5), put(2, 3, 0.5)
    put(0, 4, 0.75), put(3, 4, 1.0)  # other groups: never read
    lab = np.array([3, 3, 3, 3, 0], np.uint32)
    one = 1 << 30
    for descending in (True, False):
        med, cnt, sm, worst = R.Ref(V, descending).stats(lab)
        assert cnt.tolist() == [2, 2, 3, 3, 0]
        assert sm.tolist() == [3 * one // 4, 3 * one // 4, 5 * one // 4, 5 * one // 4, 0]
        assert med.tolist() == [2, 2, 2, 2, 4]
        assert worst[:4].tolist() == ([0.25, 0.25, 0.25, 0.25] if descending else [0.5, 0.5, 0.5, 0.5]) and np.isnan(worst[4])
        assert R.same((med, cnt, sm, worst), R.brute(V, lab, descending))
    # the sum decides where the counts tie: v23 smaller makes 3's sum the smaller one
    put(2, 3, 0.5), put(1, 3, 0.25)  # sums: 2: 1.25, 3: 1.0
    assert R.Ref(V, True).stats(lab)[0].tolist() == [2, 2, 2, 2, 4]
    assert R.Ref(V, False).stats(lab)[0].tolist() == [3, 3, 3, 3, 4]
    # without the NaN slot 0 has three pairs too, and the best sum of all under the similarity order
    put(0, 1, 1.0)  # sums: 0: 1.75, 1: 1.5, 2: 1.25, 3: 1.0
    assert R.Ref(V, True).stats(lab)[0].tolist() == [0, 0, 0, 0, 4]
    assert R.Ref(V, False).stats(lab)[0].tolist() == [3, 3, 3, 3, 4]


def test_q_rounds_exact_halves_to_even_and_inclusion_is_open_at_two():
    h = np.float32(2.0**-31)  # half a unit
    v = np.array([h, 3 * h, 5 * h, 7 * h, -h, -3 * h, -5 * h, 0.0, -0.0, 1.0, -1.0], np.float32)
    assert R.q(v).tolist() == [0, 2, 2, 4, 0, -2, -2, 0, 0, 1 << 30, -(1 << 30)]
    big = np.nextafter(np.float32(2), np.float32(0))
    assert R.q(big) == (1 << 31) - 128 and R.q(-big) == -((1 << 31) - 128)  # |q| < 2^31
    V = np.full((4, 4), np.nan, np.float32)
    for y, val in ((1, big), (2, 2.0), (3, -big)):
        V[0, y] = V[y, 0] = val
    med, cnt, sm, worst = R.Ref(V, True).stats(np.zeros(4, np.uint32))
    assert cnt.tolist() == [2, 1, 0, 1] and sm[0] == 0 and worst[0] == -big and np.isnan(worst[2])
    assert med.tolist() == [0, 0, 0, 0]
    # the two zeros are one value
    Z = np.full((3, 3), np.nan, np.float32)
    Z[0, 1] = Z[1, 0] = -0.0
    Z[0, 2] = Z[2, 0] = 0.0
    w = R.Ref(Z, False).stats(np.zeros(3, np.uint32))[3]
    assert (w == 0).all() and not np.signbit(w).any()
