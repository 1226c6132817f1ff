"""numpy reference of the nearest-neighbour selection (include/dashing_hip.h, dsh_knn): a dense [queries][references]
rectangle turned into (idx uint32 [nq][nn], val float32 [nq][nn]).  The total order k_topk and k_topk_merge implement:
value best-first (similarities descending, distances ascending), NaN ranks as the worst value and is REPORTED as NaN,
ties go to the lower slot, a query is never its own neighbour, missing entries are 0xFFFFFFFF with -inf (similarities)
or +inf (distances).  A NaN and a real value equal to that filler tie, and the lower slot wins."""
import numpy as np

from thr_ref import DISTANCE, SIMILARITY

FILL = 0xFFFFFFFF


def descending(result_type):
    """measure_descending (ctx.h) / emt2nntype (src/dashing.h:268-280)"""
    assert result_type in SIMILARITY or result_type in DISTANCE
    return result_type in SIMILARITY


def worst(result_type):
    return np.float32(-np.inf if descending(result_type) else np.inf)


def _keys(vals, result_type):
    """ascending sort keys of one row: NaN -> the worst value; similarities negated (-0.0 and 0.0 stay equal)"""
    k = np.asarray(vals).copy()
    k[np.isnan(k)] = worst(result_type)
    return -k if descending(result_type) else k


def _self_col(q, q_begin, r_begin, nr, exclude_self):
    s = q_begin + q - r_begin
    return s if exclude_self and 0 <= s < nr else -1


def select(dense, nn, q_begin, r_begin, exclude_self, result_type):
    """`dense` = [queries][references] float32 as dist_rect gives it; row q is slot q_begin + q, column r slot r_begin + r"""
    dense = np.asarray(dense, np.float32)
    assert dense.ndim == 2
    nq, nr = dense.shape
    idx = np.full((nq, nn), FILL, np.uint32)
    val = np.full((nq, nn), worst(result_type), np.float32)
    if nn == 0 or nr == 0:
        return idx, val
    order = np.argsort(_keys(dense, result_type), axis=1, kind="stable")  # stable: equal keys keep the lower slot first
    for q in range(nq):
        o = order[q]
        s = _self_col(q, q_begin, r_begin, nr, exclude_self)
        if s >= 0:
            o = o[o != s]
        o = o[:nn]
        idx[q, : o.size] = o + r_begin
        val[q, : o.size] = dense[q, o]  # (a NaN stays a NaN)
    return idx, val


def same(a, b):
    """both (idx, val) pairs equal bit for bit (values as uint32 words)"""
    return (a[0].dtype == np.uint32 and a[1].dtype == np.float32 and a[0].shape == np.shape(b[0]) and
            a[1].shape == np.shape(b[1]) and np.array_equal(a[0], np.asarray(b[0], np.uint32)) and
            np.array_equal(np.ascontiguousarray(a[1]).view(np.uint32),
                           np.ascontiguousarray(b[1], np.float32).view(np.uint32)))


# ---- comparison with values the device did not produce: the oracle, or dense values under the float 1/k ---------------
UNDECIDED_REL = 2e-6   # twice the 1e-6 relative contract between GPU and oracle values; floor 1e-9 as thr_ref
# Share of a case's LIST POSITIONS that may be undecided: a condition on the cases, not a measurement (the worst measured
# on the oracle alone is 1.25e-3: related_sketches(700, 12, seed=91), FULL_CONTAINMENT_DIST, nn = 64).  It bounds
# positions, not rows: there 54 of 700 rows (8 %) hold at least one undecided position.
UNDECIDED_CAP = 5e-3
JUMP = SIMILARITY      # the index measures and SIZES: max(0, .) gives an exact 0 on one side and ~1e-14 on the other


def _window(v):
    return UNDECIDED_REL * np.maximum(np.abs(v), 1e-9)


def _ref_keys(row, result_type):
    """float64 sort keys of a reference row; for the measures that jump at 0 every |v| < 1e-9 is one class (at_jump)"""
    k = _keys(np.asarray(row, np.float64), result_type)
    if result_type in JUMP:
        k[np.abs(k) < 1e-9] = 0.0
    return k


def check_tolerant(ref64, got_idx, got_val, nn, q_begin, r_begin, exclude_self, result_type):
    """asserts what a correct selection satisfies against reference values it was not computed from; returns
    (undecided list positions, list positions).  A position is decided when every reference candidate within
    UNDECIDED_REL of its value has exactly its value -- except the class |v| < 1e-9 of the measures that jump at 0, which
    is undecided as soon as it has two members.  A decided position holds the reference's index; where the reference has
    an exact tie there, it holds a member of that tie, and the members the list holds stand in slot order as far as the
    list's OWN values tie (the own-order check).  That is all a float32 reference can ask of its exact ties: a duplicated
    sketch ties on every implementation and so comes out by slot, but two values less than a float32 ulp apart tie in one
    arithmetic (the float 1/k, glibc) and not in the other (the double 1/k, the device), which then ranks them by value."""
    ref64 = np.asarray(ref64, np.float64)
    nq, nr = ref64.shape
    got_idx = np.asarray(got_idx)
    got_val = np.asarray(got_val)
    assert got_idx.dtype == np.uint32 and got_val.dtype == np.float32
    assert got_idx.shape == (nq, nn) and got_val.shape == (nq, nn)
    w32 = worst(result_type)
    fin = np.isfinite(ref64)
    scale = max(float(np.abs(ref64[fin]).max()) if fin.any() else 1.0, 1.0)
    undecided = positions = 0
    for q in range(nq):
        s = _self_col(q, q_begin, r_begin, nr, exclude_self)
        cand = nr - (1 if s >= 0 else 0)
        take = min(nn, cand)
        gi = got_idx[q].astype(np.int64)
        gv = got_val[q]
        # shape of the list: `take` real entries, then fillers
        assert (gi[:take] != FILL).all() and (gi[take:] == FILL).all(), (q, "count", take)
        assert (gv[take:].view(np.uint32) == w32.view(np.uint32)).all(), (q, "filler value")
        c = gi[:take] - r_begin
        assert ((c >= 0) & (c < nr)).all(), (q, "range")
        assert np.unique(c).size == take, (q, "duplicate")
        assert not (exclude_self and (gi[:take] == q_begin + q).any()), (q, "self")
        # values: the _close rule of tests/test_gpu_fuzz.py, and non-finite values equal in kind
        want = ref64[q, c]
        got = gv[:take].astype(np.float64)
        f = np.isfinite(want)
        assert (np.isfinite(got) == f).all() and (np.isnan(got) == np.isnan(want)).all(), (q, "finiteness")
        assert (got[~f & ~np.isnan(want)] == want[~f & ~np.isnan(want)]).all(), (q, "infinity")
        err = np.abs(got[f] - want[f])
        assert (err <= 1e-6 * np.maximum(np.abs(want[f]), 1e-9) + 1e-12 * scale).all(), (q, "value", err.max())
        # the list is sorted under the total order on its OWN float32 values, exactly
        ok = _keys(gv[:take], result_type)
        assert ((ok[:-1] < ok[1:]) | ((ok[:-1] == ok[1:]) & (c[:-1] < c[1:]))).all(), (q, "own order")
        if take == 0:
            continue
        # the reference's list
        rk = _ref_keys(ref64[q], result_type)
        ro = np.argsort(rk, kind="stable")
        if s >= 0:
            ro = ro[ro != s]
        w = rk[ro]  # ascending keys of all candidates
        # nothing left out is better than the last one taken by more than the window
        left = np.ones(nr, bool)
        left[c] = False
        if s >= 0:
            left[s] = False
        if left.any():
            last = rk[c[-1]]
            best_left = rk[left].min()
            if best_left < last:
                assert np.isfinite(best_left) and np.isfinite(last) and last - best_left <= _window(last), \
                    (q, "left out", best_left, last)
        # decided positions hold the reference's index
        wt = w[:take]
        finite = np.isfinite(wt)
        win = np.where(finite, _window(np.where(finite, wt, 0.0)), 0.0)
        with np.errstate(invalid="ignore"):
            lo = np.searchsorted(w, np.where(finite, wt - win, wt), side="left")
            hi = np.searchsorted(w, np.where(finite, wt + win, wt), side="right") - 1
        decided = (w[lo] == wt) & (w[hi] == wt)
        if result_type in JUMP:
            decided &= ~((wt == 0.0) & (hi > lo))
        pos = np.empty(nr, np.int64)
        pos[ro] = np.arange(ro.size)  # place of a candidate in the reference's list
        ok = (pos[c] >= lo) & (pos[c] <= hi)
        assert ok[decided].all(), (q, "decided index", np.flatnonzero(decided & ~ok)[:5])
        undecided += int((~decided).sum())
        positions += take
    return undecided, positions


_ORACLE_RECT = {}


def oracle_rect(oracle, case):
    """(regs, float64 [n][n] rectangle of the ORACLE under the double 1/k dsho_knn reports) of an oracle case, computed
    once per process; `oracle` is the fixture of tests/conftest.py"""
    name, make_regs, rt, k, _ = case
    if (name, rt, k) not in _ORACLE_RECT:
        regs = make_regs()
        _ORACLE_RECT[(name, rt, k)] = (regs, oracle.dist_rect(regs, regs, 2, rt, k, ksinv_double=True).astype(np.float64))
    return _ORACLE_RECT[(name, rt, k)]


def oracle_cases():
    """(name, make_regs, result_type, k, nn) the GPU test compares with the oracle; tests/test_knn_ref.py holds every
    entry's undecided share, measured on the oracle alone, to UNDECIDED_CAP"""
    from dashing_amd import synth

    def c300():
        r = synth.synthetic_sketches(300, 10, seed=55)
        r[7] = r[8] = r[9]
        r[20] = 0
        return r

    def c700():
        return synth.related_sketches(700, 12, seed=91)[0]

    def c3000():
        return synth.survey_sketches(3000, 12, seed=0x5EED0000)[0]

    return [
        # (JI and SYMMETRIC_CONTAINMENT_INDEX at nn = 64 are not here: a third of this collection's rows have fewer than 64
        # non-zero similarities, the zeros are ONE undecided class of the measures that jump at 0, and the share is 1.6 %)
        ("synthetic300p10", c300, 1, 21, 32),
        ("synthetic300p10", c300, 0, 21, 64),
        ("synthetic300p10", c300, 7, 21, 32),
        ("synthetic300p10", c300, 7, 21, 5),
        ("synthetic300p10", c300, 5, 21, 17),
        ("synthetic300p10", c300, 4, 21, 1),
        ("related700p12", c700, 1, 31, 64),
        ("related700p12", c700, 4, 31, 64),
        ("related700p12", c700, 0, 31, 33),
        ("related700p12", c700, 5, 31, 7),
        ("survey3000p12", c3000, 1, 31, 10),
        ("survey3000p12", c3000, 0, 31, 64),
        ("survey3000p12", c3000, 5, 31, 2),
    ]
