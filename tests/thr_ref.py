"""numpy reference of the thresholded output (include/dashing_hip.h, dsh_dist_threshold*): a dense packed span of the
triangle, or a dense rectangle, turned into (row_ptr uint64, col uint32, val float32).  The comparison is a float32
comparison of the stored value with the float32 threshold: similarities pass with v >= t, distances with v <= t, NaN
never; rows ascending, columns ascending inside a row; row_ptr relative to the first row."""
import numpy as np

# bns::EmissionType numbers (include/dashing_hip.h); the similarity forms rank descending (emt2nntype)
SIMILARITY = frozenset((1, 2, 5, 7))  # JI, SIZES, CONTAINMENT_INDEX, SYMMETRIC_CONTAINMENT_INDEX
DISTANCE = frozenset((0, 3, 4, 6, 8))


def passes(vals, t, result_type):
    v = np.asarray(vals, np.float32)
    t = np.float32(t)
    assert result_type in SIMILARITY or result_type in DISTANCE
    with np.errstate(invalid="ignore"):
        return (v >= t) if result_type in SIMILARITY else (v <= t)


def row_lengths(n, row_begin, row_end):
    row_end = min(row_end, n)
    return np.array([n - 1 - i for i in range(row_begin, max(row_end, row_begin))], np.int64)


def tri(span, n, row_begin, row_end, t, result_type):
    """`span` = the dense values of rows [row_begin, row_end) of the packed triangle of n sketches (dist_rows)"""
    span = np.asarray(span, np.float32)
    lens = row_lengths(n, row_begin, row_end)
    assert span.size == int(lens.sum())
    hit = passes(span, t, result_type)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    row_ptr = np.zeros(lens.size + 1, np.uint64)
    if lens.size:
        csum = np.concatenate([[0], np.cumsum(hit, dtype=np.int64)])
        row_ptr[:] = csum[starts]
    pos = np.flatnonzero(hit)
    row = np.searchsorted(starts, pos, side="right") - 1  # (rows without values repeat a start: side=right takes the last)
    col = (row_begin + row + 1 + (pos - starts[row])).astype(np.uint32)
    return row_ptr, col, span[pos].copy()


def rect(dense, r_begin, t, result_type):
    """`dense` = [queries][references] as dist_rect gives it; col = reference slot"""
    dense = np.asarray(dense, np.float32)
    assert dense.ndim == 2
    hit = passes(dense, t, result_type)
    row_ptr = np.concatenate([[0], np.cumsum(hit.sum(axis=1), dtype=np.int64)]).astype(np.uint64)
    q, r = np.nonzero(hit)
    return row_ptr, (r + r_begin).astype(np.uint32), dense[q, r].copy()


def same(a, b):
    """both CSR triples equal bit for bit (values as uint32 words)"""
    return (a[0].dtype == np.uint64 and a[1].dtype == np.uint32 and a[2].dtype == np.float32 and
            np.array_equal(a[0], np.asarray(b[0], np.uint64)) and np.array_equal(a[1], np.asarray(b[1], np.uint32)) and
            np.array_equal(np.asarray(a[2]).view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32)))


# ---- comparison with the oracle, "undecided pairs" (tests/test_gpu_threshold.py, item 3) -------------------------------
UNDECIDED_REL = 2e-6   # twice the 1e-6 relative contract between GPU and oracle values (RTOL, tests/test_gpu_compare.py)
UNDECIDED_CAP = 1e-5   # share of a case's pairs that may be undecided


def undecided(oracle_vals, t):
    """pairs whose ORACLE value lies so close to t that the GPU value may fall on either side"""
    v = np.asarray(oracle_vals, np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(v - t) <= UNDECIDED_REL * max(abs(t), 1e-9)


def oracle_cases():
    """(name, make_regs, result_type, k, thresholds) the GPU test compares with the oracle; no exact-tie thresholds"""
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
        ("synthetic300p10", c300, 1, 21, (0.03, 0.3, 0.9)),
        ("synthetic300p10", c300, 0, 21, (0.05, 0.1, 0.2)),
        ("related700p12", c700, 1, 31, (0.01, 0.03, 0.3, 0.9)),
        ("related700p12", c700, 0, 31, (0.02, 0.1, 0.2)),
        ("related700p12", c700, 5, 31, (0.05, 0.5)),
        ("related700p12", c700, 6, 31, (0.02, 0.1)),
        ("survey3000p12", c3000, 1, 31, (0.01, 0.03, 0.3, 0.9)),
        ("survey3000p12", c3000, 0, 31, (0.05, 0.1, 0.2)),
    ]
