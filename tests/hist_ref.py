"""numpy reference of the value histograms (include/dashing_hip.h, dsh_dist_histogram*): float32 values counted over
strictly increasing float32 edges into n_edges + 2 classes.  The closed side of an edge is the side that passes as a
threshold: similarity forms class(v) = #{e : e <= v} (bins [e_{b-1}, e_b)), *_DIST forms class(v) = #{e : e < v} (bins
(e_{b-1}, e_b]); NaN is class n_edges + 1.  With a `same` mask (the pair's two slots carry equal labels) the counts come
in two planes: 0 intra, 1 inter."""
import numpy as np

# bns::EmissionType numbers; the similarity forms rank descending (tests/thr_ref.py)
SIMILARITY = frozenset((1, 2, 5, 7))


def classes(values, edges, descending):
    """class of every value (int64, the shape of `values`)"""
    v = np.asarray(values, np.float32)
    e = np.asarray(edges, np.float32).reshape(-1)
    nan = np.isnan(v)
    safe = np.where(nan, np.float32(0), v)  # NaN is masked BEFORE the search: searchsorted sorts it behind +inf
    k = np.searchsorted(e, safe.reshape(-1), side="right" if descending else "left").astype(np.int64).reshape(v.shape)
    k[nan] = e.size + 1
    return k


def count_classes(k, n_edges, same=None):
    """the classes `k` of classes() counted: uint64 (planes, n_edges + 2)"""
    k = np.asarray(k, np.int64).reshape(-1)
    nclass = n_edges + 2
    if same is None:
        return np.bincount(k, minlength=nclass).astype(np.uint64).reshape(1, nclass)
    s = np.asarray(same, bool).reshape(-1)
    assert s.size == k.size
    return np.bincount(k + np.where(s, 0, nclass), minlength=2 * nclass).astype(np.uint64).reshape(2, nclass)


def histogram(values, edges, descending, same=None):
    """uint64 (planes, n_edges + 2); same: None (one plane) or a bool array of the shape of `values`"""
    e = np.asarray(edges, np.float32).reshape(-1)
    return count_classes(classes(values, e, descending), e.size, same)


def hits(counts, descending):
    """per edge b the values that pass a threshold at edges[b]: the cumulative sums of the contract, NaN class excluded"""
    c = np.asarray(counts, np.uint64)
    body = c[..., :-1].astype(np.int64)
    if descending:
        return np.cumsum(body[..., ::-1], axis=-1)[..., ::-1][..., 1:].astype(np.uint64)
    return np.cumsum(body, axis=-1)[..., :-1].astype(np.uint64)


def tri_ij(n, row_begin=0, row_end=None):
    """(i, j) of every value of rows [row_begin, row_end) of the packed triangle of n sketches, in dist_rows order"""
    row_end = n if row_end is None else min(row_end, n)
    rows = np.arange(row_begin, max(row_end, row_begin), dtype=np.int64)
    lens = n - 1 - rows
    i = np.repeat(rows, lens)
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    j = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(starts, lens) + i + 1
    return i, j


def rect_ij(q_begin, q_end, r_begin, r_end):
    """(query slot, reference slot) of every value of dist_rect, row-major"""
    q = np.arange(q_begin, max(q_end, q_begin), dtype=np.int64)
    r = np.arange(r_begin, max(r_end, r_begin), dtype=np.int64)
    return np.repeat(q, r.size), np.tile(r, q.size)


def tri_same(labels, n, row_begin=0, row_end=None):
    lab = np.asarray(labels)
    i, j = tri_ij(n, row_begin, row_end)
    return lab[i] == lab[j]


def rect_same(labels, q_begin, q_end, r_begin, r_end):
    lab = np.asarray(labels)
    i, j = rect_ij(q_begin, q_end, r_begin, r_end)
    return lab[i] == lab[j]
