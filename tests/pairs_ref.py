"""Plain numpy/oracle reference of the explicit pair list (include/dashing_hip.h, dsh_dist_pairs*): for a pair
(lhs, rhs) the value is result_cmp(lhs = sketch[lhs], rhs = sketch[rhs]) composed exactly as the oracle's dsho_pair
composes it (oracle/dsh_oracle.c:505-513) -- union histogram, estimate, the two cardinalities, then the J arm or the
triple arm -- plus the helpers that pick the dense values of a pair list out of a dist_rows span and a dist_rect matrix."""
import numpy as np

ALL_TYPES = (0, 1, 2, 3, 4, 5, 6, 7, 8)  # bns::EmissionType numbers (include/dashing_hip.h)
J_ARM = frozenset((0, 1, 3))             # MASH_DIST, JI, FULL_MASH_DIST go through the Jaccard index


def pair_values(oracle, regs, lhs, rhs, result_types=(1,), estim=2, k=31):
    """float32 [n_types][n_pairs], pair by pair through the oracle's scalar entry points"""
    regs = np.ascontiguousarray(regs, np.uint8)
    p = int(regs.shape[1]).bit_length() - 1
    lhs = np.asarray(lhs, np.int64).reshape(-1)
    rhs = np.asarray(rhs, np.int64).reshape(-1)
    card = oracle.cardinalities(regs, estim)
    out = np.zeros((len(result_types), lhs.size), np.float32)
    for x in range(lhs.size):
        a, b = int(lhs[x]), int(rhs[x])
        us = oracle.estimate(oracle.hist_union(regs[a], regs[b]), p, estim)
        ca, cb = float(card[a]), float(card[b])
        for t, rt in enumerate(result_types):
            if rt in J_ARM:
                out[t, x] = oracle.result(oracle.jaccard_from(ca, cb, us), rt, k)
            else:
                out[t, x] = oracle.result_triple(ca, cb, us, rt, k)
    return out


def tri_index(n, i, j):
    """position of (i, j > i) in the packed triangle of n sketches (dsh_tri_index)"""
    i = np.asarray(i, np.int64)
    j = np.asarray(j, np.int64)
    return i * n - i * (i + 1) // 2 + (j - i - 1)


def pick_tri(span, n, lhs, rhs):
    """the values of the pairs (lhs = j > rhs = i) out of the full packed triangle `span` (dist_rows / dist_tri)"""
    lhs = np.asarray(lhs, np.int64)
    rhs = np.asarray(rhs, np.int64)
    assert (lhs > rhs).all()
    return np.asarray(span)[tri_index(n, rhs, lhs)]


def pick_rect(mat, lhs, rhs, q_begin=0, r_begin=0):
    """the values of the pairs out of a dist_rect matrix [query = rhs][reference = lhs]"""
    return np.asarray(mat)[np.asarray(rhs, np.int64) - q_begin, np.asarray(lhs, np.int64) - r_begin]


def all_tri_pairs(n):
    """every pair (lhs = j, rhs = i), i < j, in the order of the packed triangle"""
    i, j = np.triu_indices(n, 1)
    return j.astype(np.uint32), i.astype(np.uint32)


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
