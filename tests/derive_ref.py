"""numpy model of the derived-sketch operations (dsh_fold*, dsh_upload_sketches_folded*, dsh_union_groups*), written from
the hash argument, not from the host loop it checks (tests/test_derive_ref.py pins the two against each other).

A register of value v at index idx of a p-bit sketch stands for a 64-bit hash whose top p bits are idx and whose
remaining 64 - p bits begin with v - 1 zeros (v = 64 - p + 1: all of them are zero).  Folding to new_p re-reads that same
hash at the lower precision: the index is its top new_p bits, and the index bits that were dropped become the leading
bits of the remainder.  So the model rebuilds one such hash per non-empty register, inserts it into an empty sketch of
precision new_p the way sketching does, and keeps the maximum per register."""
import numpy as np

_POW2 = np.array([1 << k for k in range(64)], np.uint64)


def _bit_length(x):
    """exact bit length of uint64 values (0 -> 0)"""
    return np.searchsorted(_POW2, x, side="right").astype(np.int64)


def fold(rows, new_p):
    rows = np.ascontiguousarray(rows, np.uint8)
    n, m = rows.shape
    p = int(m).bit_length() - 1
    assert m == 1 << p and 0 <= new_p <= p
    out = np.zeros(n << new_p, np.uint8)
    flat = rows.reshape(-1)
    at = np.flatnonzero(flat)
    if not at.size:
        return out.reshape(n, 1 << new_p)
    v = flat[at].astype(np.int64)
    assert v.max() <= 64 - p + 1, "not a sketch of precision %d" % p
    row, idx = at >> p, (at & (m - 1)).astype(np.uint64)
    q = 64 - p
    # a hash that leaves exactly (idx, v): index bits on top, then v - 1 zeros and a one (nothing at all for v = q + 1)
    one = np.where(v <= q, np.left_shift(np.uint64(1), np.clip(q - v, 0, 63).astype(np.uint64)), np.uint64(0))
    h = np.left_shift(idx, np.uint64(q)) | one if p else one
    nq = 64 - new_p
    nidx = np.right_shift(h, np.uint64(nq)) if new_p else np.zeros_like(h)
    rest = h & np.uint64((1 << nq) - 1)
    nv = (nq - _bit_length(rest) + 1).astype(np.uint8)  # leading zeros of the remainder in its nq-bit field, plus one
    np.maximum.at(out, (row << new_p) + nidx.astype(np.int64), nv)
    return out.reshape(n, 1 << new_p)


def union_groups(rows, group_ptr, members):
    rows = np.ascontiguousarray(rows, np.uint8)
    gp = np.asarray(group_ptr, np.int64)
    mem = np.asarray(members, np.int64)
    out = np.zeros((gp.size - 1, rows.shape[1]), np.uint8)
    for g in range(gp.size - 1):
        if gp[g + 1] > gp[g]:
            out[g] = np.maximum.reduce(rows[mem[gp[g] : gp[g + 1]]], axis=0)
    return out
