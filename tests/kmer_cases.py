"""k-mers MADE for a wanted register: Thomas Wang's hash is a bijection of 64-bit words (tests/hashinv.py), so for every
precision p, index and value the hashes that leave exactly that (index, value) can be written down and inverted until the
preimage is a k-mer.  Pure Python and numpy: the helper of tests/test_kmer_cases.py (CPU) and
tests/test_gpu_sketch_values.py (device).

A hash leaves (index, value) at precision p, q = 64 - p, iff its top p bits are the index and its low q bits begin with
value - 1 zeros: for value <= q a one follows and the q - value bits behind it are FREE; value = q + 1 is the all-zero
tail, one hash per index.  The expected registers follow from this construction alone (one_hot), not from the oracle's
or the kernel's reading of the rule."""
import numpy as np

from hashinv import revcomp, unwang

M64 = (1 << 64) - 1
BUDGET = 4096  # inversions one make() may spend
_LETTERS = np.frombuffer(b"ACGT", np.uint8)


def V(p):
    """The values every sketch instance is held to at precision p: the two smallest; both sides of the 32|33 edge, where
    the high word of t = (h << p) | guard runs out (31, 32 from the high word; 33, 34 from the low word, 33 being
    zl + 32 with zl = 0); and the top of the domain, where only the guard bit tells q from q + 1."""
    q = 64 - p
    return sorted({1, 2, 31, 32, 33, 34, q - 1, q, q + 1})


def rule(h, p):
    """the register rule in Python integers: (index, value) of the hash h at precision p"""
    t = ((h << p) | (1 << (p - 1))) & M64
    return h >> (64 - p), (64 - t.bit_length()) + 1


def make(p, value, k, canon, index=None, skip=0, start=0, budget=BUDGET):
    """The k-mer x (k bases as 2-bit codes, first base most significant; its own canonical form if canon) whose hash
    leaves (index, value) at precision p, as (x, index); None when `budget` inversions did not find one.  Deterministic:
    indices upward from `start` (wrapping), inside an index the free low bits upward; with `index` that index only.
    skip: pass over that many k-mers that would have been returned (a second, third ... k-mer of the cell)."""
    q = 64 - p
    assert 4 <= p <= 24 and 1 <= value <= q + 1 and 1 <= k <= 32
    nfree = q - value if value <= q else 0
    top = (1 << (q - value)) if value <= q else 0
    indices = [index] if index is not None else ((start + i) & ((1 << p) - 1) for i in range(1 << p))
    tries = 0
    for idx in indices:
        for free in range(1 << nfree):
            if tries == budget:
                return None
            tries += 1
            x = unwang((idx << q) | top | free)
            if x >> (2 * k) or (canon and revcomp(x, k) < x):
                continue
            if skip:
                skip -= 1
                continue
            return x, idx
    return None


def text(x, k):
    """the k-mer as ASCII bases (uint8 array)"""
    return _LETTERS[[(x >> (2 * (k - 1 - t))) & 3 for t in range(k)]]


def rc_text(x, k):
    """the text of the reverse complement"""
    return text(revcomp(x, k), k)


def one_hot(p, index, value):
    row = np.zeros(1 << p, np.uint8)
    row[index] = value
    return row


def spread(p, *salt):
    """a deterministic index of [0, 2^p) that moves with every salt (where make()'s walk over the indices starts)"""
    z = 0x9E3779B97F4A7C15
    for s in salt:
        z = ((z ^ (int(s) + 1)) * 0xBF58476D1CE4E5B9) & M64
        z ^= z >> 29
    return z >> (64 - p)
