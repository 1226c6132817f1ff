"""The k-mer maker of tests/kmer_cases.py, on the CPU: every cell of p = 4 ... 24 x V(p) x k in {31, 32} x canonical or not
holds a k-mer; its hash leaves the wanted (index, value) under the rule in Python integers; both oracles sketch the bare
k-mer -- a genome of exactly k bases -- to exactly the one-hot row of the construction; and V(p) is rich enough that every
restated mistake of the register rule shows on one of its k-mers at every p."""
import numpy as np
import pytest

import kmer_cases as kc
import oracle.oracle_py as opy
from dashing_amd import synth
from hashinv import revcomp

PS = range(4, 25)
KCS = [(31, True), (31, False), (32, True), (32, False)]


def cells(p):
    for k, canon in KCS:
        for v in kc.V(p):
            yield k, canon, v, kc.make(p, v, k, canon)


def test_value_set():
    for p in PS:
        q = 64 - p
        assert set(kc.V(p)) >= {1, 2, 31, 32, 33, 34, q - 1, q, q + 1} and max(kc.V(p)) == q + 1


def test_rule_agrees_with_the_oracles_rule_but_is_not_it():
    rng = np.random.default_rng(5)
    for p in PS:
        for h in [0, 1, kc.M64, 1 << (64 - p), (1 << (64 - p)) - 1, 1 << 31, 1 << 32] + [int(x) for x in rng.integers(0, 1 << 63, 50)]:
            assert kc.rule(h, p) == opy.reg_rule(h, p)


@pytest.mark.parametrize("p", PS)
def test_every_cell_holds_a_kmer_with_the_wanted_register(p):
    """completeness is a condition: no cell may be empty"""
    n = 0
    for k, canon, v, made in cells(p):
        assert made is not None, "no k-mer for p=%d value=%d k=%d canon=%s within %d inversions" % (p, v, k, canon, kc.BUDGET)
        x, idx = made
        assert 0 <= x < 4 ** k
        assert kc.rule(opy.wang(x), p) == (idx, v)
        if canon:
            assert revcomp(x, k) >= x
        assert opy.kmers(kc.text(x, k).tobytes(), k, False) == [x] and opy.kmers(kc.rc_text(x, k).tobytes(), k, False) == [revcomp(x, k)]
        n += 1
    assert n == len(KCS) * len(kc.V(p))


def test_the_scarcest_cell_has_exactly_one_kmer():
    """p = 4, k = 31, canonical, value q + 1 = 61: one hash per index, 16 in all, and one of their preimages is a canonical 31-mer"""
    found = [kc.make(4, 61, 31, True, skip=s) for s in range(3)]
    assert found[0] is not None and found[1] is None and found[2] is None


def test_make_is_deterministic_and_honours_index_skip_and_start():
    a = kc.make(12, 20, 31, True)
    assert a == kc.make(12, 20, 31, True)
    b = kc.make(12, 20, 31, True, skip=1)
    assert b is not None and b != a
    x, idx = kc.make(12, 20, 31, True, index=1234)
    assert idx == 1234 and kc.rule(opy.wang(x), 12) == (1234, 20)
    y, idy = kc.make(12, 20, 31, True, index=1234, skip=1)
    assert idy == 1234 and y != x and kc.rule(opy.wang(y), 12) == (1234, 20)
    z, idz = kc.make(12, 53, 32, False, start=4000)
    assert kc.rule(opy.wang(z), 12) == (idz, 53) and (idz >= 4000 or idz < 200)
    assert kc.make(12, 53, 31, True, index=7, budget=1) in (None, kc.make(12, 53, 31, True, index=7))
    # (value q + 1 with a given index is one candidate: most indices have no k-mer, and the maker says so)
    assert sum(kc.make(12, 53, 31, True, index=i) is None for i in range(64)) > 32


def test_text_and_reverse_complement_text():
    x = int("".join("%d" % c for c in [0, 1, 2, 3, 3, 0]), 4)
    assert kc.text(x, 6).tobytes() == b"ACGTTA"
    assert kc.rc_text(x, 6).tobytes() == b"TAACGT"
    assert kc.text(0, 31).tobytes() == b"A" * 31 and kc.rc_text(0, 32).tobytes() == b"T" * 32


@pytest.mark.parametrize("p", PS)
def test_both_oracles_sketch_the_bare_kmer_to_the_one_hot_row(p, oracle):
    """a genome of exactly k bases; for canonical cells the reverse-complement text gives the same row, for the others the
    row of the reverse complement's own hash"""
    for k, canon in KCS:
        made = [(v, kc.make(p, v, k, canon)) for v in kc.V(p)]
        texts, want = [], []
        for v, (x, idx) in made:
            texts += [kc.text(x, k), kc.rc_text(x, k)]
            want += [(idx, v), (idx, v) if canon else kc.rule(opy.wang(revcomp(x, k)), p)]
        seq, off = synth.concat_for_device(texts)
        rows = oracle.sketch_batch(seq, off, k, p, canon)
        for g, (t, (idx, v)) in enumerate(zip(texts, want)):
            hot = kc.one_hot(p, idx, v)
            assert np.array_equal(rows[g], hot), ("C oracle", p, k, canon, g)
            assert np.array_equal(opy.sketch(t.tobytes(), k, p, canon), hot), ("Python oracle", p, k, canon, g)


# ---- the value set bites: mistakes of the rule, restated.  Each returns (index, value) like kc.rule.
def _clz64(t):
    return 64 - (t & kc.M64).bit_length()


def no_guard_bit(h, p):
    return h >> (64 - p), _clz64(h << p) + 1


def guard_bit_at_p(h, p):
    return h >> (64 - p), _clz64((h << p) | (1 << p)) + 1


def high_word_only(h, p):
    """the value from the high word of t alone, a zero word giving 0"""
    thi = (((h << p) | (1 << (p - 1))) & kc.M64) >> 32
    return h >> (64 - p), (32 - thi.bit_length()) + 1 if thi else 0


def capped_at_32(h, p):
    idx, v = kc.rule(h, p)
    return idx, min(v, 32)


def low_word_plus_31(h, p):
    t = ((h << p) | (1 << (p - 1))) & kc.M64
    thi, tlo = t >> 32, t & 0xFFFFFFFF
    zh = 32 - thi.bit_length() if thi else 1 << 32  # (v_ffbh_u32 of 0 is -1: unsigned, the minimum never picks it)
    zl = 32 - tlo.bit_length()
    return h >> (64 - p), min(zh, zl + 31) + 1


def index_one_bit_low(h, p):
    return h >> (64 - p - 1), kc.rule(h, p)[1]


MUTANTS = [no_guard_bit, guard_bit_at_p, high_word_only, capped_at_32, low_word_plus_31, index_one_bit_low]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda f: f.__name__)
def test_every_mutant_of_the_rule_differs_on_a_made_kmer_at_every_p(mutant):
    for p in PS:
        hashes = [opy.wang(made[0]) for _, _, _, made in cells(p)]
        assert any(mutant(h, p) != kc.rule(h, p) for h in hashes), "%s survives V(%d)" % (mutant.__name__, p)


def test_the_mutants_are_mutants_of_this_rule():
    """on a hash of the bulk -- value 3, nothing near an edge -- every mutant but the index one IS the rule"""
    for p in PS:
        h = (5 << (64 - p)) | (1 << (64 - p - 3)) | 1
        assert kc.rule(h, p) == (5, 3)
        for m in MUTANTS[:-1]:
            assert m(h, p) == (5, 3), m.__name__
