"""The collections of tests/test_gpu_paths.py and the matrix they have to fill (tests/test_path_census.py): small families
of LEGAL register matrices (values <= 64 - p + 1) that take the compare path's data-dependent branches by construction
-- tools/path_census.py names the branches and says which a collection takes.  Host only: numpy and dashing_amd.synth."""
import os
import sys

import numpy as np

from dashing_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import path_census as pcs  # noqa: E402

# The instances under test, by precision (with the default list caps): what tools/path_census.py::instance must say.
INSTANCES = {
    8: {"CT": 2, "RK": 7, "tile_kernel": "free"},       # free-running k_pair_counts, wide records
    10: {"CT": 2, "RK": 7, "tile_kernel": "lockstep"},  # lockstep tile kernel, wide records
    14: {"CT": 2, "RK": 3, "tile_kernel": "lockstep"},  # narrow records
    15: {"CT": 2, "RK": 3, "tile_kernel": "lockstep"},  # the 16-bit counts at their limit (a bin can hold 2^15), two positions to a bucket
    16: {"CT": 4, "RK": 3, "tile_kernel": "lockstep"},  # uint32_t counts, four positions to a bucket
}

# Cells of the matrix instance x condition that no legal input reaches, each with its arithmetic.
IMPOSSIBLE = {
    (8, "join.group_entry_dropped"): "a bucket holds 1 << max(p - 14, 0) positions: one at p <= 14, so same_position() is not even evaluated",
    (10, "join.group_entry_dropped"): "a bucket holds 1 << max(p - 14, 0) positions: one at p <= 14",
    (14, "join.group_entry_dropped"): "a bucket holds 1 << max(p - 14, 0) positions: one at p <= 14",
}
# (Every other cell is possible at these five precisions: more than 48 tail bins needs a register >= 48 above a tile
# threshold <= 14, i.e. q + 1 = 64 - p + 1 >= 48, p <= 17; w0 >= 2 needs a threshold >= 31 <= q + 1; RK = 7 needs p <= 12
# and is part of the instance, not a condition; a bucket beyond 64 + RK entries needs 72 of a block's 128 columns to list
# one position on one side.)

POOL = 16  # shared positions of the planted families


def _pool(rng, p):
    """16 positions every sketch of a family draws from: 8 pairs of neighbours (4g, 4g + 1), which share a bucket of the
    position index wherever a bucket holds more than one position (p > 14)"""
    g = np.sort(rng.choice((1 << p) // 4, POOL // 2, replace=False)) * 4
    return np.concatenate((g, g + 1))


def empty(n, p, seed=0):
    """all registers 0: failed inputs, cleared slots"""
    return np.zeros((n, 1 << p), np.uint8)


def constant_outliers(n, p, seed, level=5):
    """every register `level`; per sketch three registers above it (values in [level + 1, q + 1]) and three below (values
    in [0, level - 1]), at six of the 16 shared positions: T = L = level in every sketch, both lists hold three entries"""
    rng = np.random.default_rng(seed)
    top = 64 - p + 1
    pool = _pool(rng, p)
    regs = np.full((n, 1 << p), level, np.uint8)
    for g in range(n):
        pos = rng.choice(pool, 6, replace=False)
        regs[g, pos[:3]] = rng.integers(level + 1, top + 1, 3)
        regs[g, pos[3:]] = rng.integers(0, level, 3)
    return regs


def constant_high(n, p, seed):
    """the same around the value 33: thresholds in the third 16-byte word of the tail histogram"""
    return constant_outliers(n, p, seed, level=33)


def planted_maxima(n, p, seed):
    """low cardinality (2^p / 2 elements: most registers 0 or 1) with six of twelve shared positions per sketch set to
    values in [20, q + 1]: a long upper tail far above the law's own, crowded upper buckets"""
    rng = np.random.default_rng(seed)
    top = 64 - p + 1
    pool = _pool(rng, p)[:12]
    regs = np.stack([synth.hll_registers(seed * 1000 + g, (1 << p) // 2, p) for g in range(n)])
    for g in range(n):
        regs[g, rng.choice(pool, 6, replace=False)] = rng.integers(20, top + 1, 6)
    return regs


def sparse(n, p, seed):
    """nearly empty sketches: registers 0 but for four of eight shared positions (values in [1, q + 1]); everything above
    the lowest bin fits the list, T = lo = 0"""
    rng = np.random.default_rng(seed)
    top = 64 - p + 1
    pool = _pool(rng, p)[:8]
    regs = np.zeros((n, 1 << p), np.uint8)
    for g in range(n):
        regs[g, rng.choice(pool, 4, replace=False)] = rng.integers(1, top + 1, 4)
    return regs


def near_duplicates(n, p, seed):
    """one base sketch of the register law, copy g differs from it in five registers: every copy lists the same positions"""
    from test_gpu_finalize_join import near_duplicates as nd

    return nd(n, p, seed)


def mixed(n, p, seed):
    """130 empty sketches, 130 of the constant family and 40 ordinary ones: the key order puts pure and mixed blocks side
    by side"""
    assert n == 300
    return np.concatenate((empty(130, p), constant_outliers(130, p, seed), synth.synthetic_sketches(40, p, seed=seed + 1)))


def mixed_high(n, p, seed):
    """100 empty sketches, 100 of the constant family around 33 and 57 ordinary ones: blocks whose values start at 0 meet
    thresholds of 33 -- tiles of more dense planes than one batch"""
    assert n == 257
    return np.concatenate((empty(100, p), constant_high(100, p, seed), synth.synthetic_sketches(57, p, seed=seed + 1)))


def identical_constant(n, p, seed):
    """n identical sketches of one value: every pair's histogram is one bin of 2^p"""
    return np.full((n, 1 << p), 9, np.uint8)


def two_valued_and_constant(n, p, seed):
    """identical two-valued sketches (7 and 9, half the registers each) beside identical constant ones (12): the tile's
    threshold is 12, so the planes above 9 count ALL 2^p registers of a two-valued pair -- C(v) = 2^p from the tile kernel"""
    regs = np.full((n, 1 << p), 12, np.uint8)
    half = (n + 1) // 2
    regs[:half] = 7
    regs[:half, ::2] = 9
    return regs


FAMILIES = {f.__name__: f for f in (empty, constant_outliers, constant_high, planted_maxima, sparse, near_duplicates, mixed, mixed_high,
                                    identical_constant, two_valued_and_constant)}

# What each family is chosen for: conditions that hold BY CONSTRUCTION at every precision and size it is used at and in
# both column orders (with the default list caps) -- asserted on the host before the device runs.
NAMED_FOR = {
    # T = hi = lo = L = 0 everywhere: nothing listed, pbase = T = 0
    "empty": {"sketch.nothing_listed", "tile.no_dense_plane", "collection.no_planes"},
    # three registers above 5 fit every cap (auto caps are >= 8), the 2^p - 6 fives do not: T = 5; three below: L = 5 = T > lo.
    # Every tile: Lp = T = 5 > vlo, x0 = 0 and some register >= 48 among 3n draws from [6, q + 1]; 24 columns of a block share
    # a row entry's position on its side, a fifth to a 44th of them its value
    "constant_outliers": {"sketch.L_at_T_above_lo", "tile.no_dense_plane", "tile.bins_below_dense", "tile.tail_bins_beyond_48",
                          "join.upper_equal_values", "join.lower_equal_values", "join.entry_for_lane_without_pair",
                          "join.bucket_beyond_record", "collection.no_planes"},
    # the same at T = L = 33: w0 = 34 >> 4 = 2
    "constant_high": {"sketch.L_at_T_above_lo", "tile.no_dense_plane", "tile.bins_below_dense", "tile.tail_words_cut",
                      "join.upper_equal_values", "join.lower_equal_values", "join.entry_for_lane_without_pair",
                      "join.bucket_beyond_record", "collection.no_planes"},
    # at half an element per register the law's own registers are mostly 0 and 1 and thin out geometrically: every T -- and so
    # every tile's -- stays far below 15 (x0 = 0) while 6n planted draws from [20, q + 1] reach 48; half of a block's columns
    # list each planted position
    "planted_maxima": {"tile.tail_bins_beyond_48", "join.bucket_beyond_record", "join.entry_for_lane_without_pair"},
    # four registers above 0 fit every cap: the first walk ends at lo = 0 = T, and 4n draws from [1, q + 1] reach 48
    "sparse": {"sketch.T_at_lo", "tile.no_dense_plane", "tile.tail_bins_beyond_48", "join.upper_equal_values",
               "join.entry_for_lane_without_pair", "join.bucket_beyond_record", "collection.no_planes"},
    # every copy lists the base's positions: ~128 entries to a bucket
    "near_duplicates": {"join.bucket_beyond_record", "join.bucket_beyond_wave_read", "join.queue_drained_early"},
    # blocks of empty sketches alone (no plane) beside blocks that hold ordinary ones (planes); an empty sketch (lo = L = 0)
    # in a block of constant ones pulls the block's Lp to 0 < their L = 5, and their T = 5 lies below the ordinary sketches'
    "mixed": {"collection.band_mixed_planes", "tile.no_dense_plane", "tile.row_lower_in_dense", "tile.row_upper_in_dense",
              "tile.column_entry_rejected"},
    # a block with an empty sketch has lo = L = 0: its tile with the block of T = 33 holds 33 planes
    "mixed_high": {"tile.planes_beyond_batch", "tile.tail_words_cut", "tile.row_lower_in_dense"},
    "identical_constant": {"sketch.nothing_listed", "tile.no_dense_plane", "collection.no_planes"},
    # (what this family is for is no named condition: counts_at_the_limit() below)
    "two_valued_and_constant": {"sketch.nothing_listed", "collection.band_mixed_planes"},
}


def counts_at_the_limit(case, census):
    """host assertion of the family two_valued_and_constant: its first block holds two-valued sketches (T = 9, L = lo = 7)
    and constant ones (T = L = 12), so its diagonal tile has Lp = 7, T = 12 and the five planes C(8) .. C(12); a pair of
    two-valued sketches has no register at 10 or above, so the tile kernel counts C(10) = C(11) = C(12) = 2^p for it and the
    bin 9 of its histogram column holds 2^p - 2^(p-1) after C(9) = 2^(p-1): at p = 15 the largest 16-bit counts there are"""
    assert case.family == "two_valued_and_constant"
    regs, m = case.regs(), 1 << case.p
    t = census.tiles[0]
    assert (t["bi"], t["bj"], t["Lp"], t["T"], t["planes"], t["vlo"], t["vhi"]) == (0, 0, 7, 12, 5, 7, 12), t
    cols = census.blocks[0]["cols"]
    two = [int(s) for s in cols if int(regs[s].max()) == 9]
    assert len(two) >= 2 and len(two) < len(cols)
    a, b = regs[two[0]], regs[two[1]]
    assert int((np.maximum(a, b) < 10).sum()) == m and int((np.maximum(a, b) < 9).sum()) == m // 2


class Case:
    """one collection of the GPU file: family x p x n (its registers are built once and never changed)"""

    def __init__(self, family, p, n):
        self.family, self.p, self.n = family, p, n
        self.id = "%s-p%d-n%d" % (family, p, n)
        self._regs = None
        self._census = {}

    def regs(self):
        if self._regs is None:
            r = np.ascontiguousarray(FAMILIES[self.family](self.n, self.p, 1000 * self.p + self.n), np.uint8)
            assert r.shape == (self.n, 1 << self.p) and int(r.max()) <= 64 - self.p + 1
            r.setflags(write=False)
            self._regs = r
        return self._regs

    def census(self, emax=None, elow=None, sort=True):
        key = (emax, elow, bool(sort))
        if key not in self._census:
            self._census[key] = pcs.census(self.regs(), self.p, emax, elow, sort)
        return self._census[key]


# the list caps the GPU file runs every collection under (None: the defaults, plan::auto_list_cap)
CAPS = ((None, None), (0, 0), (3, 2), (255, 255))


def cases():
    out = []
    for p in INSTANCES:
        for fam in ("empty", "constant_outliers", "constant_high", "planted_maxima", "sparse", "near_duplicates"):
            out.append(Case(fam, p, 131))
        for fam in ("empty", "constant_outliers", "constant_high", "planted_maxima", "sparse", "near_duplicates"):
            out.append(Case(fam, p, 257))  # three blocks: an off-diagonal tile whose 128 lanes all own a pair
        out.append(Case("mixed", p, 300))
        out.append(Case("mixed_high", p, 257))
    out.append(Case("identical_constant", 15, 131))
    out.append(Case("two_valued_and_constant", 15, 131))
    return out


CASES = cases()


class Run:
    """one (collection, list caps, column order) the GPU file sends through the device"""

    def __init__(self, case, emax, elow, sort):
        self.case, self.p, self.emax, self.elow, self.sort = case, case.p, emax, elow, sort

    def regs(self):
        return self.case.regs()

    def census(self):
        return self.case.census(self.emax, self.elow, self.sort)


def census_runs():
    """every run of the GPU file: the default caps in both column orders (options sort = 1 and 0), the other caps in
    the default (key) order"""
    out = []
    for c in CASES:
        out.append(Run(c, None, None, True))
        out.append(Run(c, None, None, False))
        for emax, elow in CAPS[1:]:
            out.append(Run(c, emax, elow, True))
    return out
