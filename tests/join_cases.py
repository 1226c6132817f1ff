"""Collections on which every decision of k_finalize's tail join moves the float32 result (numpy only, no device).

A register in bin v weighs 2^-v, so on sketches of the register law a count that a wrong join decision moves between a
tail bin and the tile's boundary bin changes the estimate by less than the suite's tolerance from about p = 14 upwards
("Which inputs make the join observable").  The builders here make every such count heavy:

  family S  all registers 0, except at most emax(p) planted registers with values in 1 .. q + 1: T = L = 0, no dense
            plane, the whole sketch is its upper list and c[0] = m - |union of the listed positions|: one decision is one
            register more or less in a union of a few dozen.
  family C  registers alternate b and b + 1 (L = b, T = b + 1: one dense plane between the two tails, the seam c[T] /
            C(Lp)); at most emax planted registers above b + 1 and at most elow below b, with values 0 .. b - deep: a lower
            match weighs at least 2^-(b - deep) against the base's 2^-b.

All sketches of a collection have the same thresholds (asserted with tools/join_model.py by tests/test_join_cases.py),
so every tile's boundary bins are T and Lp = L whatever the column order or block.  Planted per tail:
  a core     positions that all sketches (crowded variants and small n) or all of a cluster (n >= 129, plain variants)
             list, with values that are smaller, equal and larger between two sketches; 1 and q + 1 above, 0 below; the
             last position of the sketch (2^p - 1) is one of them;
  near misses  positions of one position group (x >> sh equal, sh = max(p - 14, 0); the neighbouring position where
             sh = 0) with other low bits, chosen per sketch from a small pool -- two of them per group at p >= 20;
  private    positions.
Crowded variants: the fullest bucket of a 128-column block holds more than 64 + record_inline entries -- at n >= 129
because every column lists the core, at p = 22 and 24 (small n) because every sketch lists many positions of one group.

The error model (kernels_compare.hip, header pieces (2) and (3), and finalize_block: the tail bins start as the sum of the
two tail histograms, a match takes the smaller value out again and counts into corr, c[T] = m - |union above T| - C(T); the
bins below Lp hold the matches at the larger value, their number C(Lp) is taken from c[Lp]).  With H = bincount(max(a, b)):

  missed upper match at x                H[min(a_x, b_x)] += 1,  H[T] -= 1
  false upper match of a near miss x, x' H[min(a_x, b_x')] -= 1, H[T] += 1
  missed lower match at x                H[max(a_x, b_x)] -= 1,  H[L] += 1
  false lower match of a near miss x, x' H[max(a_x, b_x')] += 1, H[L] -= 1

A false match may name a bin that is empty (perturbed()).

Tails that cannot be designated: C upper from p = 17.  One upper count moved between a bin >= b + 2 and bin b + 1 changes
the harmonic sum by at least 2^-(b+2) of about 0.75 * 2^p * 2^-b, and JI (near 1 between two sketches of the same base:
d JI ~ 2 d us / us) by about 2 / (3 * 2^p): measured with these builders 4.0e-5 at p = 14 and 2.0e-5 at p = 15, which clear
the bar of 16 tolerances = 1.6e-5, then 1.0e-5 at p = 16 and 4.8e-6 at p = 17, which do not (the three estimators within
5 % of each other).  No choice of b or of the planted values changes that factor; a smaller JI does, since the relative
change grows like (ca + cb) / (us * JI).  So at p = 16 half the sketches have the base the other way round (b + 1 where
the others have b): the union of two such sketches is b + 1 everywhere, JI is near 1/3, one count is worth about 2 / 2^p
= 3.0e-5 (measured), and the pairs out of phase are the designated ones.  At p = 17 that gives 1.5e-5, just under the
bar.  The planted upper registers of C are still there and joined at every p; only the sensitivity claim is not made
for them from p = 17."""
import collections
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import join_model as jm  # noqa: E402

TILE = 128
MARGIN = 16  # a decision must move the reference by this many tolerances

# (p, n) of the device tests: the smallest shapes at which the join can still go wrong
SHAPES = [(p, n) for p in (9, 10, 12, 13, 14, 15, 16) for n in (129, 260)] + [(17, 129), (18, 129), (19, 129), (20, 129), (22, 20), (24, 6)]
# family C: base value b and the depth of the lower plants (values 0 .. b - deep) per p
C_PARAMS = {9: (5, 2), 10: (5, 2), 12: (5, 2), 13: (5, 2), 14: (5, 2), 15: (8, 3), 16: (8, 3), 17: (12, 3), 18: (12, 5), 19: (12, 6),
            20: (12, 8), 22: (12, 9), 24: (12, 10)}
C_UPPER_MAX_P = 16  # family C's upper tail is designated up to here (module docstring)
C_PHASED_P = 16     # ... at this p only between sketches whose bases are out of phase

Decision = collections.namedtuple("Decision", "kind tail x x2 va vb")  # kind: "missed" | "false"; tail: "upper" | "lower"


def shift(p):
    return max(p - 14, 0)


def caps(p):
    return jm.auto_list_cap(p, True), jm.auto_list_cap(p, False)


class Collection:
    """regs [n, 2^p] uint8 (read-only), the family's parameters and the designated tails"""

    def __init__(self, name, family, p, regs, crowded, tails, cluster, b=None, deep=None):
        self.name, self.family, self.p, self.regs, self.crowded, self.tails = name, family, p, regs, crowded, tuple(tails)
        self.n = regs.shape[0]
        self.cluster = cluster  # cluster id per sketch (the core is shared inside a cluster)
        self.b, self.deep = b, deep
        self.phase = np.zeros(self.n, np.int64)  # family C at C_PHASED_P: which way round the base alternates
        self.emax, self.elow = caps(p)
        regs.setflags(write=False)
        self._thr = None
        self._listed = {}

    def listed(self, s, tail):
        """positions sketch s lists in a tail of a tile with the collection's thresholds (found once per sketch)"""
        if (s, tail) not in self._listed:
            T, L = self.uniform()
            self._listed[(s, tail)] = np.flatnonzero(self.regs[s] > T if tail == "upper" else self.regs[s] < L)
        return self._listed[(s, tail)]

    def thresholds(self):
        """lo, hi, T, L, listed above, listed below: per sketch, by the model of k_selfhist_card"""
        if self._thr is None:
            self._thr = jm.list_thresholds(self.regs, self.emax, self.elow)
        return self._thr

    def uniform(self):
        """(T, L) of every sketch; asserts that they are equal over the collection"""
        _, _, T, L, _, _ = self.thresholds()
        assert (T == T[0]).all() and (L == L[0]).all(), (self.name, np.unique(T), np.unique(L))
        return int(T[0]), int(L[0])


# ---------------------------------------------------------------- planting
class _Units:
    """The position range in units of one position group (at least 4 positions, so that at sh = 0 the planted items are
    no neighbours of each other): items take whole units alternately from the top and from the bottom, private registers
    go to the free units."""

    def __init__(self, p, nitems):
        self.unit = max(4, 1 << shift(p))
        self.U = (1 << p) // self.unit
        assert nitems + 2 <= self.U, (p, nitems)
        step = max(1, self.U // (nitems + 2))
        self.taken = 0
        self.units = [self.U - 1 - (t // 2) * step if t % 2 == 0 else (t // 2) * step for t in range(nitems)]
        assert len(set(self.units)) == nitems
        self.free = np.setdiff1d(np.arange(self.U), np.array(self.units))

    def take(self):
        u = self.units[self.taken]
        self.taken += 1
        return u * self.unit

    def private(self, rng, count):
        u = self.free[rng.choice(len(self.free), count, replace=False)]
        return u * self.unit + rng.integers(0, self.unit, count)


def _pool(p, size):
    """low-bit offsets inside a position group for near misses: the neighbour at sh = 0, else the group's ends and middle"""
    G = 1 << shift(p)
    if G == 1:
        return [0, 1]
    out = []
    for o in (G - 1, 0, G // 2, G // 2 - 1, G // 4, 3 * G // 4):
        if o not in out and 0 <= o < G:
            out.append(o)
    return out[:size]


def _plan(p, cap, n, crowded):
    """how many core items, near-miss groups and private registers a tail gets, and the crowded group's load"""
    small = cap < 24
    ncore, nnm, npriv = (8, 6, 2) if small else (12, 8, 4)
    per_nm = 2 if p >= 20 else 1
    ncrowd = 0
    if crowded and n < TILE:  # few sketches: the bucket fills with many positions of one group, listed by every sketch
        ncrowd = -(-(64 + 7 + 1) // n) + 1  # (beyond one wave-wide read and the widest record, whatever the order)
        assert 2 * ncrowd <= (1 << shift(p)), "the group is too small to crowd"
    assert ncore + nnm * per_nm + npriv + ncrowd <= cap, (p, cap)
    return ncore, nnm, per_nm, npriv, ncrowd


def _nclusters(n, crowded):
    return 1 if crowded or n <= TILE else 4


def _core_choice(rng, n, k, nvals):
    """which of an item's nvals values a sketch gets.  Items 1 .. 2 * nbits follow a bit of the sketch number and its
    complement, so that any two sketches meet smaller, larger and (item 0) equal values; the others are random"""
    nbits = max(1, int(n - 1).bit_length())
    s = np.arange(n)
    if 1 <= k <= 2 * nbits and n <= 32:
        bit = (s >> ((k - 1) // 2)) & 1
        return np.minimum(bit if k % 2 else 1 - bit, nvals - 1)
    return rng.integers(0, nvals, n)


def _plant_tail(regs, rng, p, units, cl, ncl, plan, core_values, free_values):
    """plants one tail into regs: core items per cluster, near-miss groups, the crowded group, private registers"""
    n = regs.shape[0]
    ncore, nnm, per_nm, npriv, ncrowd = plan
    G = 1 << shift(p)
    s = np.arange(n)
    first = True
    for c in range(ncl):
        for k in range(ncore):
            base = units.take()
            # the core's first item of the first cluster is the sketch's last position when it got the top unit
            off = units.unit - 1 if first else (k % 2 if G == 1 else (G - 1, 0, G // 2)[k % 3] % G)
            first = False
            vals = np.asarray(core_values(k))
            v = vals[_core_choice(rng, n, k, len(vals))]
            rows = s[cl == c]
            regs[rows, base + off] = v[rows]
    pool = _pool(p, 4 if per_nm == 2 else 3)
    for k in range(nnm):
        base = units.take()
        for r in range(n):
            offs = rng.choice(len(pool), per_nm, replace=False)
            for o in offs:
                regs[r, base + pool[o]] = free_values(rng)
    if ncrowd:
        base = units.take()
        for r in range(n):
            offs = rng.choice(2 * ncrowd, ncrowd, replace=False)
            for o in offs:
                regs[r, base + (G - 1 - o if o % 2 else o)] = free_values(rng)
    for r in range(n):
        for x in units.private(rng, npriv):
            regs[r, x] = free_values(rng)


def _nitems(plan, ncl):
    ncore, nnm, _, _, ncrowd = plan
    return ncl * ncore + nnm + (1 if ncrowd else 0)


def _upper_values(vmin, q):
    def core(k):
        if k == 0:
            return [q + 1]
        if k == 1:
            return [vmin, vmin + 1, q + 1]
        return [vmin + k % 5, vmin + k % 5 + 1, vmin + k % 5 + 3]

    return core, lambda rng: vmin + int(rng.integers(0, 7))


def _lower_values(vmax):
    def core(k):
        if k == 0:
            return [0]
        return sorted({k % (vmax + 1), (k + 1) % (vmax + 1), (k + 3) % (vmax + 1)})

    return core, lambda rng: int(rng.integers(0, vmax + 1))


def build_S(n, p, crowded=False, seed=0):
    """family S: the whole sketch is its upper list"""
    rng = np.random.default_rng(0x5000 + 100 * p + n + (7 if crowded else 0) + seed)
    emax, _ = caps(p)
    ncl = _nclusters(n, crowded)
    plan = _plan(p, emax, n, crowded)
    units = _Units(p, _nitems(plan, ncl))
    regs = np.zeros((n, 1 << p), np.uint8)
    cl = np.arange(n) % ncl
    core, free = _upper_values(1, 64 - p)
    _plant_tail(regs, rng, p, units, cl, ncl, plan, core, free)
    return Collection("S%s-p%d-n%d" % ("x" if crowded else "", p, n), "S", p, regs, crowded, ("upper",), cl)


def build_C(n, p, crowded=False, seed=0):
    """family C: a constant base with both tails and one dense plane between them"""
    b, deep = C_PARAMS[p]
    rng = np.random.default_rng(0xC000 + 100 * p + n + (7 if crowded else 0) + seed)
    emax, elow = caps(p)
    ncl = _nclusters(n, crowded)
    plan_u, plan_l = _plan(p, emax, n, crowded), _plan(p, elow, n, crowded)
    units = _Units(p, _nitems(plan_u, ncl) + _nitems(plan_l, ncl))
    regs = np.empty((n, 1 << p), np.uint8)
    # which positions hold b and which b + 1: the same in every sketch, except at C_PHASED_P, where half the sketches
    # have them the other way round (the union of two such sketches is b + 1 everywhere: JI near 1/3)
    phase = (np.arange(n) >> 2) & 1 if p == C_PHASED_P else np.zeros(n, np.int64)
    for ph in (0, 1):
        regs[phase == ph] = (b + ((np.arange(1 << p) + ph) & 1)).astype(np.uint8)
    cl = np.arange(n) % ncl
    core, free = _upper_values(b + 2, 64 - p)
    _plant_tail(regs, rng, p, units, cl, ncl, plan_u, core, free)
    core, free = _lower_values(b - deep)
    _plant_tail(regs, rng, p, units, cl, ncl, plan_l, core, free)
    tails = ("upper", "lower") if p <= C_UPPER_MAX_P else ("lower",)
    coll = Collection("C%s-p%d-n%d" % ("x" if crowded else "", p, n), "C", p, regs, crowded, tails, cl, b, deep)
    coll.phase = phase
    return coll


def build_mixed(n, p):
    """rows of S, of C and of the register law, interleaved: no uniform thresholds and no sensitivity claim -- tiles whose
    blocks disagree on T and L, where entries at or below the tile's T are not looked up"""
    from dashing_amd import synth

    parts = (build_S(n, p, True).regs, build_C(n, p, True).regs, synth.related_sketches(n, p, seed=0xA11 + p)[0])
    regs = np.empty((n, 1 << p), np.uint8)
    for k in range(3):
        regs[k::3] = parts[k][k::3]
    return Collection("M-p%d-n%d" % (p, n), "M", p, regs, True, (), np.zeros(n, np.int64))


_BUILDERS = {"S": lambda n, p: build_S(n, p), "Sx": lambda n, p: build_S(n, p, True), "C": lambda n, p: build_C(n, p),
             "Cx": lambda n, p: build_C(n, p, True), "M": build_mixed}
MIXED = [(14, 260), (20, 129)]
KEYS = [(v, p, n) for (p, n) in SHAPES for v in ("S", "Sx", "C", "Cx")] + [("M", p, n) for (p, n) in MIXED]


def build(key):
    v, p, n = key
    return _BUILDERS[v](n, p)


def key_id(key):
    return "%s-p%d-n%d" % key


# ---------------------------------------------------------------- the join's decisions and the error model
def decisions(regs, i, j, p, T, L, listed=None):
    """every decision the join takes for the pair (i, j) in a tile with the thresholds T and Lp = L: the matches (a
    position both sketches list in the same tail -- the wrong decision is to miss it) and the near misses (two listed
    positions of one position group -- the neighbouring position at sh = 0 --; the wrong decision is to match them).
    listed(s, tail): the positions a sketch lists, where the caller has them already"""
    sh = shift(p)
    a, b = regs[i], regs[j]
    out = []
    for tail in ("upper", "lower"):
        if listed is not None:
            xa, xb = listed(i, tail), listed(j, tail)
        else:
            xa = np.flatnonzero(a > T if tail == "upper" else a < L)
            xb = np.flatnonzero(b > T if tail == "upper" else b < L)
        for x in np.intersect1d(xa, xb):
            out.append(Decision("missed", tail, int(x), int(x), int(a[x]), int(b[x])))
        if sh:
            near = ((xa[:, None] >> sh) == (xb[None, :] >> sh)) & (xa[:, None] != xb[None, :])
        else:
            near = np.abs(xa[:, None] - xb[None, :]) == 1
        for ka, kb in zip(*np.nonzero(near)):
            out.append(Decision("false", tail, int(xa[ka]), int(xb[kb]), int(a[xa[ka]]), int(b[xb[kb]])))
    return out


def perturbed(H, d, T, L, p):
    """the histogram a wrong decision leaves (the table of the module docstring).  A false match can take a count out of
    an empty bin (one sketch lists both positions of the near miss, the larger value at x'): the device's counter, 16 bits
    wide up to p = 15 and 32 bits above, wraps there, and so does the bin here"""
    H = np.asarray(H, np.int64).copy()
    wrap = 1 << (16 if p <= 15 else 32)
    if d.tail == "upper":
        sign = 1 if d.kind == "missed" else -1
        H[min(d.va, d.vb)] += sign
        H[T] -= sign
    else:
        sign = 1 if d.kind == "missed" else -1
        H[max(d.va, d.vb)] -= sign
        H[L] += sign
    return np.where(H < 0, H + wrap, H)


def reference(oracle, H, ca, cb, p, estim, result_type=1, k=31):
    """the float32 the device owes for a pair whose union histogram is H"""
    return np.float32(oracle.result(oracle.jaccard_from(ca, cb, oracle.estimate(np.asarray(H, np.uint32), p, estim)), result_type, k))


def union_hist(regs, i, j):
    return np.bincount(np.maximum(regs[i], regs[j]), minlength=64).astype(np.int64)


def pair_facts(coll, i, j):
    """matches, near misses and value orders per tail of a pair"""
    T, L = coll.uniform()
    ds = decisions(coll.regs, i, j, coll.p, T, L, coll.listed)
    facts = {}
    for tail in ("upper", "lower"):
        m = [d for d in ds if d.tail == tail and d.kind == "missed"]
        facts[tail] = {"matches": len(m), "near": sum(1 for d in ds if d.tail == tail and d.kind == "false"),
                       "orders": {(d.va > d.vb) - (d.va < d.vb) for d in m}}
    facts["in phase"] = bool(coll.phase[i] == coll.phase[j])
    return ds, facts


def structurally_fit(coll, facts):
    """>= 8 matches of every value order and >= 4 near misses per designated tail; where the bases of a collection differ
    in phase (family C at C_PHASED_P), only pairs out of phase: their JI is small enough for the upper tail to show"""
    if coll.phase.any() and facts["in phase"]:
        return False
    return all(facts[t]["matches"] >= 8 and facts[t]["near"] >= 4 and facts[t]["orders"] == {-1, 0, 1} for t in coll.tails)


def blocks(coll):
    """block of every sketch in the key order of the columns (plan::sort_rows_by_key), and the number of blocks"""
    lo, hi, T, L, _, _ = coll.thresholds()
    rank = np.empty(coll.n, np.int64)
    rank[jm.key_order(hi, T, L)] = np.arange(coll.n)
    return rank // TILE, (coll.n + TILE - 1) // TILE


def designated_pairs(coll, want=64):
    """The pairs the sensitivity claim is made for: all pairs where there are at most `want`, else at least `want` pairs
    that meet the structural conditions (>= 8 matches and >= 4 near misses per designated tail, every value order), taken
    in turn from a diagonal tile, an off-diagonal tile and the ragged last block.  Returns [(i, j, kind)], i < j."""
    n = coll.n
    if n * (n - 1) // 2 <= want:
        return [(i, j, "all") for i in range(n) for j in range(i + 1, n)]
    blk, nblk = blocks(coll)
    cand = {"diagonal": [], "off-diagonal": [], "ragged": []}
    for i in range(n):
        for j in range(i + 1, n):
            if coll.cluster[i] != coll.cluster[j]:
                continue
            bi, bj = sorted((int(blk[i]), int(blk[j])))
            if nblk > 1 and bj == nblk - 1 and n % TILE:
                cand["ragged"].append((i, j))
            elif bi == bj:
                cand["diagonal"].append((i, j))
            else:
                cand["off-diagonal"].append((i, j))
    cand = {k: v for k, v in cand.items() if v}  # (n = 129: the only off-diagonal tile is the ragged one)
    rng = np.random.default_rng(n * 131 + coll.p)

    def fit(kind, prs):
        for k in rng.permutation(len(prs)):
            i, j = prs[k]
            if structurally_fit(coll, pair_facts(coll, i, j)[1]):
                yield (i, j, kind)

    out = []
    source = [fit(kind, prs) for kind, prs in cand.items()]
    share = -(-want // len(source))
    for it in source:  # an equal share of every kind, then whatever the kinds still have
        out += [pr for _, pr in zip(range(share), it)]
    for it in source:
        out += [pr for _, pr in zip(range(max(want - len(out), 0)), it)]
    return out


def fullest_bucket(coll):
    """entries of the fullest bucket of a 128-column block, in the key order and in the identity order of the columns
    (the smaller of the two), and what a bucket's record and one wave-wide read hold together"""
    lo, hi, T, L, _, _ = coll.thresholds()
    E = max(1, coll.emax + coll.elow)
    full = None
    for order in (jm.key_order(hi, T, L), np.arange(coll.n)):
        cur = max(int(jm.ColumnBlock(coll.regs, order[b : b + TILE], T, L, coll.p).count.max()) for b in range(0, coll.n, TILE))
        full = cur if full is None else min(full, cur)
    return full, 64 + jm.record_inline(coll.p, E)


def margin(got, ref, rtol):
    """|got - ref| in units of the suite's tolerance (test_gpu_compare.close: rtol * max(|ref|, 1e-9))"""
    return abs(float(got) - float(ref)) / (rtol * max(abs(float(ref)), 1e-9)) if math.isfinite(float(got)) else math.inf
