"""CPU: the planner's output pinned value for value.  tests/test_plan.py and its neighbours hold a plan to its CONTRACT
(coverage, order, caps); this file holds it to its IDENTITY: dshh_plan_digest (csrc/host/plan_capi.cpp) builds layout and
plan as the contract checks do and returns one 64-bit FNV-1a digest per section of the Layout, the PairPlan, the two device
lists and band_item_count, plus a word that says which branches of the planner the case reached.  The digests are compared
with tests/golden/plan_digest.json, which was written from the planner as it stood BEFORE build_tiles was cut into steps
(the hook alone applied to that commit) and is never regenerated from the code under test: a planner change that is meant
to alter a plan replaces the entries it alters and says so.

The inputs come from the integer generator below, so they do not depend on a numpy version.  Writing mode (for a planner
whose output is the reference): DSH_PLAN_DIGEST_WRITE=1 python -m pytest tests/test_plan_digest.py

One case is larger than the rest (n = 12 000, 4 465 tiles): a part only cuts a band from 2 048 tiles on, which no smaller
collection holds; the hook checks no pairs, so the case still takes milliseconds."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_digest.json")
FEATURES = ["bands>1", "band cut by a large part", "tail cut", "overflow fragments", "band at small_round_items", "parts>1",
            "rowsorted", "two-run rowsorted", "extra segments", "rectangle", "sorted_rows", "identity layout", "W<kc", "nsplit>0",
            "not lockstep", "two-plane items", "sided items", "transposed items", "table-only slabs", "routed from the bottom",
            "cum_bytes=4"]


class Gen:
    """a 64-bit linear congruential generator (Knuth's MMIX constants), the top 31 bits of every state"""

    def __init__(self, seed):
        self.x = (seed * 0x9E3779B97F4A7C15 + 1) & 0xFFFFFFFFFFFFFFFF

    def below(self, k):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.x >> 33) % k


def make_inputs(seed, n, p, spread, cap):
    """per-sketch keys as k_selfhist_card writes them (lo <= L <= T <= hi <= 64 - p + 1), counts g0 | g1 << 16 and thresholds
    vU | vA << 8 that agree with the counts at `cap` (tools/cabi/sparse_sided_walk.cpp: vU follows from g0 / g1, vA below it)"""
    g = Gen(seed)
    q1 = 64 - p + 1
    keys, cnt, thr = [], [], []
    for _ in range(n):
        lo = g.below(max(1, q1 - spread))
        L = min(lo + g.below(spread + 1), q1)
        T = min(L + g.below(spread + 1), q1)
        hi = min(T + g.below(spread + 1), q1)
        keys.append(hi << 18 | T << 12 | L << 6 | lo)
        g0 = g.below(1500)
        g1 = g0 + g.below(900)
        cnt.append(g0 | g1 << 16)
        if g1 <= cap:
            vU = max(T - 1, 0)
            vU -= min(vU, g.below(3))
        elif g0 <= cap:
            vU = T
        else:
            vU = T + 1 + g.below(3)
        vA = min(max(vU - 1, 0), L + g.below(4))
        thr.append(vU | vA << 8)
    return keys, cnt, thr


DEFAULTS = dict(n=1500, p=12, spread=6, mode=0, sorted=1, rb=0, re=None, cb=0, ce=0, nparts=1, want_parts=0, budget=8 << 30, lockstep=1,
                nsplit=0, chunks=64, ri=0, sp=0, sd=0, cap=1280, plan_cap=None, counts=True, thr=True, extra=())


def _cases():
    c = {}
    # layouts and tile lists: sorted and identity, row ranges, sizes around a tile (tests/test_plan.py:54, :67)
    c["tri_sorted"] = dict()
    c["tri_identity"] = dict(sorted=0)
    c["one_sketch"] = dict(n=1)
    c["n129_p9"] = dict(n=129, p=9)
    c["rows_sorted_p10"] = dict(n=1700, p=10, rb=300, re=1100)
    c["rows_identity"] = dict(n=1700, sorted=0, rb=300, re=1100)
    c["rows_empty"] = dict(n=1000, rb=1000, re=1000, want_parts=1, nparts=2)
    # parts, row-sorted parts, a long row-sorted range in two runs (:77, :102, :354)
    c["parts8_short_range"] = dict(n=2600, rb=640, re=1280, nparts=8, want_parts=1)
    c["rowsorted8"] = dict(n=2600, spread=10, mode=3, rb=0, re=640, nparts=8)
    c["rowsorted_two_runs"] = dict(n=3000, mode=3, rb=1536, re=3000, nparts=8)
    # bands under the scratch budget, with parts across them, one tile per band, a large part (:119)
    c["budget_4MiB"] = dict(budget=4 << 20)
    c["budget_1KiB"] = dict(n=700, budget=1 << 10)
    c["budget_parts4"] = dict(budget=2 << 20, nparts=4, want_parts=1)
    c["large_part"] = dict(n=12000, p=10, nparts=2, want_parts=1)
    # rectangles and sorted rows (:138)
    c["rect"] = dict(n=900, mode=1, rb=100, re=300, cb=0, ce=900)
    c["rect_empty"] = dict(n=900, mode=1, rb=5, re=5, cb=0, ce=10)
    c["sorted_rows"] = dict(n=900, mode=2, rb=256, re=900)
    # item options (:149)
    for name, kw in (("nsplit1", dict(nsplit=1)), ("nsplit5", dict(nsplit=5)), ("chunks1", dict(chunks=1)), ("chunks16", dict(chunks=16)),
                     ("chunks100000", dict(chunks=100000)), ("no_lockstep", dict(lockstep=0)), ("p8", dict(p=8)), ("p4", dict(p=4)),
                     ("p17", dict(p=17))):
        c["items_" + name] = dict(dict(n=1000, p=14, spread=12), **kw)
    # row sets: extra segments, as the destination (one part) and as a source (row-sorted parts) (:275)
    c["extra_destination"] = dict(n=2000, rb=256, re=768, extra=(1536, 1792, 1920, 2000), want_parts=1)
    c["extra_rowsorted"] = dict(n=2000, mode=3, rb=256, re=768, extra=(1536, 1792, 1920, 2000), nparts=4)
    # tail bands, alone and estimated with either sparse route (:315, :335)
    c["tail_bands"] = dict(n=3000, p=14, spread=8, mode=3, rb=0, re=1280, nparts=8)
    c["tail_bands_second"] = dict(n=3000, p=14, spread=3, mode=3, rb=0, re=2816, nparts=8)
    c["tail_bands_sided"] = dict(n=3000, p=14, spread=8, mode=3, rb=0, re=1280, nparts=8, ri=768, sp=-1, sd=-1)
    c["tail_bands_two_plane"] = dict(n=3000, p=14, spread=8, mode=3, rb=0, re=1280, nparts=8, ri=768, sp=-1, sd=0, cap=2040)
    # overflow fragments and the small round (:409)
    for n in (1500, 1800, 2100, 2400):
        c["overflow_n%d" % n] = dict(n=n, p=14)
    c["small_round"] = dict(n=1000, p=14, ri=768)
    # the two sparse routes: every setting of the two options at p = 14, then other precisions, a stale cap, missing inputs,
    # a range in parts under a small budget (bands on both sides of the automatic gate)
    for sp in (-1, 0, 1, 2):
        for sd in (-1, 0, 1):
            c["sparse_p14_sp%d_sd%d" % (sp, sd)] = dict(n=2000, p=14, spread=4, ri=768, sp=sp, sd=sd, cap=2040)
    c["sparse_p16_auto"] = dict(n=1200, p=16, spread=4, ri=768, sp=-1, sd=-1)
    c["sparse_p16_two_plane"] = dict(n=1200, p=16, spread=4, ri=768, sp=2, sd=0, cap=2040)
    c["sparse_p16_sided_only"] = dict(n=1200, p=16, spread=4, ri=512, sp=0, sd=1)
    c["sparse_p13_auto"] = dict(n=2500, p=13, spread=5, ri=768, sp=-1, sd=-1)
    c["sparse_p12_forced"] = dict(n=1500, p=12, spread=4, ri=768, sp=1, sd=1, cap=2040)
    c["sparse_p12_auto"] = dict(n=1500, p=12, spread=4, ri=768, sp=-1, sd=-1)
    c["sparse_p10_forced"] = dict(n=1500, p=10, spread=4, ri=512, sp=2, sd=-1, cap=2040)
    c["sparse_p9_forced"] = dict(n=800, p=9, spread=4, ri=512, sp=2, sd=1, cap=2040)
    c["sparse_stale_cap"] = dict(n=2000, p=14, spread=4, ri=768, sp=-1, sd=-1, cap=1280, plan_cap=2040)
    c["sparse_cap_1280"] = dict(n=2000, p=14, spread=4, ri=768, sp=-1, sd=-1)
    c["sparse_no_thresholds"] = dict(n=2000, p=14, spread=4, ri=768, sp=-1, sd=1, thr=False, cap=2040)
    c["sparse_no_counts"] = dict(n=2000, p=14, spread=4, ri=768, sp=2, sd=1, counts=False, cap=2040)
    c["sparse_parts_small_bands"] = dict(n=2500, p=14, spread=4, ri=768, sp=-1, sd=-1, rb=384, re=2200, nparts=3, want_parts=1, budget=48 << 20)
    c["sparse_identity"] = dict(n=1500, p=14, spread=4, sorted=0, ri=768, sp=2, sd=1)
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    u64, i32, u32, vp = C.c_uint64, C.c_int, C.c_uint32, C.c_void_p
    lib.dshh_plan_digest_names.restype = C.c_char_p
    lib.dshh_plan_digest.argtypes = [u64, vp, vp, vp, u32, i32, i32, u64, u64, u64, u64, u32, i32, i32, u64, i32, i32, i32, u32, i32, i32, u32,
                                     vp, u32, vp, u32, C.POINTER(u64), C.c_char_p, C.c_size_t]
    return lib


def digest(host, index, kw):
    a = dict(DEFAULTS, **kw)
    n = a["n"]
    keys, cnt, thr = make_inputs(1000 + index, n, a["p"], a["spread"], a["cap"])
    arr = lambda v: (C.c_uint32 * n)(*v)
    keys_a, cnt_a, thr_a = arr(keys), arr(cnt) if a["counts"] else None, arr(thr) if a["thr"] else None
    extra = (C.c_uint64 * len(a["extra"]))(*a["extra"])
    names = host.dshh_plan_digest_names().decode().split(",")
    out = (C.c_uint64 * len(names))()
    feat = C.c_uint64(0)
    err = C.create_string_buffer(512)
    rc = host.dshh_plan_digest(n, keys_a, cnt_a, thr_a, a["cap"], a["mode"], a["sorted"], a["rb"], n if a["re"] is None else a["re"], a["cb"],
                               a["ce"], a["nparts"], a["want_parts"], a["p"], a["budget"], a["lockstep"], a["nsplit"], a["chunks"], a["ri"],
                               a["sp"], a["sd"], a["cap"] if a["plan_cap"] is None else a["plan_cap"], extra, len(a["extra"]), out, len(names),
                               C.byref(feat), err, 512)
    assert rc == len(names), err.value.decode()
    return {"features": feat.value, "digests": {nm: "%016x" % out[i] for i, nm in enumerate(names)}}


@pytest.fixture(scope="module")
def results(host):
    res = {name: digest(host, i, kw) for i, (name, kw) in enumerate(CASES.items())}
    if os.environ.get("DSH_PLAN_DIGEST_WRITE") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(res, f, indent=0, sort_keys=True)
            f.write("\n")
    return res


def test_every_plan_is_the_golden_plan(results):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(results)
    wrong = []
    for name, r in results.items():
        g = golden[name]
        wrong += ["%s: %s" % (name, sec) for sec, d in r["digests"].items() if g["digests"].get(sec) != d]
        if g["features"] != r["features"] or len(g["digests"]) != len(r["digests"]):
            wrong.append("%s: features / sections" % name)
    assert not wrong, wrong


def test_the_cases_reach_every_branch(results):
    """a condition on the inputs above: every bit of the feature word is set by some case (and by more than a single one
    where that was cheap), so the golden file pins every branch of the planner"""
    union = 0
    for r in results.values():
        union |= r["features"]
    missing = [FEATURES[b] for b in range(len(FEATURES)) if not union >> b & 1]
    assert not missing, missing
