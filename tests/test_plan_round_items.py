"""CPU: the pair planner at a round of 768 work items (three items per workgroup of the lockstep tile kernel instead of
two; engine.hip sets Tuning::round_items = 256 x the items per workgroup and, under pair_groups = auto, lets a band of
at most two rounds of 512 keep that round).  dshh_plan_check_ri is dshh_plan_check (tests/test_plan.py) with the
round given: every wanted pair owned by exactly one (tile, lane), items covering every tile's chunks once, overflow
fragments only behind whole rounds of the band's own round, tail bands cut at whole rounds."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    u64, i32, u32, vp = C.c_uint64, C.c_int, C.c_uint32, C.c_void_p
    lib.dshh_plan_check_ri.argtypes = [u64, vp, i32, i32, u64, u64, u64, u64, u32, i32, i32, u64, i32, i32, i32, u32, vp, C.c_char_p, C.c_size_t]
    lib.dsh_balance_rows.argtypes = [u64, u32, vp]
    return lib


def make_keys(rng, n, p, spread=6):
    """per-sketch keys as k_selfhist_card writes them: lo <= L <= T <= hi <= 64 - p + 1"""
    q1 = 64 - p + 1
    lo = rng.integers(0, max(1, q1 - spread), n)
    w = rng.integers(0, spread + 1, (3, n))
    L = np.minimum(lo + w[0], q1)
    T = np.minimum(L + w[1], q1)
    hi = np.minimum(T + w[2], q1)
    return (hi.astype(np.uint32) << 18 | T.astype(np.uint32) << 12 | L.astype(np.uint32) << 6 | lo.astype(np.uint32)).astype(np.uint32)


def check(host, keys, ri, rb=0, re=None, nparts=1, want_parts=0, p=12, budget=8 << 30, nsplit=0, expect_ok=True):
    n = len(keys)
    re = n if re is None else re
    stats = np.zeros(10, np.uint64)
    err = C.create_string_buffer(512)
    rc = host.dshh_plan_check_ri(n, keys.ctypes.data, 0, 1, rb, re, 0, 0, nparts, want_parts, p, budget, 1, nsplit, 64, ri,
                                 stats.ctypes.data, err, 512)
    if not expect_ok:
        assert rc != 0
        return None
    assert rc == 0, err.value.decode()
    return dict(tiles=int(stats[0]), bands=int(stats[1]), items=int(stats[2]), parts=int(stats[3]), rounds=int(stats[7]), frags=int(stats[8]),
                round=int(stats[9]))


def test_every_pair_is_covered_once_at_a_round_of_768(host):
    rng = np.random.default_rng(41)
    for n in (1, 2, 127, 129, 700, 1500):
        for p in (10, 12, 14):
            keys = make_keys(rng, n, p)
            a, b = check(host, keys, 512, p=p), check(host, keys, 768, p=p)
            nt = (n + 127) // 128
            assert a["tiles"] == b["tiles"] == nt * (nt + 1) // 2
            # the round only moves where whole items end and fragments begin
            assert a["items"] - a["frags"] <= b["items"] or b["frags"]
    for _ in range(10):
        n = int(rng.integers(2, 1800))
        keys = make_keys(rng, n, 12)
        rb = int(rng.integers(0, n))
        check(host, keys, 768, rb=rb, re=int(rng.integers(rb, n + 1)), nsplit=int(rng.integers(0, 4)))


def test_fragments_sit_only_behind_whole_rounds_of_the_bands_round(host):
    """one band each: it runs in rounds of 768 or, when it holds at most 1 024 items (two rounds of two-item workgroups),
    of 512; fragments only behind whole rounds of THAT round, at most one round of them"""
    rng = np.random.default_rng(31)
    seen = {"frag": 0, "none": 0, 512: 0, 768: 0}
    for n in range(600, 3400, 100):
        keys = make_keys(rng, n, 14, spread=6)
        st = check(host, keys, 768, p=14)
        ri = st["round"]
        assert ri in (512, 768) and st["bands"] == 1, st
        seen[ri] += 1
        whole = st["items"] - st["frags"]
        if st["frags"]:
            seen["frag"] += 1
            assert whole % ri == 0 and 2 <= st["frags"] <= ri, st
        else:
            seen["none"] += 1
        assert st["rounds"] == -(-whole // ri) + (1 if st["frags"] else 0)
        # (a fragment is at least half an item: the band held between whole + frags / 2 and whole + frags items)
        if whole + st["frags"] <= 1024:
            assert ri == 512, st
        if whole + st["frags"] // 2 > 1024:
            assert ri == 768, st
    assert seen["frag"] >= 2 and seen["none"] >= 1 and seen[512] >= 2 and seen[768] >= 2, seen


def test_the_headline_ranges_over_8_ranks_plan_at_768(host):
    """every rank's range of dsh_balance_rows(10 000, 8), in 8 parts (tail bands cut at whole rounds of 768)"""
    rng = np.random.default_rng(3)
    n = 10000
    keys = make_keys(rng, n, 14)
    bounds = np.zeros(9, np.uint64)
    assert host.dsh_balance_rows(n, 8, bounds.ctypes.data) == 0
    for r in range(8):
        st = check(host, keys, 768, rb=int(bounds[r]), re=int(bounds[r + 1]), nparts=8, want_parts=1, p=14)
        assert st["parts"] >= 1
        assert st["rounds"] <= -(-st["items"] // 512) + st["bands"], st


def test_the_round_must_be_a_multiple_of_256(host):
    keys = make_keys(np.random.default_rng(5), 300, 12)
    for ri in (0, 100, 700):
        check(host, keys, ri, expect_ok=False)
