"""CPU: the launch order of the sparse items (plan.cpp, order_sparse_items -- counting passes over a packed key) held to the
order rule restated in numpy (tests/sparse_order_ref.py: stable np.lexsort, the least-loaded assignment, the interleave),
band by band, on the items dshh_plan_sparse_items returns in launch order.  The inputs are those of
tests/test_plan_digest.py (an integer generator: no numpy version enters); what the cases have to contain -- fewer than eight
table blocks, blocks with equal item counts, bands of one and of no item, transposed items, both routes, several bands, 80
blocks -- is asserted on the plans themselves."""
import numpy as np
import pytest

import sparse_order_ref as ref
from test_plan_digest import make_inputs

# name -> (seed, n, p, spread, keyword arguments of sparse_order_ref.plan)
CASES = {
    "few_blocks_sided": (11, 600, 14, 4, dict(sp=0, sd=1)),
    "few_blocks_two_plane": (12, 700, 14, 4, dict(sp=2, sd=0, thr_cap=2040)),
    "both_routes_forced": (13, 2000, 14, 4, dict(sp=2, sd=1, thr_cap=2040)),
    "automatic": (14, 2600, 14, 4, dict()),
    "bands_4MiB": (15, 2000, 14, 4, dict(sp=2, sd=1, budget=4 << 20)),
    "bands_1MiB": (16, 1100, 14, 5, dict(sp=2, sd=1, budget=1 << 20)),
    "bands_one_tile": (17, 900, 13, 6, dict(sp=1, sd=1, budget=1 << 10)),
    "parts_small_bands": (18, 2500, 14, 4, dict(rb=384, re=2200, nparts=3, want_parts=1, budget=48 << 20)),
    "p16": (19, 1200, 16, 4, dict(sp=-1, sd=-1)),
    "p13_two_plane": (20, 2500, 13, 5, dict(sp=2, sd=0)),
    "blocks_80": (21, 10200, 14, 4, dict()),
    "blocks_80_two_bands": (22, 10200, 14, 3, dict(sp=2, sd=1, thr_cap=2040, budget=1 << 30)),
}
CASES.update({"sweep_%d" % s: (100 + s, 300 + 137 * s, 13 + s % 4, 3 + s % 5, dict(sp=(-1, 1, 2, 0)[s % 4], sd=(1, -1, 1)[s % 3],
                                                                                   budget=(8 << 30, 2 << 20, 1 << 20, 16 << 20)[s % 4]))
              for s in range(16)})


@pytest.fixture(scope="module")
def host():
    return ref.load()


@pytest.fixture(scope="module")
def plans(host):
    out = {}
    for name, (seed, n, p, spread, kw) in CASES.items():
        cap = kw.get("thr_cap", 1280)
        keys, cnt, thr = make_inputs(seed, n, p, spread, cap)
        out[name] = ref.plan(host, keys, cnt, thr, p, **kw)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_order_is_the_rule(plans, name):
    pl = plans[name]
    for band in pl["bands"]:
        got = pl["items"][int(band[2]) : int(band[3])]
        emitted = ref.emission_sorted(pl["tiles"], band, got)
        want = emitted[ref.launch_order(pl["tiles"], band, emitted)] if len(emitted) else emitted
        assert got.tobytes() == want.tobytes(), (name, band.tolist())


def table_blocks(pl, band):
    it = pl["items"][int(band[2]) : int(band[3])]
    T = pl["tiles"][int(band[0]) + it[:, 0].astype(np.int64)]
    return np.where(it[:, 1] & ref.TRANSPOSED, T[:, 0], T[:, 1])


def test_the_cases_hold_what_the_order_can_get_wrong(plans):
    seen = dict.fromkeys(("fewer than eight table blocks", "more than eight table blocks", "equal item counts", "band of one item",
                          "band of no item beside one with items", "transposed", "two-plane items", "sided items", "several bands", "80 blocks"), False)
    for pl in plans.values():
        routed = pl["bands"][:, 3] > pl["bands"][:, 2]
        seen["several bands"] |= len(pl["bands"]) > 1 and bool(routed.any())
        seen["band of no item beside one with items"] |= bool(routed.any() and not routed.all())
        seen["transposed"] |= pl["transposed_items"] > 0
        seen["sided items"] |= pl["sided_items"] > 0
        seen["two-plane items"] |= len(pl["items"]) > pl["sided_items"]
        seen["80 blocks"] |= pl["NT"] >= 80 and len(pl["items"]) > 0
        for band in pl["bands"]:
            k = int(band[3] - band[2])
            seen["band of one item"] |= k == 1
            if k < 2:
                continue
            _, per = np.unique(table_blocks(pl, band), return_counts=True)
            seen["fewer than eight table blocks"] |= len(per) < 8
            seen["more than eight table blocks"] |= len(per) > 8
            seen["equal item counts"] |= len(per) > 8 and len(set(per.tolist())) < len(per)
    assert all(seen.values()), [k for k, v in seen.items() if not v]
