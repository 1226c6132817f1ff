"""CPU: the sparse routes planned in two steps.  build_tiles DECIDES (the planes a tile routes, the slabs in the order that
gives them their indices) and emit_sparse_items EMITS (the items in launch order, the table-only marks, the counters) behind
the dense path's own steps, as engine.hip calls them; build_pairs does both at once.

* Over a seeded sweep both ways give the same plan, list for list (dshh_plan_sparse_items, two_step = 0 and 1).
* Where Tuning::sparse_max_slabs binds, a tile's route depends on the slabs made before it, so the decisions must make the
  slabs in the order the one-step planner made them: the routes, slabs, items and dense chunk ranges of such plans are
  compared with tests/golden/sparse_emit_slabs.json, which was written by the planner as it stood BEFORE the split (this
  file's hook alone applied to that commit, two_step = 0) and is never regenerated from the code under test.  Each case
  first asserts that the budget refused at least one tile that routes without it.

Writing mode (for a planner whose output is the reference): DSH_SPARSE_EMIT_WRITE=1 python -m pytest tests/test_sparse_emit.py"""
import hashlib
import json
import os

import pytest

import sparse_order_ref as ref
from test_plan_digest import make_inputs

GOLDEN = os.path.join(ref.ROOT, "tests", "golden", "sparse_emit_slabs.json")
LISTS = ("tiles", "chunks", "bands", "items", "slabs")
SCALARS = ("sided_items", "transposed_items", "table_slabs", "dense_items")

SWEEP = {"sweep_%d" % s: (200 + s, 260 + 173 * s, 13 + s % 4, 3 + s % 5,
                          dict(sp=(-1, 2, 1, 0)[s % 4], sd=(1, -1, 1)[s % 3], budget=(8 << 30, 1 << 20, 3 << 20, 32 << 20)[s % 4],
                               **(dict(rb=128, re=200 + 150 * s, nparts=3, want_parts=1) if s % 5 == 4 else {})))
         for s in range(20)}
# sparse_max_slabs small enough to bind: (seed, n, p, spread, arguments)
BINDING = {
    "sided_40_slabs": (31, 1500, 14, 4, dict(sp=0, sd=1, max_slabs=40)),
    "both_routes_100_slabs": (32, 2000, 14, 4, dict(sp=2, sd=1, thr_cap=2040, max_slabs=100)),
    "two_plane_16_slabs": (33, 2000, 14, 4, dict(sp=2, sd=0, thr_cap=2040, max_slabs=16)),
    "bands_60_slabs": (34, 2000, 14, 4, dict(sp=2, sd=1, budget=4 << 20, max_slabs=60)),
    "automatic_p16_30_slabs": (35, 1200, 16, 4, dict(max_slabs=30)),
}


@pytest.fixture(scope="module")
def host():
    return ref.load()


def planned(host, case, **more):
    seed, n, p, spread, kw = case
    keys, cnt, thr = make_inputs(seed, n, p, spread, kw.get("thr_cap", 1280))
    return ref.plan(host, keys, cnt, thr, p, **dict(kw, **more))


def same_plan(a, b):
    return [k for k in LISTS if a[k].tobytes() != b[k].tobytes()] + [k for k in SCALARS if a[k] != b[k]]


@pytest.mark.parametrize("name", sorted(SWEEP) + sorted(BINDING))
def test_two_steps_give_the_plan_of_one(host, name):
    case = SWEEP.get(name) or BINDING[name]
    one, two = planned(host, case, two_step=0), planned(host, case, two_step=1)
    assert not same_plan(one, two), name


def test_the_sweep_routes(host):
    items = [len(planned(host, c, two_step=1)["items"]) for c in SWEEP.values()]
    assert sum(1 for k in items if k > 0) >= len(items) // 2 and sum(items) > 5000, items


def digests(pl):
    d = {k: hashlib.sha256(pl[k].tobytes()).hexdigest() for k in LISTS}
    d.update({k: pl[k] for k in SCALARS})
    d["shape"] = [len(pl[k]) for k in LISTS]
    return d


@pytest.fixture(scope="module")
def binding(host):
    res = {name: digests(planned(host, case, two_step=0)) for name, case in BINDING.items()}
    if os.environ.get("DSH_SPARSE_EMIT_WRITE") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(res, f, indent=0, sort_keys=True)
            f.write("\n")
    return res


@pytest.mark.parametrize("name", sorted(BINDING))
def test_binding_slab_budget_keeps_the_plan(host, binding, name):
    case = BINDING[name]
    free, bound = planned(host, case, max_slabs=0, two_step=1), planned(host, case, two_step=1)
    refused = ((free["tiles"][:, 4:6].sum(axis=1) > 0) & (bound["tiles"][:, 4:6].sum(axis=1) == 0)).sum()
    assert refused > 0 and len(bound["items"]) > 0 and len(bound["slabs"]) <= case[4]["max_slabs"], (name, refused, len(bound["slabs"]))
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert digests(bound) == golden[name] == binding[name], name
