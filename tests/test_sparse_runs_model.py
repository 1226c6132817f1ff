"""CPU: the runs of the LDS placement of the sparse counting kernel and its table stagings (dashing_amd/csrc/plan.h,
sparse_table_fills, through dshh_sparse_table_fills of the host library) against the numpy restatement of
tests/sparse_runs.py -- on the item lists the planner makes for the collections of tests/test_gpu_sparse_runs.py, and on
hand-made lists that hold every condition a run can meet: a table slab that changes inside a run, a transposed item followed
by a plain one of the same table slab and the reverse, a ragged last run, a run of a single item, a whole residue in one run."""
import numpy as np
import pytest

import sparse_runs as sr
from sparse_cases import pcs
from test_sparse_sided_model import case, host, plan  # noqa: F401  (host: the fixture of the host library)

T = sr.TRANSPOSED


def item(tile, row_slab, col_slab, transposed=False, plane=3):
    return (tile, plane, T if transposed else 0, row_slab, col_slab)


@pytest.mark.parametrize("n,p", ((257, 13), (257, 14), (641, 14), (257, 15)))
@pytest.mark.parametrize("kind", ("mixed_thresholds", "survey", "near_duplicates"))
def test_fills_of_planned_items(host, kind, n, p):
    _, keys, gcnt, thr = case(kind, n, p)
    st, _, items, _ = plan(host, keys, gcnt, thr, pcs.SPARSE_CAP, p, 1)
    assert st["bands"] == 1 and len(items) > 8
    for run in sr.RUNS + (5, 1 << 16):
        assert sr.host_fills(host, items, run) == sr.fills(items, run), (kind, n, p, run)
    assert sr.host_fills(host, items, 1) == 4 * len(items)
    assert sr.host_fills(host, items, 64) <= sr.host_fills(host, items, 2) <= 4 * len(items)


def test_hand_made_lists(host):
    # residue 0 of 8 holds the story; the other residues one item each of slabs of their own (single-item runs)
    story = [item(0, 10, 20),                    # plain, table slab 20
             item(1, 11, 20),                    # plain, the same table: no staging
             item(2, 20, 12, transposed=True),   # transposed: its table is the ROW block's slab, 20 again (plain then transposed)
             item(3, 13, 20),                    # plain on slab 20 (transposed then plain)
             item(4, 13, 21),                    # the table changes inside the run
             item(5, 21, 14, transposed=True),   # transposed, table 21: no staging
             item(6, 22, 15, transposed=True)]   # transposed, table 22
    items = []
    for k, it in enumerate(story):
        items.append(it)
        if k == 0:
            items += [item(100 + x, 30 + x, 40 + x) for x in range(1, 8)]
        elif k + 1 < len(story):
            items += [item(200 + 8 * k + x, 50, 60 + 8 * k + x) for x in range(1, 8)]  # residues 1..7: a new table every item
    items = np.array(items, np.uint32)  # 6 * 8 + 1 items: residue 0 has 7, the others 6
    assert len(items) == 49
    want = {}
    for run in (1, 2, 3, 4, 7, 8, 64):
        c = sr.conditions(items, run)
        want[run] = sr.fills(items, run)
        assert sr.host_fills(host, items, run) == want[run], run
        if run == 7:  # residue 0 in one run, the others (six items) end ragged
            assert c["slab_change"] and c["transposed_then_plain"] and c["plain_then_transposed"] and c["ragged"]
        if run == 4:
            assert c["ragged"] and c["slab_change"]
        if run == 64:
            assert c["whole_residue"] and c["ragged"]
    # residue 0 alone, by hand: tables 20 20 20 20 21 21 22
    alone = items[0::8]
    assert [sr.host_fills(host, alone[k : k + 1], 1) for k in range(7)] == [4] * 7
    r0 = {1: 7, 2: 1 + 1 + 1 + 1, 3: 1 + 2 + 1, 4: 1 + 2, 7: 3, 8: 3, 64: 3}  # stagings of residue 0 (runs of 2: 20 20|20 20|21 21|22)
    others = 7 * 6  # every item of the residues 1..7 has a table of its own
    for run, f in r0.items():
        assert want[run] == 4 * (f + others), (run, want[run])
    assert sr.conditions(items[:1], 8)["single"]


def test_edges(host):
    assert sr.host_fills(host, np.zeros((0, 5), np.uint32), 4) == 0
    one = np.array([item(0, 1, 2)], np.uint32)
    assert sr.host_fills(host, one, 1) == sr.host_fills(host, one, 64) == 4
    same = np.array([item(k, 1, 2) for k in range(20)], np.uint32)  # one table: a staging per run
    for run in (1, 2, 3, 8, 64):
        assert sr.host_fills(host, same, run) == sr.fills(same, run) == 4 * sum(-(-len(range(x, 20, 8)) // run) for x in range(8))
