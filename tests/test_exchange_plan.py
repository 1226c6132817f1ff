"""The round schedule of dsh_exchange_collect_async (csrc/exchange_plan.h, through dshh_exchange_plan of
csrc/host/plan_capi.cpp) against its contract, restated here in plain Python from DESIGN.md 5 and the loops of the entry
point as they stood.  Both sides of a message run the same function, so the transport tests only prove that they agree:
a changed schedule shows up here, or on a clock with more than one GPU.
  messages  a source's buffer of `total` floats travels in M = nparts messages, message q = [total q / M, total (q + 1) / M)
  gate      message q is posted behind the first part that ends at or beyond the message's end (the last part at most)
  rounds    a source posts round q where its message is not empty, the destination where any source's is not
  placement a row of a row-sorted source is placed behind the first round after which its last float has arrived: per
            round and source one entry of consecutive positions, the entries' row0 the prefix sums of a round
  tables    per row-sorted source rowoff then order, 16-byte aligned, the entries behind them; stage_off the prefix sums
            of the sources' totals; what the destination derives from the keys is what the source's layout holds
The digests of tests/golden/exchange_plan.json were made where the loops of dsh_exchange_collect_async had been moved
behind xplan::schedule verbatim, before anything was reshaped."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "exchange_plan.json")
ENT_BYTES = 40  # sizeof(PlaceEnt): three pointers, pos0, row0, nrows
DTYPES = ["<u8", "<u8", "u1", "<u4", "<u8", "<u8", "<u8", "<u8", "<u4", "<u4", "<u8", "<u4", "<u4", "<u8"]
NAMES = ["total", "msg", "post", "gate", "part_end", "stage_off", "tab_off", "ents", "round_ent", "round_rows", "rowoff", "order", "modes", "cut"]


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    u64, u32, i32, vp = C.c_uint64, C.c_uint32, C.c_int, C.c_void_p
    lib.dshh_exchange_plan.argtypes = [u64, vp, vp, u32, i32, i32, i32, vp, vp, vp]
    lib.dsh_balance_rows.argtypes = [u64, u32, vp]
    lib.dsh_balance_rowsets.argtypes = [u64, u32, i32, i32, i32, vp, u32, C.POINTER(u32)]
    lib.dsh_rowsets_from_bounds.argtypes = [vp, u32, vp]
    lib.dshh_rowsorted_split.restype = u64
    lib.dshh_rowsorted_split.argtypes = [u64, u64, u64]
    return lib


def make_keys(rng, n, p, spread=6):
    """per-sketch keys as tests/test_plan.py makes them: lo <= L <= T <= hi <= 64 - p + 1"""
    q1 = 64 - p + 1
    lo = rng.integers(0, max(1, q1 - spread), n)
    w = rng.integers(0, spread + 1, (3, n))
    L = np.minimum(lo + w[0], q1)
    T = np.minimum(L + w[1], q1)
    hi = np.minimum(T + w[2], q1)
    return (hi.astype(np.uint32) << 18 | T.astype(np.uint32) << 12 | L.astype(np.uint32) << 6 | lo.astype(np.uint32)).astype(np.uint32)


def table_from_bounds(host, bounds):
    b = np.ascontiguousarray(bounds, np.uint64)
    tab = np.zeros(3 + 2 * (len(b) - 1), np.uint64)
    assert host.dsh_rowsets_from_bounds(b.ctypes.data, len(b) - 1, tab.ctypes.data) == 0
    return tab


def balanced_bounds(host, n, world):
    b = np.zeros(world + 1, np.uint64)
    assert host.dsh_balance_rows(n, world, b.ctypes.data) == 0
    return b


def balanced_rowsets(host, n, world):
    words = C.c_uint32()
    assert host.dsh_balance_rowsets(n, world, -1, -1, -1, None, 0, C.byref(words)) == 0
    tab = np.zeros(words.value, np.uint64)
    assert host.dsh_balance_rowsets(n, world, -1, -1, -1, tab.ctypes.data, len(tab), C.byref(words)) == 0
    return tab


def cases(host):
    """name -> (n, table, [(dst, nparts), ...])"""
    out = {}
    # tests/test_gpu_multirank.py: test_exchange_pair_virtual_ranks_row_sorted_parts and _row_sets
    for world, dst, nparts in ((1, 0, 4), (2, 0, 8), (3, 1, 2), (8, 0, 8), (8, 7, 3), (5, 2, 1)):
        out["bounds2600_w%d_d%d_k%d" % (world, dst, nparts)] = (2600, table_from_bounds(host, balanced_bounds(host, 2600, world)), [(dst, nparts)])
    for world, dst, nparts in ((2, 0, 8), (3, 1, 2), (4, 3, 4), (8, 0, 8), (8, 7, 3), (5, 2, 1)):
        out["rowsets3300_w%d_d%d_k%d" % (world, dst, nparts)] = (3300, balanced_rowsets(host, 3300, world), [(dst, nparts)])
    out["ragged_4"] = (1700, table_from_bounds(host, [0, 0, 640, 1699, 1700]), [(0, 4), (3, 4), (2, 8)])
    out["ragged_3"] = (1700, table_from_bounds(host, [0, 0, 900, 1700]), [(0, 4), (2, 4), (1, 3)])
    out["ranks_without_rows"] = (700, balanced_rowsets(host, 700, 8), [(0, 8), (7, 4)])
    out["ranks_without_rows_bounds"] = (700, table_from_bounds(host, balanced_bounds(host, 700, 8)), [(0, 8), (3, 2)])
    out["one_part"] = (2600, balanced_rowsets(host, 2600, 4), [(0, 1), (3, 1)])
    out["more_parts_than_tile_rows"] = (1400, table_from_bounds(host, balanced_bounds(host, 1400, 2)), [(0, 8), (1, 8)])
    out["two_runs"] = (5200, table_from_bounds(host, balanced_bounds(host, 5200, 2)), [(0, 8), (1, 8)])
    out["long_range_plain"] = (9000, table_from_bounds(host, balanced_bounds(host, 9000, 2)), [(0, 2), (1, 2)])
    out["n1"] = (1, table_from_bounds(host, [0, 1]), [(0, 4)])
    out["n1_w2"] = (1, table_from_bounds(host, [0, 0, 1]), [(0, 4), (1, 2)])
    out["n2"] = (2, table_from_bounds(host, [0, 2]), [(0, 4)])
    out["n2_w2"] = (2, table_from_bounds(host, [0, 1, 2]), [(0, 4), (1, 1)])
    return out


def keys_for(name, n):
    return make_keys(np.random.default_rng(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)), n, 12, spread=10)


def plan(host, n, keys, tab, nparts, dst, rank, fine):
    """the lists by name (sizes from a call without buffers, the lists from a second one) and info"""
    counts, info = np.zeros(14, np.uint64), np.zeros(3, np.uint64)
    args = (n, keys.ctypes.data, tab.ctypes.data, nparts, dst, rank, fine)
    assert host.dshh_exchange_plan(*args, None, counts.ctypes.data, info.ctypes.data) == 0
    lists = [np.zeros(int(c), dt) for dt, c in zip(DTYPES, counts)]
    bufs = (C.c_void_p * 14)(*[a.ctypes.data for a in lists])
    sizes = counts.copy()
    assert host.dshh_exchange_plan(*args, bufs, counts.ctypes.data, info.ctypes.data) == 0 and (counts == sizes).all()
    counts[0] -= 1  # a buffer too small is refused
    assert host.dshh_exchange_plan(*args, bufs, counts.ctypes.data, info.ctypes.data) == -2
    P = dict(zip(NAMES, lists))
    P["stage_total"], P["ent_off"], P["tab_bytes"] = (int(x) for x in info)
    return P


def rank_rows(tab, r):
    """a rank's rows (csrc/plan.h): the segments it owns, adjacent ones merged; the first is its main range"""
    nseg = int(tab[1])
    b, own = [int(x) for x in tab[2:3 + nseg]], [int(x) for x in tab[3 + nseg:3 + 2 * nseg]]
    segs = []
    for s in range(nseg):
        if own[s] != r or b[s] == b[s + 1]:
            continue
        if segs and segs[-1][1] == b[s]:
            segs[-1][1] = b[s + 1]
        else:
            segs.append([b[s], b[s + 1]])
    return segs


def span(n, b, e):
    return sum(n - 1 - i for i in range(b, e))


def split_tables(P, tab, world, dst, rank):
    """rank -> (rowoff, order) of the row-sorted ranks this plan knows: the lists hold them one behind the other in rank order"""
    out, ro_at, ord_at = {}, 0, 0
    for r in range(world):
        rs = int(P["modes"][3 * r])
        if not rs or r == dst or not (rank == dst or r == rank):
            continue
        cnt = sum(e - b for b, e in rank_rows(tab, r))
        out[r] = ([int(x) for x in P["rowoff"][ro_at:ro_at + cnt + 1]], [int(x) for x in P["order"][ord_at:ord_at + cnt]])
        ro_at += cnt + 1
        ord_at += cnt
    assert ro_at == len(P["rowoff"]) and ord_at == len(P["order"])
    return out


def check_rank(n, tab, world, nparts, dst, rank, P, tables):
    """one calling rank's plan against the contract; tables: what split_tables gave for it"""
    M = nparts
    rows = [rank_rows(tab, r) for r in range(world)]
    rs = [int(P["modes"][3 * r]) != 0 for r in range(world)]
    # a buffer's floats: a row-sorted rank's rows one behind the other, a plain range's span; the destination sends nothing
    want_total = []
    for r in range(world):
        if r == dst or not rows[r]:
            want_total.append(0)
        elif rs[r]:
            want_total.append(sum(span(n, b, e) for b, e in rows[r]) if r in tables else 0)
        else:
            assert len(rows[r]) == 1, "a rank with extra segments is row-sorted"
            want_total.append(span(n, *rows[r][0]))
    assert [int(x) for x in P["total"]] == want_total
    for r, (ro, order) in tables.items():
        assert ro[0] == 0 and ro[-1] == want_total[r] and sorted(order) == [i for b, e in rows[r] for i in range(b, e)]
        assert all(ro[s + 1] - ro[s] == n - 1 - order[s] for s in range(len(order)))
    # messages 0 .. M - 1 tile [0, total) once and in order
    msg = P["msg"].reshape(M, world, 2)
    for r in range(world):
        for q in range(M):
            first, cnt = int(msg[q, r, 0]), int(msg[q, r, 1])
            assert (first, first + cnt) == (want_total[r] * q // M, want_total[r] * (q + 1) // M)
    ends = [[want_total[r] * (q + 1) // M for q in range(M)] for r in range(world)]
    if rank != dst:
        assert P["post"].tolist() == [int(msg[q, rank, 1] != 0) for q in range(M)]
        cut = [int(x) for x in P["cut"]]
        k = int(P["modes"][3 * rank + 1])
        assert len(cut) == (k + 1 if rows[rank] else 0)
        if rs[rank]:
            part_end = [tables[rank][0][c] for c in cut[1:]]
        else:
            part_end = [span(n, rows[rank][0][0], c) for c in cut[1:]]
        assert [int(x) for x in P["part_end"]] == part_end and part_end == sorted(part_end)
        gates = []
        for q in range(M):
            if not msg[q, rank, 1]:
                continue
            g = min([i for i, e in enumerate(part_end) if e >= ends[rank][q]] + [len(part_end) - 1])
            assert int(P["gate"][q]) == g
            gates.append(g)
        assert gates == sorted(gates), "a message may not wait for an earlier part than the message before it"
        if gates:
            assert part_end[-1] == want_total[rank] and gates[-1] == len(part_end) - 1
        assert P["stage_total"] == 0 and P["tab_bytes"] == 0 and len(P["ents"]) == 0 and not P["round_rows"].any()
        return
    assert P["post"].tolist() == [int(any(msg[q, r, 1] for r in range(world))) for q in range(M)]
    assert len(P["part_end"]) == 0 and not P["gate"].any()
    # staging and the table upload
    sources = [r for r in range(world) if r in tables]
    stage_at, tab_at = 0, 0
    for r in sources:
        cnt = len(tables[r][1])
        assert int(P["stage_off"][r]) == stage_at and int(P["tab_off"][r]) == tab_at and tab_at % 16 == 0
        stage_at += want_total[r]
        tab_at += (8 * (cnt + 1) + 4 * cnt + 15) // 16 * 16
    assert P["stage_total"] == stage_at
    ents = P["ents"].reshape(-1, 4).tolist()
    if not stage_at:
        assert not ents and P["tab_bytes"] == tab_at and not P["round_rows"].any() and not P["round_ent"].any()
        return
    assert P["ent_off"] == tab_at and P["tab_bytes"] == tab_at + ENT_BYTES * len(ents)
    # every position of a row-sorted source in exactly one entry: that of the first round after which the row's last float
    # has arrived
    want = []
    round_ent, round_rows = [], []
    for q in range(M):
        round_ent.append(len(want))
        row0 = 0
        for r in sources:
            ro = tables[r][0]
            pos = [s for s in range(len(ro) - 1) if ro[s + 1] <= ends[r][q] and (q == 0 or ro[s + 1] > ends[r][q - 1])]
            if not pos:
                continue
            assert pos == list(range(pos[0], pos[-1] + 1))
            want.append([r, pos[0], row0, len(pos)])
            row0 += len(pos)
        round_rows.append(row0)
    round_ent.append(len(want))
    assert ents == want and P["round_ent"].tolist() == round_ent and P["round_rows"].tolist() == round_rows
    for r in sources:
        covered = sorted(p for e in ents if e[0] == r for p in range(e[1], e[1] + e[3]))
        assert covered == list(range(len(tables[r][1])))


def run_case(host, name, n, tab, runs, digest=None):
    world = int(tab[0])
    keys = keys_for(name, n)
    seen = dict(rowsorted=False, plain=False)
    for dst, nparts in runs:
        for fine in (0, 1):
            plans = [plan(host, n, keys, tab, nparts, dst, r, fine) for r in range(world)]
            tabs = [split_tables(plans[r], tab, world, dst, r) for r in range(world)]
            for r in range(world):
                check_rank(n, tab, world, nparts, dst, r, plans[r], tabs[r])
                if digest is not None:
                    for nm in NAMES:
                        digest.update(np.uint64(plans[r][nm].size).tobytes())
                        digest.update(plans[r][nm].tobytes())
                    digest.update(np.array([plans[r]["stage_total"], plans[r]["ent_off"], plans[r]["tab_bytes"]], np.uint64).tobytes())
            # the two sides of every message agree, and the destination derives the tables the source's layout holds
            D = plans[dst]
            for r in range(world):
                if r == dst:
                    continue
                S = plans[r]
                assert (S["msg"].reshape(nparts, world, 2)[:, r] == D["msg"].reshape(nparts, world, 2)[:, r]).all()
                assert all(D["post"][q] for q in range(nparts) if S["post"][q]), "a round a source posts, the destination posts"
                # (whether a source cut finely changes its parts, never what the destination sees)
                assert (S["modes"].reshape(world, 3)[:, 0] == D["modes"].reshape(world, 3)[:, 0]).all()
                if r in tabs[r]:
                    assert tabs[dst][r] == tabs[r][r], "rank %d: the destination's tables are not the source's" % r
                    seen["rowsorted"] = True
                    if fine:
                        assert S["modes"][3 * r + 2] >= 256 and S["modes"][3 * r + 1] >= 1
                elif rank_rows(tab, r):
                    seen["plain"] = True
    return seen


def test_schedule_against_its_contract(host):
    seen = {}
    for name, (n, tab, runs) in cases(host).items():
        seen[name] = run_case(host, name, n, tab, runs)
    assert seen["long_range_plain"] == dict(rowsorted=False, plain=True)
    assert seen["two_runs"]["rowsorted"] and seen["rowsets3300_w8_d0_k8"]["rowsorted"] and seen["ranks_without_rows"]["rowsorted"]
    # what the names promise: a range key-ordered as two runs; ranks without rows; more parts asked for than tile rows
    b = balanced_bounds(host, 5200, 2)
    assert host.dshh_rowsorted_split(5200, int(b[1]), int(b[2])) < int(b[2])
    assert any(not rank_rows(cases(host)["ranks_without_rows"][1], r) for r in range(8))
    b = balanced_bounds(host, 1400, 2)
    assert any((int(b[r + 1]) - int(b[r]) + 127) // 128 < 8 for r in range(2))


def test_golden_digests(host):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = {}
    for name, (n, tab, runs) in cases(host).items():
        h = hashlib.sha256()
        run_case(host, name, n, tab, runs, h)
        got[name] = h.hexdigest()
    assert sorted(got) == sorted(want)
    assert got == want
