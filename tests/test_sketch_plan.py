"""The sketch path's host planning (csrc/sketch_plan.h, through dshh_sketch_plan of csrc/host/plan_capi.cpp) against its
contract, restated here in plain Python.  Sketch results do not depend on how a call is cut (the merge is a byte-wise max),
so no GPU test notices a changed cut: these do.
  genomes  every genome of at least k bases is cut into work items whose sub-chunks (8 192 bases) tile [gb & ~31, ge) once
           and in order; all items of a call but a genome's last walk subs_rule(p, total sub-chunks of the call) of them
  records  a record that fits 8 192 bases from its 32-aligned base lies in exactly one run of consecutive records (greedy
           cut: span <= 8 192, at most 256 segments = non-empty records, at most 4 096 records); a longer one has its row
           cleared and is cut like a genome; above p = 17 every record is a genome
  FASTX    a genome's raw bytes in chunks of 16 KiB; the format from its first byte; bad regions refused
The digests of tests/golden/sketch_plan.json were made from the planning loops as they stood inside the entry points,
before they were unified."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sketch_plan.json")
SUB, RUN_SPAN, RUN_SEGS, RUN_RECS, MAX_P_RECORDS, FX_CHUNK = 8192, 8192, 256, 4096, 17, 16384
WORK = np.dtype([("gbeg", "<u8"), ("gend", "<u8"), ("start", "<u8"), ("nsub", "<u4"), ("slot", "<u4")])
RUN = np.dtype([("base", "<u8"), ("seg0", "<u4"), ("nseg", "<u4"), ("slot0", "<u4"), ("nrec", "<u4"), ("span", "<u4"), ("pad", "<u4")])
SEG = np.dtype([("start", "<u4"), ("slot", "<u4")])
ROW = np.dtype("<u4")
GEN = np.dtype([("off", "<u8"), ("rawlen", "<u8"), ("region_end", "<u8"), ("chunk0", "<u4"), ("nchunks", "<u4"), ("fmt", "<u4"), ("pad", "<u4")])
CHUNK = np.dtype([("begin", "<u8"), ("len", "<u4"), ("genome", "<u4")])
LISTS = {0: (WORK,), 1: (RUN, SEG, ROW, WORK), 2: (GEN, CHUNK)}
# the EDGE list of tests/test_gpu_records.py (a copy: this module imports nothing of the GPU tests)
EDGE = [0, 1, 30, 31, 32, 33, 5, 4, 6, 20, 21, 22, 150, 1000, 8191, 8192, 8193, 0, 0, 2, 64, 65, 63, 7000, 1200]


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    lib.dshh_sketch_plan.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.dshh_sketch_plan.restype = C.c_int
    return lib


def plan(host, kind, off, first_slot=0, k=31, p=10, first_byte=None, raw_len=None):
    """(rc, lists, info): the sizes from a call without buffers, the lists from a second one"""
    off = np.ascontiguousarray(off, np.uint64)
    n = off.size - 1
    fb = None if first_byte is None else np.ascontiguousarray(first_byte, np.uint8)
    rl = None if raw_len is None else np.ascontiguousarray(raw_len, np.uint64)
    counts, info = np.zeros(4, np.uint64), np.zeros(2, np.uint32)
    args = (kind, off.ctypes.data, n, first_slot, k, p, fb.ctypes.data if fb is not None else None, rl.ctypes.data if rl is not None else None)
    rc = host.dshh_sketch_plan(*args, None, counts.ctypes.data, info.ctypes.data)
    if rc:
        return rc, None, info
    lists = [np.zeros(int(c), dt) for dt, c in zip(LISTS[kind], counts)]
    assert not counts[len(lists):].any()
    bufs = (C.c_void_p * 4)(*[a.ctypes.data for a in lists])
    sizes = counts.copy()
    assert host.dshh_sketch_plan(*args, bufs, counts.ctypes.data, info.ctypes.data) == 0 and (counts == sizes).all()
    if lists[0].size:  # a buffer too small is refused
        counts[0] -= 1
        assert host.dshh_sketch_plan(*args, bufs, counts.ctypes.data, info.ctypes.data) == -2
    return 0, lists, info


def subs_rule(p, total_subs):
    cap = 16 if p <= 13 else 64 if p == 14 else 128
    return min(cap, max(16, total_subs // 1024))


def nsubs(b, e):
    return (e - (b & ~31) + SUB - 1) // SUB


def check_items(work, recs, k, per):
    """work: the items of the (begin, end, slot) in recs that have at least k bases, each cut `per` sub-chunks at a time"""
    items = [tuple(int(x) for x in w) for w in work.tolist()]
    at = 0
    for b, e, slot in recs:
        if e - b < k:
            continue
        pos = b & ~31
        while True:
            assert at < len(items), "items missing for [%d, %d)" % (b, e)
            gbeg, gend, start, nsub, s = items[at]
            at += 1
            assert (gbeg, gend, s) == (b, e, slot) and start == pos and start % 32 == 0 and 1 <= nsub <= per
            pos += nsub * SUB
            if pos >= e:
                assert pos - SUB < e, "a sub-chunk behind the genome's end"
                break
            assert nsub == per, "only a genome's last item may be short"
    assert at == len(items), "items nobody asked for"


def check_genomes(off, first_slot, k, p, work):
    o = [int(x) for x in off]
    recs = [(o[g], o[g + 1], first_slot + g) for g in range(len(o) - 1)]
    check_items(work, recs, k, subs_rule(p, sum(nsubs(b, e) for b, e, _ in recs)))


def check_records(off, first_slot, k, p, lists, info):
    runs, segs, zero, work = lists
    o = [int(x) for x in off]
    n = len(o) - 1
    if p > MAX_P_RECORDS:
        assert info[1] == 0 and runs.size == 0 and segs.size == 0 and zero.size == 0
        return check_genomes(off, first_slot, k, p, work)
    assert info[1] == 1
    is_long = [o[r + 1] - (o[r] & ~31) > RUN_SPAN for r in range(n)]
    longs = [(o[r], o[r + 1], first_slot + r) for r in range(n) if is_long[r]]
    assert zero.tolist() == [s for _, _, s in longs]
    check_items(work, longs, k, subs_rule(p, sum(nsubs(b, e) for b, e, _ in longs)))
    segl = segs.tolist()
    r, nseg_seen = 0, 0
    for base, seg0, nseg, slot0, nrec, span, pad in runs.tolist():
        while r < n and is_long[r]:
            r += 1
        assert r < n and slot0 == first_slot + r and nrec >= 1, "a run must start at the next record no run holds yet"
        assert base == o[r] & ~31 and seg0 == nseg_seen and pad == 0
        assert nrec <= RUN_RECS and nseg <= RUN_SEGS and span <= RUN_SPAN and r + nrec <= n
        assert not any(is_long[r:r + nrec]), "a long record inside a run"
        want = [(o[q] - base, q - r) for q in range(r, r + nrec) if o[q + 1] > o[q]]
        assert [tuple(x) for x in segl[seg0:seg0 + nseg]] == want and len(want) == nseg
        assert all(a[0] < b[0] for a, b in zip(want, want[1:]))
        ends = [o[q + 1] - base for q in range(r, r + nrec) if o[q + 1] > o[q]]
        assert span == (ends[-1] if ends else 0) and o[r + nrec] - base <= RUN_SPAN
        nseg_seen += nseg
        r += nrec
        if r < n and not is_long[r]:  # greedy: the next record would have broken a cap
            assert o[r + 1] - base > RUN_SPAN or nrec == RUN_RECS or (o[r + 1] > o[r] and nseg == RUN_SEGS), "run ends early"
    while r < n and is_long[r]:
        r += 1
    assert r == n and nseg_seen == len(segl), "records in no run"


def offsets(lens, lead=0):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64), dtype=np.uint64)
    return off + np.uint64(lead)


def lane_offset_lens():
    """tests/test_gpu_records.py, test_boundaries_on_every_lane_offset"""
    rng = np.random.default_rng(3)
    lens = []
    for o in range(32):
        lens += [32 * int(rng.integers(1, 40)) + o, 31 - o + 32, 8192 - 32 - o, 8192 - 64 + o, o + 1]
    return lens


def mostly_empty_lens():
    """tests/test_gpu_records.py, test_run_record_cap"""
    rng = np.random.default_rng(6)
    lens = np.zeros(10_000, int)
    lens[::97] = rng.integers(1, 60, lens[::97].size)
    lens[5000] = 200
    return lens.tolist()


def around_the_span_lens():
    """records of 8191, 8192 and 8193 bases that start at offset 0, 1 and 31 of a lane, a filler in front of each"""
    lens, pos = [], 0
    for o in (0, 1, 31):
        for L in (8191, 8192, 8193):
            fill = (o - pos) % 32 + 32
            lens += [fill, L]
            pos += fill + L
    return lens


RECORD_INPUTS = {
    "edge": offsets(EDGE),
    "edge_lead13": offsets(EDGE, 13),
    "lane_offsets": offsets(lane_offset_lens()),
    "one_base_x300": offsets([1] * 300, 7),
    "mostly_empty": offsets(mostly_empty_lens()),
    "empty_behind_the_segment_cap": offsets([1] * 256 + [0] * 5 + [1] * 44),  # (empty records join a run that is full of segments)
    "ends_on_the_span": offsets([100, 8092, 7, 8185, 1]),  # (a record may end exactly 8 192 bases behind its run's base)
    "around_the_span": offsets(around_the_span_lens()),
    "empty_call": offsets([]),
}
# every one of 8191 / 8192 / 8193 bases alone, starting at offset 0, 1 and 31 of a lane
for _o in (0, 1, 31):
    for _L in (8191, 8192, 8193):
        RECORD_INPUTS["alone_%d_at_%d" % (_L, _o)] = np.array([64 + _o, 64 + _o + _L], np.uint64)


@pytest.mark.parametrize("p", [10, 13, 14, 15, 17])
@pytest.mark.parametrize("edge", [17 * 1024, 64 * 1024, 128 * 1024])
def test_rule_at_its_thresholds(host, p, edge):
    """total sub-chunks just below and just above where the rule's value moves, from a few huge offsets (the planners never
    read the bases); the items of a call walk exactly the rule's value"""
    for total in (edge - 1, edge, edge + 1):
        parts = [total // 3, 5, total - total // 3 - 5 - 1]  # whole sub-chunks, and one genome of 30 bases: no item, one sub-chunk
        off = offsets([parts[0] * SUB, parts[1] * SUB, parts[2] * SUB, 30], 0)
        assert sum(nsubs(int(off[g]), int(off[g + 1])) for g in range(4)) == total
        rc, (work,), _ = plan(host, 0, off, 3, 31, p)
        assert rc == 0
        per = subs_rule(p, total)
        assert per == (16 if p <= 13 or total < 17 * 1024 else min(total // 1024, 64 if p == 14 else 128))
        check_genomes(off, 3, 31, p, work)
        assert work["nsub"].max() == per and (work["nsub"] == per).sum() >= work.size - 3
        # the long records of a records call follow the same rule, counted over the long records alone
        rc, lists, info = plan(host, 1, off, 3, 31, p)
        assert rc == 0
        check_records(off, 3, 31, p, lists, info)
        assert lists[3]["nsub"].max() == subs_rule(p, total - 1)


@pytest.mark.parametrize("k", [1, 31, 32])
def test_genomes(host, k):
    rng = np.random.default_rng(k)
    lens = [0, 30, 31, 32, 33, 8191, 8192, 8193, 16 * SUB, 16 * SUB + 5, 17 * SUB, 33 * SUB + 123, k - 1, k] + rng.integers(0, 300_000, 20).tolist()
    for lead in (0, 13, 31, 32):
        for p in (10, 14, 18):
            off = offsets(lens, lead)
            rc, (work,), _ = plan(host, 0, off, 2, k, p)
            assert rc == 0
            check_genomes(off, 2, k, p, work)
            short = {2 + g for g, L in enumerate(lens) if L < k}
            assert not short & set(work["slot"].tolist())


@pytest.mark.parametrize("name", sorted(RECORD_INPUTS))
def test_records(host, name):
    off = RECORD_INPUTS[name]
    for k, p, first in ((31, 10, 0), (1, 14, 5), (32, 17, 2), (31, 18, 2), (21, 24, 0)):
        rc, lists, info = plan(host, 1, off, first, k, p)
        assert rc == 0
        check_records(off, first, k, p, lists, info)


def test_record_caps_are_reached(host):
    _, (runs, segs, _, _), _ = plan(host, 1, RECORD_INPUTS["one_base_x300"], 0, 1, 10)
    assert runs["nseg"].tolist() == [256, 44]
    _, (runs, _, _, _), _ = plan(host, 1, RECORD_INPUTS["mostly_empty"], 0, 21, 10)
    assert runs["nrec"].max() == RUN_RECS
    for L, o, want_long in ((8191, 0, False), (8192, 0, False), (8193, 0, True), (8191, 1, False), (8192, 1, True), (8161, 31, False), (8162, 31, True)):
        _, (runs, _, zero, work), _ = plan(host, 1, np.array([64 + o, 64 + o + L], np.uint64), 4, 31, 10)
        if want_long:
            assert zero.tolist() == [4] and runs.size == 0 and work["nsub"].tolist() == [2]
        else:
            assert zero.size == 0 and runs.size == 1 and work.size == 0


def test_refused_arguments(host):
    """The planners take monotone offsets and slots that fit 32 bits (every list keeps a slot in 32 bits).  The hook refuses
    what breaks that with a copy of the two checks of sketch.hip's sketch_enter: it is that copy which is exercised here --
    the library's own 2^32 guard cannot be reached without more than 2^32 rows allocated."""
    assert plan(host, 0, [0, 200, 100, 300])[0] == -1
    assert plan(host, 1, [0, 200, 100, 300])[0] == -1
    assert plan(host, 0, [0, 100], first_slot=0xFFFFFFFF)[0] == -1  # slots are 32-bit in every list
    assert plan(host, 1, [0, 100], first_slot=0xFFFFFFFF)[0] == -1
    assert plan(host, 0, [0, 100], first_slot=0xFFFFFFFE)[0] == 0


def fastx_case(rng, n):
    raw_len = rng.integers(0, 5 * FX_CHUNK, n)
    raw_len[rng.integers(0, n, 3)] = [0, FX_CHUNK, 2 * FX_CHUNK + 1]
    region = (raw_len + rng.integers(0, 100, n) + 31) // 32 * 32
    off = offsets(region, 64)
    first = np.frombuffer(b">@;A", np.uint8)[rng.integers(0, 4, n)]
    return off, raw_len.astype(np.uint64), first


def test_fastx(host):
    rng = np.random.default_rng(8)
    off, raw_len, first = fastx_case(rng, 40)
    rc, (gen, chunks), _ = plan(host, 2, off, first_byte=first, raw_len=raw_len)
    assert rc == 0 and gen.size == 40
    lo = int(off[0])
    at = 0
    for g in range(40):
        b, e, L = int(off[g]) - lo, int(off[g + 1]) - lo, int(raw_len[g])
        want = [(b + x, min(FX_CHUNK, L - x), g) for x in range(0, L, FX_CHUNK)]
        assert tuple(gen[g].tolist()) == (b, L, e, at, len(want), 1 if L and first[g] == ord("@") else 0, 0)
        assert [tuple(c) for c in chunks[at:at + len(want)].tolist()] == want
        at += len(want)
    assert at == chunks.size
    # refusals name the genome: a region that does not start on a multiple of 32 (the first one too), raw bytes beyond it
    for g in (0, 7):
        bad = off.copy()
        bad[g] += np.uint64(1)
        rc, _, info = plan(host, 2, bad, first_byte=first, raw_len=raw_len)
        assert (rc, int(info[0])) == (1, g)
    big = raw_len.copy()
    big[11] = off[12] - off[11] + np.uint64(1)
    rc, _, info = plan(host, 2, off, first_byte=first, raw_len=big)
    assert (rc, int(info[0])) == (1, 11)
    big[11] -= np.uint64(1)
    assert plan(host, 2, off, first_byte=first, raw_len=big)[0] == 0


def golden_cases():
    """name -> arguments of plan(): about a dozen seeded inputs over the three kinds"""
    cases = {}
    for seed, (p, k, first) in enumerate([(10, 31, 0), (14, 21, 3), (15, 32, 1), (18, 31, 2)]):
        rng = np.random.default_rng(100 + seed)
        lens = np.exp(rng.uniform(0, np.log(3_000_000), 60)).astype(np.int64) - 1
        cases["genomes_%d" % seed] = (0, offsets(lens, int(rng.integers(0, 64))), first, k, p)
    cases["genomes_huge_p15"] = (0, offsets([70_000 * SUB + 17, 5, 40_000 * SUB, 31, 30_000 * SUB - 1], 9), 7, 31, 15)
    for seed, (p, k, first) in enumerate([(10, 31, 0), (14, 11, 2), (17, 32, 5), (20, 31, 1)]):
        rng = np.random.default_rng(200 + seed)
        lens = np.exp(rng.uniform(0, np.log(60_000), 3000)).astype(np.int64) - 1
        lens[rng.integers(0, 3000, 600)] = 0
        cases["records_%d" % seed] = (1, offsets(lens, int(rng.integers(0, 64))), first, k, p)
    cases["records_lane_offsets"] = (1, RECORD_INPUTS["lane_offsets"], 2, 31, 10)
    cases["records_mostly_empty"] = (1, RECORD_INPUTS["mostly_empty"], 0, 21, 14)
    cases["records_huge_p14"] = (1, offsets([100, 50_000 * SUB + 3, 0, 8193, 30_000 * SUB], 31), 0, 31, 14)
    for seed in range(2):
        off, raw_len, first = fastx_case(np.random.default_rng(300 + seed), 50)
        cases["fastx_%d" % seed] = (2, off, 0, 31, 10, first, raw_len)
    return cases


def digest(host, args):
    rc, lists, info = plan(host, *args)
    assert rc == 0
    h = hashlib.sha256()
    for a in lists:
        h.update(np.uint64(a.size).tobytes())
        h.update(a.tobytes())
    h.update(info.tobytes())
    return h.hexdigest()


def test_golden_digests(host):
    with open(GOLDEN) as f:
        want = json.load(f)
    cases = golden_cases()
    assert sorted(want) == sorted(cases)
    got = {name: digest(host, args) for name, args in cases.items()}
    assert got == want
