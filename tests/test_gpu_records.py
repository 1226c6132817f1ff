"""GPU parity of the per-record sketches (dsh_sketch_records*, k_sketch_records): every record's row BIT-EXACT against
the oracle sketching that record alone -- oracle.sketch_batch(seq, rec_off, ...) with rec_off as genome offsets -- rows
overwritten (not max-merged), neighbouring slots untouched."""
import numpy as np
import pytest

import dashing_amd
from hashinv import revcomp as _revcomp, unwang as _unwang  # (tests/hashinv.py)

pytestmark = pytest.mark.gpu
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def bases(rng, n, dirty=False):
    s = LETTERS[rng.integers(0, 4, n)]
    if dirty and n:
        for _ in range(max(1, n // 3000)):  # N runs and lowercase stretches
            a = int(rng.integers(0, n))
            s[a:a + int(rng.integers(1, 40))] = ord("N")
            b = int(rng.integers(0, n))
            s[b:b + int(rng.integers(1, 200))] |= 0x20
    return s


def records(rng, lens, dirty=False):
    lens = [int(x) for x in lens]
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    return bases(rng, int(off[-1]), dirty), off


def garbage(rng, n, p):
    return rng.integers(0, 64 - p + 2, (n, 1 << p)).astype(np.uint8)


def check(ctx, oracle, seq, off, k, p, canon=True, rng=None, pad=2):
    """slots [pad, pad + n) get the records; the `pad` slots on either side hold random registers that must survive"""
    rng = rng or np.random.default_rng(0)
    n = off.size - 1
    ctx.alloc(n + 2 * pad, p)
    before = garbage(rng, n + 2 * pad, p)
    ctx.upload(before)
    got = ctx.sketch_records(seq, off, pad, k, canon)
    want = oracle.sketch_batch(seq, off, k, p, canon)
    bad = np.argwhere((got != want).any(axis=1)).ravel()
    assert bad.size == 0, "rows differ: records %s (lengths %s), k=%d p=%d canon=%d" % (
        bad[:8].tolist(), [int(off[i + 1] - off[i]) for i in bad[:8]], k, p, canon)
    whole = ctx.download()
    assert (whole[:pad] == before[:pad]).all() and (whole[pad + n:] == before[pad + n:]).all(), "a neighbouring slot changed"
    assert (whole[pad:pad + n] == want).all()
    return want


EDGE = [0, 1, 30, 31, 32, 33, 5, 4, 6, 20, 21, 22, 150, 1000, 8191, 8192, 8193, 0, 0, 2, 64, 65, 63, 7000, 1200]


@pytest.mark.parametrize("k", [1, 5, 21, 31, 32])
@pytest.mark.parametrize("canon", [True, False])
def test_k_and_canon(ctx, oracle, k, canon):
    rng = np.random.default_rng(10 * k + canon)
    lens = EDGE + [k - 1, k, k + 1] + rng.integers(0, 3000, 60).tolist()
    seq, off = records(rng, lens, dirty=True)
    check(ctx, oracle, seq, off, k, 10, canon, rng)


@pytest.mark.parametrize("p", [4, 8, 10, 12, 13, 14, 15, 16, 17, 18, 24])
def test_precisions(ctx, oracle, p):
    rng = np.random.default_rng(p)
    lens = EDGE + rng.integers(0, 20000, 35 if p <= 17 else 6).tolist()
    if p > 17:
        lens += [40_000, 9_000, 31, 0]
    seq, off = records(rng, lens, dirty=True)
    want = check(ctx, oracle, seq, off, 31, p, True, rng)
    assert (want[[i for i, x in enumerate(lens) if x < 31]] == 0).all()


def test_boundaries_on_every_lane_offset(ctx, oracle):
    """record starts on every offset 0 ... 31 of a lane, on the first and the last lane of a run, runs back to back"""
    rng = np.random.default_rng(3)
    lens = []
    for o in range(32):
        lens += [32 * int(rng.integers(1, 40)) + o, 31 - o + 32, 8192 - 32 - o, 8192 - 64 + o, o + 1]
    seq, off = records(rng, lens)
    for k in (31, 32, 12):
        check(ctx, oracle, seq, off, k, 10, True, rng)
    check(ctx, oracle, seq, off, 31, 14, True, rng)


@pytest.mark.parametrize("p", [10, 14])
def test_short_and_long_records_in_one_call(ctx, oracle, p):
    rng = np.random.default_rng(p + 100)
    lens = [150, 1_000_003, 20, 0, 999, 8193, 1_200_000, 33, 64_000, 65_600, 5, 100_000]
    seq, off = records(rng, lens, dirty=True)
    check(ctx, oracle, seq, off, 31, p, True, rng)


def test_tiny_records_many_per_run(ctx, oracle):
    """thousands of records of 0 ... 40 bases: runs cut by the segment and record caps"""
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 41, 12000)
    lens[rng.integers(0, 12000, 3000)] = 0
    seq, off = records(rng, lens)
    for p in (4, 10, 17):
        check(ctx, oracle, seq, off, 11, p, True, rng)


def test_run_record_cap(ctx, oracle):
    """more than 4 096 records in a run's span (mostly empty ones): runs are cut by the record cap as well"""
    rng = np.random.default_rng(6)
    lens = np.zeros(10_000, int)
    lens[::97] = rng.integers(1, 60, lens[::97].size)
    lens[5000] = 200
    seq, off = records(rng, lens)
    for p in (4, 10, 14):
        check(ctx, oracle, seq, off, 21, p, True, rng)


@pytest.mark.parametrize("p", [10, 14])
@pytest.mark.parametrize("canon", [True, False])
def test_kmers_whose_hash_has_32_zero_bits_behind_the_index(ctx, oracle, p, canon):
    """k-mers made through the inverse hash: 32 zero bits behind the index (register values >= 33), planted in short
    records on lane offsets and at the record's first and last k-mer"""
    import oracle.oracle_py as opy

    k = 31
    rng = np.random.default_rng(77 * p + canon)
    made = []
    while len(made) < 10:
        idx, low = int(rng.integers(0, 1 << p)), int(rng.integers(0, 1 << (32 - p)))
        h = (idx << (64 - p)) | low
        x = _unwang(h)
        assert opy.wang(x) == h
        if x >> (2 * k) or (canon and _revcomp(x, k) < x):
            continue
        made.append(x)
    recs = []
    for i, x in enumerate(made):
        txt = LETTERS[[(x >> (2 * (k - 1 - t))) & 3 for t in range(k)]]
        L = int(rng.integers(k, 3000))
        a = bases(rng, L)
        at = [0, L - k, 1, 31, 32, 33 % max(L - k, 1)][i % 5]
        a[at:at + k] = txt
        recs.append(a)
        recs.append(bases(rng, int(rng.integers(0, 200))))
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    want = check(ctx, oracle, np.concatenate(recs), off, k, p, canon, rng)
    assert all((want[2 * i] >= 33).any() for i in range(len(made)))


def test_equivalent_to_one_genome_per_record(ctx, oracle):
    """property, 300 random cases: sketch_records == sketch_batch with one genome per record over cleared slots"""
    rng = np.random.default_rng(11)
    for case in range(300):
        p = int(rng.choice([4, 7, 10, 12, 13, 14, 16, 17]))
        k = int(rng.integers(1, 33))
        canon = bool(rng.integers(0, 2))
        n = int(rng.integers(1, 12))
        lens = np.exp(rng.uniform(0, np.log(20000), n)).astype(int) - 1
        seq, off = records(rng, lens, dirty=bool(case % 2))
        ctx.alloc(n, p)
        ctx.upload(garbage(rng, n, p))
        got = ctx.sketch_records(seq, off, 0, k, canon)
        ctx.clear()
        ref = ctx.sketch_batch(seq, off, 0, k, canon)
        assert (got == ref).all(), (case, p, k, canon, lens.tolist())


def test_fuzz(ctx, oracle):
    """2 000 random cases: lengths log-uniform in [0, 100 kbp], random p, k, strand mode, first slot"""
    rng = np.random.default_rng(12345)
    for case in range(2000):
        p = int(rng.integers(4, 19))
        k = int(rng.integers(1, 33))
        canon = bool(rng.integers(0, 2))
        n = int(rng.integers(1, 9))
        lens = np.exp(rng.uniform(0, np.log(100001), n)).astype(int) - 1
        seq, off = records(rng, lens, dirty=bool(case % 3 == 0))
        # (a random prefix: the call's first record need not start on a multiple of 32)
        lead = int(rng.integers(0, 64))
        seq = np.concatenate([bases(rng, lead), seq])
        off = off + np.uint64(lead)
        first = int(rng.integers(0, 3))
        ctx.alloc(first + n + 1, p)
        before = garbage(rng, first + n + 1, p)
        ctx.upload(before)
        got = ctx.sketch_records(seq, off, first, k, canon)
        want = oracle.sketch_batch(seq, off, k, p, canon)
        assert (got == want).all(), (case, p, k, canon, lead, lens.tolist())
        if case % 50 == 0:
            whole = ctx.download()
            assert (whole[:first] == before[:first]).all() and (whole[first + n:] == before[first + n:]).all()


def test_async_and_device_forms(ctx, oracle):
    import torch

    rng = np.random.default_rng(21)
    lens = EDGE + rng.integers(0, 30000, 40).tolist() + [200_000]
    seq, off = records(rng, lens, dirty=True)
    n, p = len(lens), 12
    want = oracle.sketch_batch(seq, off, 31, p, True)
    ctx.alloc(n, p)
    pin = dashing_amd.PinnedArray(seq.size, np.uint8)
    pin.array[:] = seq
    ctx.upload(garbage(rng, n, p))
    ctx.sketch_records_async(pin.array, off, 0, 31, True)
    ctx.wait()
    assert (ctx.download() == want).all()
    d = torch.zeros(seq.size + 256, dtype=torch.uint8, device="cuda")
    d[: seq.size] = torch.from_numpy(seq).to("cuda")
    torch.cuda.synchronize()
    ctx.upload(garbage(rng, n, p))
    ctx.sketch_records_device(d.data_ptr(), off, 0, 31, True)
    assert (ctx.download() == want).all()
    # a part of the records, to later slots, from the device buffer
    ctx.upload(garbage(rng, n, p))
    ctx.sketch_records_device(d.data_ptr(), off[10:31], 10, 31, True)
    assert (ctx.download(10, 20) == want[10:30]).all()


def test_argument_errors_launch_nothing(ctx):
    rng = np.random.default_rng(31)
    seq, off = records(rng, [100, 200, 300])
    ctx.alloc(5, 10)
    before = garbage(rng, 5, 10)
    ctx.upload(before)
    for args, code in [((seq, off[::-1].copy(), 0, 31), -22),
                       ((seq, off, 0, 0), -22), ((seq, off, 0, 33), -22),
                       ((seq, off, 3, 31), -22), ((seq, off, 6, 31), -22)]:
        with pytest.raises(dashing_amd.DshError) as e:
            ctx.sketch_records(*args)
        assert e.value.code == code
    bad = np.array([0, 200, 100, 300], np.uint64)
    with pytest.raises(dashing_amd.DshError) as e:
        ctx.sketch_records(seq, bad, 0, 31)
    assert e.value.code == -22
    assert (ctx.download() == before).all()
    with dashing_amd.Context(0) as fresh:
        with pytest.raises(dashing_amd.DshError) as e:
            fresh.sketch_records(seq, off, 0, 31)
        assert e.value.code == -11


@pytest.mark.parametrize("p", [10, 14])
def test_distances_and_knn_over_record_sketches(ctx, oracle, p):
    rng = np.random.default_rng(41 + p)
    # related records: mutated copies of a few templates, plus short and empty ones
    temps = [bases(rng, 4000) for _ in range(5)]
    recs = []
    for i in range(120):
        a = temps[i % 5].copy()
        m = rng.integers(0, a.size, int(rng.integers(0, 400)))
        a[m] = LETTERS[rng.integers(0, 4, m.size)]
        recs.append(a[: int(rng.integers(10, a.size))])
    recs[7] = recs[7][:0]
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    seq = np.concatenate(recs)
    ctx.alloc(len(recs), p)
    regs = ctx.sketch_records(seq, off, 0, 21, True)
    want = oracle.sketch_batch(seq, off, 21, p, True)
    assert (regs == want).all()
    for rt in (dashing_amd.JI, dashing_amd.MASH_DIST):
        got = ctx.dist_rows(result_type=rt, k=21)
        ref = oracle.dist_tri(want, oracle.ERTL_MLE, rt, 21)
        assert np.allclose(got, ref, rtol=1e-6, atol=1e-15, equal_nan=True)
    wi, wv = oracle.knn(want, 5, result_type=dashing_amd.JI, k=21)
    gi, gv = ctx.knn(5, result_type=dashing_amd.JI, k=21)
    assert (gi == wi).all() and np.allclose(gv, wv, rtol=1e-6, atol=1e-12, equal_nan=True)
