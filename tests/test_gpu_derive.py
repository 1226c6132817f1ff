"""GPU: derived sketches -- dsh_fold*, dsh_upload_sketches_folded*, dsh_union_groups*  against the numpy
model of tests/derive_ref.py, bit for bit.  Shapes are small and chosen to cross every reduction boundary of k_fold (d = 1;
d = 4, one lane; d = 5, just past a lane; d = 10 / 11, around the 1 KiB of a wave; d = 13, past one pass of a workgroup;
d = 20 with a 16 MiB row) and of the union (groups up to one chunk, groups cut into chunks once and twice)."""
import functools

import numpy as np
import pytest

import dashing_amd
import derive_ref
from dashing_amd import synth
from guard import Guarded

pytestmark = pytest.mark.gpu

D = dashing_amd
DEV = "cuda:0"
FOLDS = [(5, 4), (10, 9), (10, 6), (12, 7), (14, 4), (14, 3 + 1), (15, 4), (17, 4), (24, 4)]
UNION_PS = (4, 10, 14, 18)


@pytest.fixture(scope="module")
def c1(ctx):  # (the session's context first: it brings torch's runtime up)
    with D.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def c2(ctx):
    with D.Context(0) as c:
        yield c


class ByteGuarded(Guarded):
    """a Guarded uint8 device span any number of bytes (0..15) behind a 16-byte boundary"""

    def __init__(self, n_items, misalign, guard=256):
        super().__init__(n_items, np.uint8, guard, guard + 16, 0, DEV)
        self.front += misalign
        self.back -= misalign
        self.ptr += misalign
        self.misalign = misalign
        self.buf.fill_(self._g)
        self.buf[self.front : self.front + self.n_items] = self._s
        self._torch.cuda.synchronize()
        assert self.ptr % 16 == misalign


@functools.lru_cache(maxsize=None)
def law_rows(p):
    """three rows of the register law: sparse, dense, sparse again"""
    m = 1 << p
    rows = np.stack([synth.hll_registers(0xF01D + p, m // 64 + 3, p), synth.hll_registers(0xF02D + p, 3 * m, p),
                     synth.hll_registers(0xF03D + p, m // 1024 + 1, p)])
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def planted_rows(p, new_p):
    """an all-zero row; non-empty registers only where low == 0, one of them at the cap; only where low == 2^d - 1"""
    m, d = 1 << p, p - new_p
    rows = np.zeros((3, m), np.uint8)
    rng = np.random.default_rng(p * 100 + new_p)
    runs = rng.choice(1 << new_p, max((1 << new_p) // 2, 2), replace=False)
    rows[1, runs << d] = rng.integers(1, 64 - p + 1, runs.size)
    rows[1, runs[0] << d] = 64 - p + 1
    rows[2, (runs << d) + (1 << d) - 1] = rng.integers(1, 64 - p + 2, runs.size)
    rows.setflags(write=False)
    return rows, int(runs[0])


@functools.lru_cache(maxsize=None)
def model_fold(kind, p, new_p):
    return derive_ref.fold(law_rows(p) if kind == "law" else planted_rows(p, new_p)[0], new_p)


def dev_u8(n):
    import torch

    return torch.full((max(n, 1),), 0x5A, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("p,new_p", FOLDS)
def test_fold_against_the_model(c1, p, new_p):
    import torch

    c1.set_sketches(law_rows(p))
    want = model_fold("law", p, new_p)
    assert (c1.fold(new_p) == want).all()
    assert (c1.fold(new_p, first_slot=1, n=2) == want[1:]).all()
    rows, cap_run = planted_rows(p, new_p)
    c1.upload(rows)
    want = model_fold("planted", p, new_p)
    assert not want[0].any() and want[1, cap_run] == 64 - new_p + 1
    out = dev_u8(3 << new_p)
    c1.fold_device(out.data_ptr(), new_p)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().reshape(3, -1) == want).all()


@pytest.mark.parametrize("p,new_p", [(14, 10), (12, 8)])
def test_fold_against_sketching(c1, c2, p, new_p):
    seq = np.frombuffer(b"ACGT", np.uint8)[(synth.splitmix64(0xACE + p, 20000) & np.uint64(3)).astype(np.int64)]
    off = np.array([0, seq.size], np.uint64)
    c1.alloc(1, p)
    c1.sketch_batch(seq, off, 0, 31, True)
    c2.alloc(1, new_p)
    want = c2.sketch_batch(seq, off, 0, 31, True)
    assert want.any() and (c1.fold(new_p) == want).all()


def test_folded_upload(c1, c2):
    rng = np.random.default_rng(7)
    base = rng.integers(0, 20, (16, 1 << 10)).astype(np.uint8)
    src = np.stack([synth.hll_registers(0xAB0 + i, 900 * (i + 1), 14) for i in range(6)])
    want = base.copy()
    want[5:11] = derive_ref.fold(src, 10)
    c2.set_sketches(want)
    ref = c2.dist_rows()
    c1.set_sketches(base)
    before = c1.dist_rows()  # (derived state of the old rows exists now)
    c1.upload_folded(src, first_slot=5)
    assert (c1.download() == want).all()  # the range holds the model's rows, the slots outside it are unchanged
    got = c1.dist_rows()
    assert got.tobytes() == ref.tobytes() and got.tobytes() != before.tobytes()  # the old derived state was dropped
    # src_p == p is plain upload
    c1.upload_folded(base[2:9], src_p=10, first_slot=2)
    want[2:9] = base[2:9]
    assert (c1.download() == want).all()
    # the chunk loop of the host form: one source row per chunk
    c1.set_option("derive_chunk_bytes", 1 << 14)
    try:
        c1.upload_folded(src[3:6], first_slot=0)
    finally:
        c1.set_option("derive_chunk_bytes", 256 << 20)
    want[0:3] = derive_ref.fold(src[3:6], 10)
    assert (c1.download() == want).all()
    c1.set_option("derive_chunk_bytes", 1)  # (at least one row)
    try:
        assert (c1.fold(4) == derive_ref.fold(want, 4)).all()
    finally:
        c1.set_option("derive_chunk_bytes", 256 << 20)


@functools.lru_cache(maxsize=None)
def union_rows(p):
    rows = synth.synthetic_sketches(40, p, seed=0xD0 + p, card_lo=(1 << p) // 4 + 50, card_hi=(1 << p) * 4 + 100)
    rows[7] = 0
    rows.setflags(write=False)
    return rows


def csr(groups):
    gp = np.zeros(len(groups) + 1, np.uint64)
    gp[1:] = np.cumsum([len(g) for g in groups])
    return gp, np.array([s for g in groups for s in g], np.uint32)


GROUPS = [[], [3], [5, 17], list(range(40)), [8, 8, 2, 8], [17, 39], [], [39]]


@pytest.mark.parametrize("p", UNION_PS)
def test_union_against_numpy(c1, p):
    rows = union_rows(p).copy()
    rows[9, ::3] = 255  # union does not judge registers
    c1.set_sketches(rows)
    gp, mem = csr(GROUPS)
    got = c1.union_groups(gp, mem)
    assert (got == derive_ref.union_groups(rows, gp, mem)).all()
    assert not got[0].any() and (got[3] == np.maximum.reduce(rows, axis=0)).all()
    gp, mem = csr([[s] for s in range(40)])
    assert (c1.union_groups(gp, mem) == c1.download()).all()
    # a group_ptr that does not start at 0
    gp, mem = csr(GROUPS)
    assert (c1.union_groups(gp[2:], mem) == derive_ref.union_groups(rows, gp, mem)[2:]).all()


@pytest.mark.parametrize("p", (4, 10))
def test_union_of_groups_cut_into_chunks(c1, p):
    """more than 64 members: partial unions, then a union of those; 5000 members: twice"""
    rows = union_rows(p)
    c1.set_sketches(rows)
    rng = np.random.default_rng(p)
    groups = [[1], list(rng.integers(0, 20, 150)), [], list(rng.integers(20, 40, 5000)), list(range(40)), list(rng.integers(0, 40, 65))]
    gp, mem = csr(groups)
    assert (c1.union_groups(gp, mem) == derive_ref.union_groups(rows, gp, mem)).all()


def test_fold_and_union_commute_and_unions_attach(c1, c2, oracle):
    import torch

    rows = union_rows(14)
    gp, mem = csr(GROUPS)
    c1.set_sketches(rows)
    uni = c1.union_groups(gp, mem)
    folded = c1.fold(10)
    c2.set_sketches(uni)
    a = c2.fold(10)
    c2.set_sketches(folded)
    b = c2.union_groups(gp, mem)
    assert (a == b).all()
    # a union buffer on the device is a sketch matrix: attach it to a second context
    buf = dev_u8(len(GROUPS) << 14)
    c1.union_groups_device(buf.data_ptr(), gp, mem)
    c2.attach_device(buf.data_ptr(), len(GROUPS), 14)
    want = oracle.cardinalities(derive_ref.union_groups(rows, gp, mem))
    np.testing.assert_allclose(c2.cardinalities(), want, rtol=1e-12)
    c2.alloc(1, 10)  # (the buffer goes away)
    torch.cuda.synchronize()


def test_derived_state_is_not_touched(c1):
    c1.set_sketches(union_rows(10))
    before = c1.dist_rows()
    info = [c1.info(k) for k in ("planes", "sorted", "ncols")]
    gp, mem = csr(GROUPS)
    o1, o2 = dev_u8(40 << 6), dev_u8(len(GROUPS) << 10)
    c1.fold_device(o1.data_ptr(), 6)
    c1.union_groups_device(o2.data_ptr(), gp, mem)
    assert [c1.info(k) for k in ("planes", "sorted", "ncols")] == info
    assert c1.dist_rows().tobytes() == before.tobytes()
    assert [c1.info(k) for k in ("planes", "sorted", "ncols")] == info


@pytest.mark.parametrize("mis", (0, 1, 15))
def test_guard_bands(c1, mis):
    rows = law_rows(12)
    c1.set_sketches(rows)
    for new_p in (12, 9, 4):  # copy, wave reduction, lane reduction
        g = ByteGuarded(3 << new_p, mis)
        c1.fold_device(g.ptr, new_p)
        g.check("fold_device %d" % new_p)
        assert g.unwritten() == 0
        assert (g.host().reshape(3, -1) == derive_ref.fold(rows, new_p)).all()
    c1.set_sketches(np.maximum(rows, 1))  # (no byte of a union equals the span canary by accident: all below 0x5A)
    gp, mem = csr([[0], [0, 1, 2], [2, 2]])
    g = ByteGuarded(3 << 12, mis)
    c1.union_groups_device(g.ptr, gp, mem)
    g.check("union_groups_device")
    assert g.unwritten() == 0
    assert (g.host().reshape(3, -1) == derive_ref.union_groups(np.maximum(rows, 1), gp, mem)).all()
    # an input span: read, never written
    src = law_rows(14)
    g = ByteGuarded(3 << 14, mis)
    g.fill(src)
    c1.alloc(5, 10)
    c1.upload_folded_device(g.ptr, 14, 3, first_slot=1)
    g.check("upload_folded_device")
    assert g.host().tobytes() == src.tobytes()
    want = np.zeros((5, 1 << 10), np.uint8)
    want[1:4] = derive_ref.fold(src, 10)
    assert (c1.download() == want).all()


def test_errors(c1, c2):
    rows = law_rows(10)
    with D.Context(0) as c:
        gp, mem = csr([[0]])
        for call in (lambda: c.fold(4, 0, 0), lambda: c.union_groups(gp, mem), lambda: c.upload_folded(rows, first_slot=0)):
            with pytest.raises(D.DshError) as e:
                call()
            assert e.value.code == -11
    c1.set_sketches(rows)
    buf = dev_u8(3 << 10)
    bad = [lambda: c1.fold(3), lambda: c1.fold(11), lambda: c1.fold(8, 2, 2), lambda: c1.fold(8, 4, 0),
           lambda: c1.fold_device(buf.data_ptr(), 11), lambda: c1.fold_device(buf.data_ptr(), 8, 1, 3),
           lambda: c1.upload_folded(law_rows(5)), lambda: c1.upload_folded(rows, first_slot=1),
           lambda: c1.upload_folded_device(buf.data_ptr(), 9, 1), lambda: c1.upload_folded_device(buf.data_ptr(), 25, 1),
           lambda: c1.upload_folded_device(buf.data_ptr(), 10, 2, first_slot=2),
           lambda: c1.union_groups(np.array([0, 2, 1], np.uint64), np.array([0, 1], np.uint32)),
           lambda: c1.union_groups(np.array([0, 2], np.uint64), np.array([0, 3], np.uint32)),
           lambda: c1.union_groups_device(buf.data_ptr(), np.array([0, 1], np.uint64), np.array([1 << 31], np.uint32))]
    for call in bad:
        with pytest.raises(D.DshError) as e:
            call()
        assert e.value.code == -22
    assert (c1.download() == rows).all()  # nothing was enqueued
    # the folded upload needs a matrix of the context's own
    c2.attach_device(buf.data_ptr(), 3, 10)
    with pytest.raises(D.DshError) as e:
        c2.upload_folded(rows)
    assert e.value.code == -11
    c2.alloc(1, 10)
    # empty calls
    assert c1.fold(6, 3, 0).shape == (0, 64) and c1.union_groups(np.zeros(1, np.uint64), np.zeros(0, np.uint32)).shape == (0, 1 << 10)
    c1.fold_device(0, 6, 0, 0)
    c1.union_groups_device(0, np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    c1.upload_folded(np.zeros((0, 1 << 12), np.uint8))
    c1.upload_folded_device(0, 12, 0)
    # a register above the cap: values planted by upload, the message names the slot, the context stays usable
    broken = rows.copy()
    broken[2, 77] = 64 - 10 + 2
    c1.upload(broken)
    for call in (lambda: c1.fold(6), lambda: c1.fold_device(buf.data_ptr(), 10)):
        with pytest.raises(D.DshError) as e:
            call()
        assert e.value.code == -22 and "sketch 2 " in str(e.value)
    assert (c1.fold(6, 0, 2) == derive_ref.fold(rows[:2], 6)).all()  # rows no call names are not judged
    c2.alloc(4, 8)
    with pytest.raises(D.DshError) as e:
        c2.upload_folded(broken, first_slot=1)
    assert e.value.code == -22 and "sketch 3 " in str(e.value)
    c2.upload_folded(rows, first_slot=1)
    want = np.zeros((4, 1 << 8), np.uint8)
    want[1:] = derive_ref.fold(rows, 8)
    assert (c2.download() == want).all()
    assert c1.union_groups(*csr([[2]]))[0, 77] == 64 - 10 + 2  # union does not judge
