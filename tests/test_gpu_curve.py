"""dsh_union_curve* on the device against the numpy model of tests/curve_ref.py: histograms exactly, cardinalities against the
C oracle on the model's running-maximum rows, at the smallest shapes at which each part of the kernels can go wrong
(DESIGN.md 4.18)."""
import functools

import numpy as np
import pytest

import curve_ref
import dashing_amd
from dashing_amd import api, synth
from guard import Guarded

pytestmark = pytest.mark.gpu

D = dashing_amd
DEV = "cuda:0"
N = 24
L = 4  # rows whose loads a lane of k_curve_walk has in flight (kernels.h: kCurveLoadsInFlight)
# one lane owns the row; 16 lanes; one wave; exactly one workgroup; two per order; uint32 counters, 16 and 64 workgroups
PS = (4, 8, 10, 12, 13, 16, 18)
LENS = (1, 2, L, L + 1, 2 * L + 3, 37)
ORDERS = (1, 3, 17)
ESTIMS = (D.ESTIM_ORIGINAL, D.ESTIM_ERTL_IMPROVED, D.ESTIM_ERTL_MLE)


@pytest.fixture(scope="module")
def c1(ctx):  # (the session's context first: it brings torch's runtime up)
    with D.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def c2(ctx):
    with D.Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def rows(p):
    """24 rows: the register law sparse, dense and sparse again, an all-zero row, a saturated one, the rest synthetic"""
    m = 1 << p
    law = [synth.hll_registers(0xF01D + p, m // 64 + 3, p), synth.hll_registers(0xF02D + p, 3 * m, p),
           synth.hll_registers(0xF03D + p, m // 1024 + 1, p)]
    r = np.concatenate([np.stack(law), np.zeros((1, m), np.uint8), np.full((1, m), 64 - p + 1, np.uint8),
                        synth.synthetic_sketches(N - 5, p, seed=100 + p)]).astype(np.uint8)
    assert r.shape == (N, m)
    r.setflags(write=False)
    return r


def make_orders(length, n_orders, seed):
    """identity, reversed, a random permutation, one with repeats (every odd position repeats its predecessor), one slot
    `length` times -- in turn"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n_orders, length), np.uint32)
    for o in range(n_orders):
        kind = o % 5
        if kind == 0:
            v = np.arange(length) % N
        elif kind == 1:
            v = (N - 1 - np.arange(length)) % N
        elif kind == 2:
            v = np.concatenate([rng.permutation(N) for _ in range(length // N + 1)])[:length]
        elif kind == 3:
            v = rng.integers(0, N, length)
            v[1::2] = v[0:-1:2][: v[1::2].size]
        else:
            v = np.full(length, rng.integers(0, N))
        out[o] = v
    return out


_MODEL = {}


def model(regs, p, order, oracle, key=None):
    """(hist uint32 [len][64], {estim: float64 [len]}) of one order, computed once"""
    k = (key if key is not None else p, np.asarray(order, np.uint32).tobytes())
    if k not in _MODEL:
        run = curve_ref.running_max(regs, order)
        hist = np.stack([np.bincount(r, minlength=64) for r in run]).astype(np.uint32) if len(run) else np.zeros((0, 64), np.uint32)
        _MODEL[k] = (hist, {e: oracle.cardinalities(run, e) for e in ESTIMS})
    return _MODEL[k]


def check_against_model(c, regs, p, ords, oracle, key=None, estims=ESTIMS):
    want = [model(regs, p, o, oracle, key) for o in ords]
    want_hist = np.stack([w[0] for w in want])
    for e in estims:
        card, hist = c.union_curve(ords, estim=e, want_hist=True)
        assert hist.dtype == np.uint32 and card.dtype == np.float64
        assert np.array_equal(hist, want_hist)
        assert (hist.sum(axis=2) == 1 << p).all()
        want_card = np.stack([w[1][e] for w in want])
        fin = np.isfinite(want_card)
        assert (np.isfinite(card) == fin).all()
        assert np.allclose(card[fin], want_card[fin], rtol=1e-12, atol=0)
        # equal histograms carry bit-identical doubles
        seen = {}
        for h, v in zip(hist.reshape(-1, 64), card.reshape(-1).view(np.uint64)):
            assert seen.setdefault(h.tobytes(), v) == v
        assert np.array_equal(c.union_curve(ords, estim=e).view(np.uint64), card.view(np.uint64))  # (without the histograms)
    return card, hist


@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("p", PS)
def test_curve_against_the_model(c1, oracle, p, length):
    regs = rows(p)
    c1.set_sketches(regs)
    for n_orders in ORDERS:
        ords = make_orders(length, n_orders, 1000 * p + length)
        check_against_model(c1, regs, p, ords, oracle)
    # a 1-D order gives 1-D results
    card, hist = c1.union_curve(ords[0], want_hist=True)
    assert card.shape == (length,) and hist.shape == (length, 64)
    assert np.array_equal(hist, model(regs, p, ords[0], oracle)[0])


def test_the_last_prefixes_of_permutations_of_all_slots_are_identical(c1, oracle):
    for p in (10, 13):
        regs = rows(p)
        c1.set_sketches(regs)
        ords = D.curve_permutations(N, 6, 77 + p)
        for e in ESTIMS:
            card, hist = c1.union_curve(ords, estim=e, want_hist=True)
            assert (hist[:, -1] == np.bincount(regs.max(axis=0), minlength=64)).all()
            assert len(set(card[:, -1].view(np.uint64).tolist())) == 1
        check_against_model(c1, regs, p, ords, oracle)


def order_bytes(length, p):
    """scratch of one order that is one segment and one scan chunk: deltas and counters (curve_plan.h)"""
    return length * 256 + length * 64 * (2 if p <= 15 else 4)


@pytest.mark.parametrize("p", (10, 13))
def test_segments_and_batches_change_no_byte(c1, p):
    import torch

    regs = rows(p)
    c1.set_sketches(regs)
    length, n_orders = 37, 17
    ords = make_orders(length, n_orders, 5 + p)
    base = {e: c1.union_curve(ords, estim=e, want_hist=True) for e in ESTIMS}
    assert np.array_equal(base[2][1], np.stack([curve_ref.curve_hist(regs, o) for o in ords]))
    d_ord = torch.from_numpy(ords.view(np.int32).copy()).to(DEV)
    d_card = torch.zeros(n_orders * length, dtype=torch.float64, device=DEV)
    d_hist = torch.zeros(n_orders * length * 64, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def same():
        for e in ESTIMS:
            card, hist = c1.union_curve(ords, estim=e, want_hist=True)
            assert card.tobytes() == base[e][0].tobytes() and hist.tobytes() == base[e][1].tobytes()
        assert c1.union_curve(ords).tobytes() == base[2][0].tobytes()
        c1.union_curve_device(d_ord.data_ptr(), length, n_orders, d_card.data_ptr(), d_hist.data_ptr())
        assert d_card.cpu().numpy().tobytes() == base[2][0].tobytes()
        assert d_hist.cpu().numpy().view(np.uint32).tobytes() == base[2][1].tobytes()

    try:
        for seg in (1, 2, 5, 36, 37):
            c1.set_option("curve_segment", seg)
            same()
        for seg in (0, 5):
            c1.set_option("curve_segment", seg)
            nseg = -(-length // seg) if seg else 1
            one = order_bytes(length, p) + ((nseg << p) if nseg > 1 else 0)
            for budget in (3 * one + 5, one, 1):  # batches of three orders, of one, and an order that outgrows the budget
                c1.set_option("curve_scratch_bytes", budget)
                same()
    finally:
        c1.set_option("curve_segment", 0)
        c1.set_option("curve_scratch_bytes", 256 << 20)


@pytest.mark.parametrize("p,n_orders,length", [(4, 17, 11), (10, 3, 37), (13, 3, 5)])
def test_guard_bands(c1, p, n_orders, length):
    import torch

    regs = rows(p)
    c1.set_sketches(regs)
    ords = make_orders(length, n_orders, 31 + p)
    want = np.stack([curve_ref.curve_hist(regs, o) for o in ords])
    g_ord = Guarded(ords.size, np.uint32, device=DEV)
    g_ord.fill(ords)
    try:
        for budget in (256 << 20, 2 * order_bytes(length, p)):  # one batch; several
            c1.set_option("curve_scratch_bytes", budget)
            g_card = Guarded(n_orders * length, np.float64, device=DEV)
            g_hist = Guarded(n_orders * length * 64, np.uint32, device=DEV)
            c1.union_curve_device(g_ord.ptr, length, n_orders, g_card.ptr, g_hist.ptr)
            for g in (g_card, g_hist, g_ord):
                g.check("union_curve_device")
            assert g_card.unwritten() == 0 and g_hist.unwritten() == 0
            assert np.array_equal(g_hist.host().reshape(want.shape), want)
            assert g_card.host().tobytes() == c1.union_curve(ords).tobytes()
            assert g_ord.host().tobytes() == ords.tobytes()  # an input span: read, never written
            # without histograms
            g_card = Guarded(n_orders * length, np.float64, device=DEV)
            c1.union_curve_device(g_ord.ptr, length, n_orders, g_card.ptr)
            g_card.check("union_curve_device, no histograms")
            assert g_card.unwritten() == 0
    finally:
        c1.set_option("curve_scratch_bytes", 256 << 20)
    # nothing to do: nothing is touched
    g_card, g_hist = Guarded(8, np.float64, device=DEV), Guarded(8 * 64, np.uint32, device=DEV)
    c1.union_curve_device(g_ord.ptr, 0, n_orders, g_card.ptr, g_hist.ptr)
    c1.union_curve_device(g_ord.ptr, length, 0, g_card.ptr, g_hist.ptr)
    for g in (g_card, g_hist):
        g.check("empty union_curve_device")
        assert g.unwritten() == g.n_items
    torch.cuda.synchronize()


def raw(c, estim, ords, card, hist, length=None, n_orders=None):
    """dsh_union_curve on the caller's arrays (None: a NULL pointer); returns (code, message)"""
    lib = api.load_library()
    ords2 = None if ords is None else np.ascontiguousarray(ords, np.uint32).reshape(-1 if np.ndim(ords) == 1 else ords.shape[0], -1)
    if n_orders is None:
        n_orders, length = (1, ords2.size) if np.ndim(ords) == 1 else ords2.shape
    rc = lib.dsh_union_curve(c._h, estim, None if ords2 is None else ords2.ctypes.data, length, n_orders,
                             None if card is None else card.ctypes.data, None if hist is None else hist.ctypes.data)
    return rc, lib.dsh_last_error(c._h).decode()


def test_errors(c1, oracle):
    import torch

    p = 10
    regs = rows(p)
    lib = api.load_library()
    ords = make_orders(5, 3, 1)
    card, hist = np.full((3, 5), -7.0), np.full((3, 5, 64), 0xC0DE, np.uint32)

    def untouched():
        return (card == -7.0).all() and (hist == 0xC0DE).all()

    # no resident sketches
    with D.Context(0) as c:
        assert raw(c, 2, ords, card, hist)[0] == -11 and untouched()
        with pytest.raises(D.DshError) as e:
            c.union_curve_device(0, 5, 3, 0)
        assert e.value.code == -11
    c1.set_sketches(regs)
    # a bad estimator, NULL pointers
    for est in (-1, 3):
        assert raw(c1, est, ords, card, hist)[0] == -22 and untouched()
    assert raw(c1, 2, None, card, hist, 5, 3)[0] == -22 and raw(c1, 2, ords, None, hist)[0] == -22 and untouched()
    d_ord = torch.from_numpy(ords.view(np.int32).copy()).to(DEV)
    d_card = torch.zeros(15, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    for a, b in ((0, d_card.data_ptr()), (d_ord.data_ptr(), 0)):
        with pytest.raises(D.DshError) as e:
            c1.union_curve_device(a, 5, 3, b)
        assert e.value.code == -22
    with pytest.raises(D.DshError) as e:
        c1.union_curve_device(d_ord.data_ptr(), 5, 3, d_card.data_ptr(), estim=7)
    assert e.value.code == -22
    # nothing to do
    assert raw(c1, 2, None, None, None, 0, 3)[0] == 0 and raw(c1, 2, None, None, None, 5, 0)[0] == 0
    assert c1.union_curve(np.zeros((3, 0), np.uint32)).shape == (3, 0) and c1.union_curve(np.zeros((0, 5), np.uint32)).shape == (0, 5)
    # an entry >= n: the message names the order and the position
    wrong = ords.copy()
    wrong[1, 2] = N
    wrong[2, 4] = 1 << 31
    rc, msg = raw(c1, 2, wrong, card, hist)
    assert rc == -22 and "order 1" in msg and "position 2" in msg and untouched()
    g_card = Guarded(15, np.float64, device=DEV)
    d_wrong = torch.from_numpy(wrong.view(np.int32).copy()).to(DEV)
    torch.cuda.synchronize()
    with pytest.raises(D.DshError) as e:
        c1.union_curve_device(d_wrong.data_ptr(), 5, 3, g_card.ptr)
    assert e.value.code == -22 and "order 1" in str(e.value) and "position 2" in str(e.value)
    g_card.check("refused device call")
    # a register above the cap: fails only where an order names the sketch, the message names the smallest such slot
    broken = regs.copy()
    broken[6, 77] = 64 - p + 2
    broken[9, 1000] = 200
    broken[20, 5] = 64 - p + 2
    c1.upload(broken)
    clean = np.array([[0, 1, 2, 3, 4], [5, 7, 8, 10, 11], [12, 13, 14, 15, 7]], np.uint32)
    check_against_model(c1, broken, p, clean, oracle, key="broken")
    for named, slot in (([[0, 20, 2, 9, 4], [5, 7, 8, 10, 11], [12, 13, 6, 15, 7]], 6), ([[0, 1, 2, 3, 4]] * 2 + [[20, 20, 9, 20, 9]], 9),
                        ([[0, 1, 2, 3, 20]] * 3, 20)):
        named = np.array(named, np.uint32)
        for budget in (256 << 20, order_bytes(5, p)):  # one batch; three (the histograms wait on the host)
            c1.set_option("curve_scratch_bytes", budget)
            rc, msg = raw(c1, 2, named, card, hist)
            assert rc == -22 and "sketch %d holds a register value above %d" % (slot, 64 - p + 1) in msg and untouched()
            g_card, g_hist = Guarded(15, np.float64, device=DEV), Guarded(15 * 64, np.uint32, device=DEV)
            d_named = torch.from_numpy(named.view(np.int32).copy()).to(DEV)
            torch.cuda.synchronize()
            with pytest.raises(D.DshError) as e:
                c1.union_curve_device(d_named.data_ptr(), 5, 3, g_card.ptr, g_hist.ptr)
            assert e.value.code == -22 and "sketch %d " % slot in str(e.value)
            g_card.check("failed device call")
            g_hist.check("failed device call")
    c1.set_option("curve_scratch_bytes", 256 << 20)
    # the context stays usable
    c1.upload(regs)
    check_against_model(c1, regs, p, ords, oracle)
    assert lib.dsh_set_option(c1._h, b"curve_segment", -1) == -22 and lib.dsh_set_option(c1._h, b"curve_scratch_bytes", 0) == -22


def test_state(c1, c2, oracle):
    import torch

    p = 10
    regs = rows(p)
    c1.set_sketches(regs)
    ords = make_orders(11, 3, 9)
    before = c1.dist_rows()
    info = [c1.info(k) for k in ("planes", "sorted", "ncols")]
    first = check_against_model(c1, regs, p, ords, oracle, estims=(2,))
    assert [c1.info(k) for k in ("planes", "sorted", "ncols")] == info
    assert c1.dist_rows().tobytes() == before.tobytes()
    assert [c1.info(k) for k in ("planes", "sorted", "ncols")] == info
    # an upload between two calls is seen by the second
    changed = regs.copy()
    changed[2] = synth.hll_registers(0xABC, 5000, p)
    c1.upload(changed[2:3], first_slot=2)
    second = check_against_model(c1, changed, p, ords, oracle, key="changed", estims=(2,))
    assert second[1].tobytes() != first[1].tobytes()
    # attached rows give the curve of owned ones
    buf = torch.from_numpy(changed.copy()).to(DEV)
    torch.cuda.synchronize()
    c2.attach_device(buf.data_ptr(), N, p)
    for e in ESTIMS:
        a, b = c1.union_curve(ords, estim=e, want_hist=True), c2.union_curve(ords, estim=e, want_hist=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c2.alloc(1, p)  # (the buffer goes away)
    torch.cuda.synchronize()


def test_a_mid_size_case(c1, oracle):
    """300 x p = 12, five permutations: the planner's own segments (five of 64 members) and three scan chunks per order"""
    n, p = 300, 12
    regs = synth.synthetic_sketches(n, p, seed=12)
    c1.set_sketches(regs)
    ords = D.curve_permutations(n, 5, 2024)
    card, hist = check_against_model(c1, regs, p, ords, oracle, key="mid")
    assert len(set(card[:, -1].view(np.uint64).tolist())) == 1
