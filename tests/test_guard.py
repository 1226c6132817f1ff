"""CPU: the guard-band helper (tests/guard.py) against stand-in "entry points" -- plain functions that store through a
raw pointer the way a kernel does: one correct, the others with one planted fault each.  The helper's power is proven
here and nowhere else: no kernel is ever altered to write out of range (on the device the detection is shown once, by a
torch write of the test's own into a guard, tests/test_gpu_guard_bands.py)."""
import ctypes as C

import numpy as np
import pytest

import guard
from guard import Guarded, GuardError, guard_items, unwritten


def tri_index(n, i, j):
    return i * (2 * n - i - 1) // 2 + j - (i + 1)


def tri_span(n, rb, re):
    return tri_index(n, re, re + 1) - tri_index(n, rb, rb + 1) if re > rb else 0


def store(ptr, off, value):
    """*(float *)(ptr + 4 off) = value: the store of a kernel, any offset, no bounds"""
    C.c_float.from_address(ptr + 4 * off).value = value


def store_bits(ptr, off, bits):
    C.c_uint32.from_address(ptr + 4 * off).value = bits


def value(i, j):
    return float(i * 1000 + j) + 0.5


def rows_entry_point(ptr, n, rb, re, fault=None):
    """stand-in of dsh_dist_rows_device: rows [rb, re) of the packed triangle of n, relative to `ptr`"""
    base = tri_index(n, rb, rb + 1)
    span = tri_span(n, rb, re)
    skip = tri_index(n, rb, n - 1) - base if fault in ("skip", "span_canary") else -1  # the last value of the first row
    for i in range(rb, re):
        for j in range(i + 1, n):
            off = tri_index(n, i, j) - base
            if off != skip:
                store(ptr, off, value(i, j))
    if fault == "before":
        store(ptr, -1, 1.0)
    elif fault == "behind":
        store(ptr, span, 1.0)
    elif fault == "tile_row_behind":
        store(ptr, span + guard.TILE * n, 1.0)
    elif fault == "full_position":  # the last row's first value at its position in the FULL triangle
        store(ptr, tri_index(n, re - 1, re), value(re - 1, re))
    elif fault == "base_twice":  # ... and the opposite: the base subtracted twice
        store(ptr, -base, value(rb, rb + 1))
    elif fault == "span_canary":  # the span canary's own bit pattern stored as a value
        store_bits(ptr, skip, guard.span_canary(np.float32))
    elif fault is not None and fault != "skip":
        raise AssertionError(fault)
    return span


def reference(n, rb, re):
    return np.array([value(i, j) for i in range(rb, re) for j in range(i + 1, n)], np.float32)


N, RB, RE = 37, 5, 20


def run(fault, misalign=0, n=N, rb=RB, re=RE):
    g = Guarded(tri_span(n, rb, re), np.float32, guard_items(n), guard_items(n), misalign)
    rows_entry_point(g.ptr, n, rb, re, fault)
    return g


@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
@pytest.mark.parametrize("n,rb,re", [(N, RB, RE), (N, 0, N), (N, N - 1, N), (1, 0, 1), (2, 0, 2), (130, 128, 130)])
def test_correct_entry_point_passes_at_every_misalignment(misalign, n, rb, re):
    g = run(None, misalign, n, rb, re)
    assert g.ptr % 16 == 4 * misalign
    g.check()
    assert unwritten(g) == 0 and g.unwritten() == 0
    assert g.host().tobytes() == reference(n, rb, re).tobytes()


@pytest.mark.parametrize("misalign", [0, 3])
@pytest.mark.parametrize("fault,offset", [
    ("before", -1),
    ("behind", tri_span(N, RB, RE)),
    ("tile_row_behind", tri_span(N, RB, RE) + 128 * N),
    ("full_position", tri_index(N, RE - 1, RE)),
    ("base_twice", -tri_index(N, RB, RB + 1)),
])
def test_planted_stores_outside_the_span_are_reported_with_their_offset(fault, offset, misalign):
    span = tri_span(N, RB, RE)
    assert offset < 0 or offset >= span, "the planted store is meant to lie outside the span"
    g = run(fault, misalign)
    with pytest.raises(GuardError) as e:
        g.check(fault)
    assert (e.value.first, e.value.last, e.value.count) == (offset, offset, 1)
    assert fault in str(e.value) and str(offset) in str(e.value)
    assert unwritten(g) == 0 and g.host().tobytes() == reference(N, RB, RE).tobytes()  # the span itself is right


def test_first_last_and_count_of_several_disturbed_elements():
    g = run(None)
    for off in (-7, -2, g.n_items + 3, g.n_items + 900):
        store(g.ptr, off, 0.0)
    with pytest.raises(GuardError) as e:
        g.check()
    assert (e.value.first, e.value.last, e.value.count) == (-7, g.n_items + 900, 4)


def test_a_skipped_element_is_counted_and_the_guards_stay_intact():
    g = run("skip")
    g.check()
    assert unwritten(g) == 1 and unwritten(g.host()) == 1
    got, want = g.host(), reference(N, RB, RE)
    ne = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert ne.tolist() == [tri_index(N, RB, N - 1) - tri_index(N, RB, RB + 1)]


def test_the_canary_as_a_value_inside_the_span():
    """Inside the span a canary is no guard hit.  The span canary's bit pattern stored as a result is what `unwritten`
    reports (no kernel of the library produces that NaN, so it can only be a value that was never computed)."""
    g = run("span_canary")
    g.check()
    assert unwritten(g) == 1
    # the GUARD canary's bit pattern inside the span: not a guard hit either, and a written element
    g = run(None)
    store_bits(g.ptr, 3, guard.guard_canary(np.float32))
    g.check()
    assert unwritten(g) == 0
    assert g.host().tobytes() != reference(N, RB, RE).tobytes()  # (the comparison with the reference is what sees it)


def test_the_canarys_numeric_value_is_not_the_canary():
    """The comparison is one of integers.  The float whose VALUE is the canary's number (2143346349.0) has other bits:
    stored into a guard it is a hit, stored into the span it is a written element."""
    for can in (guard.guard_canary(np.float32), guard.span_canary(np.float32)):
        assert np.float32(can).view(np.uint32) != can
        g = run(None)
        store(g.ptr, 2, float(can))
        g.check()
        assert unwritten(g) == 0
        store(g.ptr, -1, float(can))
        with pytest.raises(GuardError) as e:
            g.check()
        assert (e.value.first, e.value.count) == (-1, 1)
    # NaN != NaN must not hide an intact guard, nor make two NaNs with different payloads equal
    g = run(None)
    store_bits(g.ptr, g.n_items, 0x7FC00000)
    with pytest.raises(GuardError):
        g.check()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint32, np.float32, np.uint64, np.float64])
@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
def test_every_element_type(dtype, misalign):
    isz = np.dtype(dtype).itemsize
    g = Guarded(50, dtype, 40, 33, misalign)
    assert g.ptr % 16 == (misalign * isz) % 16
    assert g.span().dtype == np.dtype(dtype) and g.span().size == 50
    g.check()
    assert unwritten(g) == 50
    assert guard.guard_canary(dtype) != guard.span_canary(dtype)
    g.fill(np.arange(50))
    assert unwritten(g) == 0 and np.array_equal(g.host(), np.arange(50).astype(dtype))
    g.check()
    g.reset()
    assert unwritten(g) == 50
    C.c_uint8.from_address(g.ptr + 50 * isz).value = 0  # one BYTE of the first element behind the span
    with pytest.raises(GuardError) as e:
        g.check()
    assert (e.value.first, e.value.last, e.value.count) == (50, 50, 1)
    g = Guarded(50, dtype, 40, 33, misalign)
    C.c_uint8.from_address(g.ptr - 1).value = 0
    with pytest.raises(GuardError) as e:
        g.check()
    assert (e.value.first, e.value.last, e.value.count) == (-1, -1, 1)


def test_an_empty_span_and_the_default_guard_size():
    assert guard_items(1) == 128 and guard_items(2) == 1 + 256 and guard_items(700) == 700 * 699 // 2 + 128 * 700
    g = Guarded(0, np.float32, guard_items(2), guard_items(2), 1)
    g.check()
    assert unwritten(g) == 0 and g.host().size == 0
    store(g.ptr, 0, 1.0)  # with no span the first element behind the pointer is a guard
    with pytest.raises(GuardError) as e:
        g.check()
    assert (e.value.first, e.value.count) == (0, 1)
    # a full-triangle position of ANY range call of n sketches lies inside guards of the default size, in both directions
    for n in (2, 129, 300):
        total = n * (n - 1) // 2
        assert guard_items(n) >= total + 128 * n and tri_index(n, n - 2, n - 1) < guard_items(n)
