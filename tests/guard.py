"""Guard bands around a caller's buffer (tests/test_gpu_guard_bands.py on the device, tests/test_guard.py for the helper
itself): ONE allocation laid out as

    [front guard | misalign items | span | back guard]

on the device (a torch tensor) or on the host (a numpy array).  The guards hold a canary no kernel of this library can
produce -- a quiet NaN with a payload for floats, 0xDEADBEEF for words, 0xA5 for registers --, the span a second,
different one, so that a store outside the span AND a span element that was never stored are both seen.  Everything is
compared as integers of the element's width: NaN != NaN, and a float that merely has the canary's numeric value is not
the canary.  Plain helper module; no fixtures, importable without a device.

Guard size is the caller's choice; the default, guard_items(n), is the whole packed triangle of the collection plus one
tile row.  A range, part or shard call writes relative to a pointer that stands for a position INSIDE the triangle: a
value stored at its full-triangle position instead of its range-relative one (or the other way round) is then still
inside the allocation, where check() sees it, instead of outside, where it would fault."""
import numpy as np

TILE = 128

# element dtype -> (integer type of the same width, guard canary, span canary)
_CANARIES = {
    "float32": (np.uint32, 0x7FC0DEAD, 0x7FC0C0DE),
    "uint32": (np.uint32, 0xDEADBEEF, 0xC0DEC0DE),
    "uint8": (np.uint8, 0xA5, 0x5A),
    "float64": (np.uint64, 0x7FF8DEADDEADBEEF, 0x7FF8C0DEC0DEC0DE),
    "uint64": (np.uint64, 0xDEADBEEFDEADBEEF, 0xC0DEC0DEC0DEC0DE),
}
ALIGN = 16  # bytes: the boundary `misalign` moves the span off


class GuardError(AssertionError):
    """a guard element was disturbed; first / last: offsets relative to the span (negative: before it, >= n_items:
    behind it), count: how many"""

    def __init__(self, what, first, last, count, n_items):
        super().__init__("%s: %d guard element(s) disturbed, first at span offset %d, last at %d (the span is [0, %d))" % (
            what, count, first, last, n_items))
        self.first, self.last, self.count = first, last, count


def guard_items(n):
    """the default guard: the packed triangle of n sketches plus one tile row, in items"""
    n = int(n)
    return n * (n - 1) // 2 + TILE * n


def guard_canary(dtype):
    return _CANARIES[np.dtype(dtype).name][1]


def span_canary(dtype):
    return _CANARIES[np.dtype(dtype).name][2]


def _signed(value, bits):
    """the two's-complement reading of an unsigned bit pattern (torch has no unsigned 32 / 64-bit arithmetic)"""
    return value - (1 << bits) if value >> (bits - 1) else value


class Guarded:
    """`n_items` elements of `dtype` between guards of `front` and `back` items (default 64), the span `misalign` items
    (0..3) behind a 16-byte boundary.  device=None: host memory (numpy); "pinned": page-locked host memory of the
    library (dsh_alloc_host); else a torch device.

      ptr          address of the span (for the C-ABI)
      span()       a view of the span: numpy array of `dtype`, or torch tensor (float32 / float64 as such, the integer
                   types as torch's signed type of the same width)
      host()       the span as a numpy array of `dtype` (a copy for device memory)
      fill(a)      overwrite the span with the values of `a` (an input buffer)
      check()      raises GuardError unless every guard element still holds the guard canary
      unwritten()  number of span elements that still hold the span canary
    """

    def __init__(self, n_items, dtype=np.float32, front=64, back=64, misalign=0, device=None):
        self.dtype = np.dtype(dtype)
        self.itype, self.gcan, self.scan = _CANARIES[self.dtype.name]
        self.itype = np.dtype(self.itype)
        isz = self.itype.itemsize
        assert 0 <= misalign <= 3 and n_items >= 0 and front >= 0 and back >= 0
        per = max(ALIGN // isz, 1)
        self.n_items = int(n_items)
        self.front = (int(front) + per - 1) // per * per + int(misalign)  # (whole 16-byte units, then the misalignment)
        self.back = int(back)
        self.misalign = int(misalign)
        self.device = device
        total = self.front + self.n_items + self.back
        if device == "pinned":
            import dashing_amd

            self._pin = dashing_amd.PinnedArray(total * isz + ALIGN, np.uint8)
            self.device = device = None
        if device is None:
            raw = self._pin.array if hasattr(self, "_pin") else np.empty(total * isz + ALIGN, np.uint8)
            skip = (-raw.ctypes.data) % ALIGN
            self._raw = raw
            self.buf = raw[skip : skip + total * isz].view(self.itype)
            self.buf[:] = self.gcan
            self.buf[self.front : self.front + self.n_items] = self.scan
            base = self.buf.ctypes.data
        else:
            import torch

            self._torch = torch
            tt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[isz]
            bits = 8 * isz
            g, s = (self.gcan, self.scan) if isz == 1 else (_signed(self.gcan, bits), _signed(self.scan, bits))
            self._g, self._s = g, s
            self.buf = torch.full((max(total, 1),), g, dtype=tt, device=device)
            self.buf[self.front : self.front + self.n_items] = s
            torch.cuda.synchronize()  # torch fills on its own stream, the library writes on the context's
            base = self.buf.data_ptr()
        assert base % ALIGN == 0
        self.ptr = base + self.front * isz
        assert self.ptr % ALIGN == (self.misalign * isz) % ALIGN

    # ---- views
    def _span_int(self):
        return self.buf[self.front : self.front + self.n_items]

    def span(self):
        v = self._span_int()
        if self.device is None:
            return v.view(self.dtype)
        t = self._torch
        return v.view({"float32": t.float32, "float64": t.float64}.get(self.dtype.name, v.dtype))

    def host(self):
        v = self._span_int()
        if self.device is None:
            return v.view(self.dtype)
        self._torch.cuda.synchronize()
        return v.cpu().numpy().view(self.dtype)

    def fill(self, values):
        a = np.ascontiguousarray(values, self.dtype).reshape(-1)
        assert a.size == self.n_items
        if self.device is None:
            self._span_int()[:] = a.view(self.itype)
        elif a.size:
            t = self._torch
            as_torch = {1: np.uint8, 4: np.int32, 8: np.int64}[self.itype.itemsize]
            self._span_int().copy_(t.from_numpy(a.view(as_torch).copy()))
            t.cuda.synchronize()

    def reset(self):
        """the span canary again (the guards are left as they are)"""
        if self.device is None:
            self._span_int()[:] = self.scan
        else:
            self._span_int().fill_(self._s)
            self._torch.cuda.synchronize()

    # ---- the two checks
    def _disturbed(self, lo, hi):
        """indices (into the allocation) of the elements of [lo, hi) that do not hold the guard canary"""
        if hi <= lo:
            return np.zeros(0, np.int64)
        if self.device is None:
            return np.flatnonzero(self.buf[lo:hi] != self.itype.type(self.gcan)).astype(np.int64) + lo
        bad = self._torch.nonzero(self.buf[lo:hi] != self._g).flatten()
        return bad.cpu().numpy().astype(np.int64) + lo

    def check(self, what="guard"):
        if self.device is not None:
            self._torch.cuda.synchronize()
        end = self.front + self.n_items
        bad = np.concatenate([self._disturbed(0, self.front), self._disturbed(end, end + self.back)])
        if bad.size:
            raise GuardError(what, int(bad[0]) - self.front, int(bad[-1]) - self.front, int(bad.size), self.n_items)

    def unwritten(self):
        v = self._span_int()
        if self.device is None:
            return int((v == self.itype.type(self.scan)).sum())
        self._torch.cuda.synchronize()
        return int((v == self._s).sum().item())


def unwritten(span):
    """count of the elements that still hold the span canary: of a Guarded, or of a numpy array taken from one (by its
    dtype).  Every call under test must leave 0."""
    if isinstance(span, Guarded):
        return span.unwritten()
    a = np.ascontiguousarray(span)
    itype, _, scan = _CANARIES[a.dtype.name]
    return int((a.view(itype) == itype(scan)).sum())
