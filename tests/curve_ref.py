"""The model of the union growth curve (dsh_union_curve*): plain numpy, no device.  Helper module of
tests/test_curve_ref.py, tests/test_gpu_curve.py and tests/test_gpu_cli_curve.py."""
import numpy as np

BINS = 64
_M64 = (1 << 64) - 1


def running_max(regs, order):
    """uint8 [len][2^p]: row i = the registers of the union of the sketches order[0 .. i]"""
    order = np.asarray(order, np.int64).reshape(-1)
    if order.size == 0:
        return np.zeros((0, regs.shape[1]), np.uint8)
    return np.maximum.accumulate(regs[order], axis=0)


def curve_hist(regs, order):
    """uint32 [len][64]: bin v of row i = the number of registers of the union of order[0 .. i] that hold v"""
    rows = running_max(regs, order)
    out = np.zeros((rows.shape[0], BINS), np.uint32)
    for i, row in enumerate(rows):
        out[i] = np.bincount(row, minlength=BINS)
    return out


def _next(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return x, z ^ (z >> 31)


def permutations(n, n_perm, seed):
    """uint32 [n_perm][n]: permutation r is Fisher-Yates from the identity, drawn from splitmix64 started at seed + r"""
    out = np.zeros((n_perm, n), np.uint32)
    for r in range(n_perm):
        row = list(range(n))
        x = (seed + r) & _M64
        for i in range(n - 1, 0, -1):
            x, z = _next(x)
            j = z % (i + 1)
            row[i], row[j] = row[j], row[i]
        out[r] = row
    return out
