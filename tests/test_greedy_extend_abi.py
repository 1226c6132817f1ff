"""CPU checks of dsh_greedy_extend and dsh_greedy_extend_device: declared in a header that is still plain C11, exported by
the library, bound in Python, added without a new ABI version; and the argument errors that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dsh_greedy_extend", "dsh_greedy_extend_device"]


def test_extend_entry_points_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dashing_hip.h")) as f:
        hdr = f.read()
    lib = ctypes.CDLL(dashing_amd.lib_path())
    for s in NAMES:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in api.SYMBOLS
        assert getattr(api.load_library(), s).argtypes is not None, s
    for m in ("greedy_extend", "greedy_extend_device"):
        assert callable(getattr(dashing_amd.Context, m))
    assert api.ABI_VERSION == 7 and api.abi_version() == 7  # entry points were only added
    added = hdr[hdr.index("only ADDED") : hdr.index("#define DSH_ABI_VERSION")]
    for s in NAMES:
        assert s in added, s
    assert re.search(r"#define DSH_GREEDY_FIRST 0\b", hdr) and re.search(r"#define DSH_GREEDY_BEST 1\b", hdr)
    assert (dashing_amd.GREEDY_FIRST, dashing_amd.GREEDY_BEST) == (0, 1)
    # the older entry points are still there, unchanged
    for s in ("dsh_greedy_threshold", "dsh_greedy_threshold_device"):
        assert re.search(r"\bint %s\(dsh_ctx \*ctx, int estim, int result_type, int k, float threshold," % s, hdr), s


def test_a_null_context_is_an_argument_error():
    lib = api.load_library()
    n = ctypes.c_uint64()
    lab = np.zeros(4, np.uint32)
    for mode in (0, 1, 7):
        assert lib.dsh_greedy_extend(None, 2, 1, 31, 0.5, mode, 0, None, lab.ctypes.data, ctypes.byref(n)) == -22
        assert lib.dsh_greedy_extend_device(None, 2, 1, 31, 0.5, mode, 0, None, None, ctypes.byref(n)) == -22
        assert lib.dsh_greedy_extend(None, 2, 1, 31, 0.5, mode, 4, lab.ctypes.data, lab.ctypes.data, ctypes.byref(n)) == -22


def test_the_binding_refuses_what_it_can_see():
    ex = dashing_amd.Context._extend_args
    assert ex(0, None, "first")[0] == 0 and ex(0, None, "best")[0] == 1 and ex(0, None, 1)[0] == 1
    for bad in ("nearest", 2, None, True):
        with pytest.raises(ValueError):
            ex(0, None, bad)
    with pytest.raises(ValueError):
        ex(3, [0, 0], "first")  # one label per old slot
    with pytest.raises(ValueError):
        ex(-1, None, "first")
    mode, li, ptr = ex(3, [0, 0, 2], "best")
    assert li.dtype == np.uint32 and li.tolist() == [0, 0, 2] and ptr == li.ctypes.data


def test_header_with_the_extend_section_is_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dashing_hip.h"\n'
                   "int main(void) { dsh_ctx *c = 0; uint64_t nr = 0; uint32_t lab[2]; const uint32_t in[1] = {0};\n"
                   "  return dsh_greedy_extend(c, 2, 1, 31, 0.5f, DSH_GREEDY_BEST, 1, in, lab, &nr)\n"
                   "       + dsh_greedy_extend_device(c, 2, 1, 31, 0.5f, DSH_GREEDY_FIRST, 0, 0, 0, &nr); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
