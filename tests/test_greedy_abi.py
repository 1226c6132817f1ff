"""CPU checks of the greedy entry points (dsh_greedy_threshold, dsh_greedy_threshold_device): declared in a header that is
still plain C11, exported by the library, bound in Python, added without a new ABI version; and the argument errors that
need no device."""
import ctypes
import os
import re
import subprocess

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dsh_greedy_threshold", "dsh_greedy_threshold_device"]


def test_greedy_entry_points_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dashing_hip.h")) as f:
        hdr = f.read()
    lib = ctypes.CDLL(dashing_amd.lib_path())
    for s in NAMES:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in api.SYMBOLS
    for m in ("greedy_threshold", "greedy_threshold_device"):
        assert callable(getattr(dashing_amd.Context, m))
    assert api.ABI_VERSION == 7 and api.abi_version() == 7  # entry points were only added
    added = hdr[hdr.index("only ADDED") : hdr.index("#define DSH_ABI_VERSION")]
    for s in NAMES:
        assert s in added, s
    assert '"greedy_band_rows"' in hdr  # the option is documented in the option list


def test_a_null_context_is_an_argument_error():
    lib = api.load_library()
    n = ctypes.c_uint64()
    assert lib.dsh_greedy_threshold(None, 2, 1, 31, 0.5, None, ctypes.byref(n)) == -22
    assert lib.dsh_greedy_threshold_device(None, 2, 1, 31, 0.5, None, ctypes.byref(n)) == -22


def test_header_with_the_greedy_section_is_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dashing_hip.h"\n'
                   "int main(void) { dsh_ctx *c = 0; uint64_t nr = 0; uint32_t lab[1];\n"
                   "  return dsh_greedy_threshold(c, 2, 1, 31, 0.5f, lab, &nr) + dsh_greedy_threshold_device(c, 2, 1, 31, 0.5f, 0, &nr); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
