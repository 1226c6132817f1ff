"""CPU checks of the density-cluster entry points (dsh_dbscan_threshold*, dsh_dbscan_tri, dsh_degree_threshold*): declared in a
header that is still plain C11, exported by the library, bound in Python, added without a new ABI version; and the argument
errors that need no device."""
import ctypes
import os
import re
import subprocess

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dsh_dbscan_threshold", "dsh_dbscan_threshold_device", "dsh_dbscan_tri", "dsh_degree_threshold", "dsh_degree_threshold_device"]


def test_dbscan_entry_points_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dashing_hip.h")) as f:
        hdr = f.read()
    lib = ctypes.CDLL(dashing_amd.lib_path())
    for s in NAMES:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in api.SYMBOLS
    for m in ("dbscan_threshold", "dbscan_threshold_device", "dbscan_tri", "degree_threshold", "degree_threshold_device"):
        assert callable(getattr(dashing_amd.Context, m))
    assert api.ABI_VERSION == 7 and api.abi_version() == 7  # entry points were only added
    added = hdr[hdr.index("only ADDED") : hdr.index("#define DSH_ABI_VERSION")]
    for s in NAMES:
        assert s in added, s
    # the kinds; the assignment rules are the two constants of dsh_greedy_extend, not new ones
    for name, value in (("DSH_DBSCAN_NOISE", 0), ("DSH_DBSCAN_BORDER", 1), ("DSH_DBSCAN_CORE", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    assert (dashing_amd.DBSCAN_NOISE, dashing_amd.DBSCAN_BORDER, dashing_amd.DBSCAN_CORE) == (0, 1, 2)
    assert len(re.findall(r"#define DSH_GREEDY_(FIRST|BEST)\b", hdr)) == 2 and "DSH_DBSCAN_FIRST" not in hdr


def test_a_null_context_is_an_argument_error():
    lib = api.load_library()
    nc, nn = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.dsh_dbscan_threshold(None, 2, 1, 31, 0.5, 3, 0, None, None, None, ctypes.byref(nc), ctypes.byref(nn)) == -22
    assert lib.dsh_dbscan_threshold_device(None, 2, 1, 31, 0.5, 3, 0, None, None, None, ctypes.byref(nc), ctypes.byref(nn)) == -22
    assert lib.dsh_dbscan_tri(None, 4, None, 1, 0.5, 3, 0, None, None, None, ctypes.byref(nc), ctypes.byref(nn)) == -22
    assert lib.dsh_degree_threshold(None, 2, 1, 31, 0.5, None) == -22
    assert lib.dsh_degree_threshold_device(None, 2, 1, 31, 0.5, None) == -22


def test_the_binding_refuses_what_it_can_see():
    import pytest

    for bad in ("nearest", 2, True, None):
        with pytest.raises(ValueError):
            dashing_amd.Context._dbscan_args(3, bad)
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError):
            dashing_amd.Context._dbscan_args(bad, "first")
    assert dashing_amd.Context._dbscan_args(5, "best") == (5, api.GREEDY_BEST)
    assert dashing_amd.Context._dbscan_args(1, 0) == (1, api.GREEDY_FIRST)


def test_header_with_the_dbscan_section_is_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dashing_hip.h"\n'
                   "int main(void) { dsh_ctx *c = 0; uint64_t nc = 0, nn = 0; uint32_t lab[1], deg[1]; uint8_t kind[1]; float tri[1] = {0};\n"
                   "  return dsh_dbscan_threshold(c, 2, 1, 31, 0.5f, 3, DSH_GREEDY_FIRST, lab, kind, deg, &nc, &nn) +\n"
                   "         dsh_dbscan_threshold_device(c, 2, 1, 31, 0.5f, 3, DSH_GREEDY_BEST, 0, 0, 0, &nc, 0) +\n"
                   "         dsh_dbscan_tri(c, 2, tri, 1, 0.5f, 3, DSH_GREEDY_BEST, lab, 0, 0, &nc, &nn) +\n"
                   "         dsh_degree_threshold(c, 2, 1, 31, 0.5f, deg) + dsh_degree_threshold_device(c, 2, 1, 31, 0.5f, 0) +\n"
                   "         DSH_DBSCAN_NOISE + DSH_DBSCAN_BORDER + DSH_DBSCAN_CORE; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
