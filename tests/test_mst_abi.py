"""CPU checks of the MST entry points (dsh_mst, dsh_mst_tri, dsh_mst_linkage): declared in a header that is still plain C11,
exported by the library, bound in Python, added without a new ABI version; the definition the header must state; and the
argument errors that need no device."""
import ctypes
import os
import re
import subprocess

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dsh_mst", "dsh_mst_tri", "dsh_mst_linkage"]


def header():
    with open(os.path.join(ROOT, "include", "dashing_hip.h")) as f:
        return f.read()


def test_mst_entry_points_declared_exported_and_bound():
    hdr = header()
    lib = ctypes.CDLL(dashing_amd.lib_path())
    for s in NAMES:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in api.SYMBOLS
    for m in ("mst", "mst_tri"):
        assert callable(getattr(dashing_amd.Context, m))
    assert callable(dashing_amd.mst_linkage)
    assert api.ABI_VERSION == 7 and api.abi_version() == 7  # entry points were only added
    added = hdr[hdr.index("only ADDED") : hdr.index("#define DSH_ABI_VERSION")]
    for s in NAMES:
        assert re.search(r"\b%s\b" % s, added), s


def test_the_header_states_the_definition():
    hdr = header()
    sec = hdr[hdr.index("minimum spanning tree of the pair values") : hdr.index("int dsh_mst(")]
    for phrase in ("lexicographically", "best spanning forest", "prefix", "internal: mst round bound exceeded", "Not built", "mst_rounds",
                   "strict total order", "DSH_ESTATE", "NaN cutoff passes nothing", "threshold_band_bytes"):
        assert phrase in sec, phrase
    linkage = hdr[hdr.index("average-linkage clusters at a threshold") : hdr.index("int dsh_linkage_tri(")]
    assert "dendrogram" in linkage and "dsh_mst" in linkage
    assert '"mst_rounds"' in hdr[hdr.index("int dsh_set_option") : hdr.index("int dsh_get_info")]


def test_a_null_context_is_an_argument_error():
    lib = api.load_library()
    n = ctypes.c_uint64()
    assert lib.dsh_mst(None, 2, 1, 31, 0.5, None, None, None, ctypes.byref(n), None) == -22
    assert lib.dsh_mst_tri(None, 4, None, 0, 0.5, None, None, None, ctypes.byref(n), None) == -22


def test_header_with_the_mst_section_is_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dashing_hip.h"\n'
                   "int main(void) { dsh_ctx *c = 0; uint64_t ne = 0; uint32_t a[1], b[1], s[1], lab[2]; float v[1], tri[1] = {0};\n"
                   "  return dsh_mst(c, 2, 1, 31, 0.5f, a, b, v, &ne, lab) + dsh_mst_tri(c, 2, tri, 0, 0.5f, a, b, v, &ne, 0) +\n"
                   "         dsh_mst_linkage(2, a, b, v, 1, a, b, v, s); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
