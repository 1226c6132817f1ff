"""CPU checks of the linkage entry points (dsh_linkage_threshold*, dsh_linkage_tri): declared in a header that is still plain
C11, exported by the library, bound in Python, added without a new ABI version; the contract the header must state; and the
argument errors that need no device."""
import ctypes
import os
import re
import subprocess

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dsh_linkage_threshold", "dsh_linkage_threshold_device", "dsh_linkage_tri"]


def header():
    with open(os.path.join(ROOT, "include", "dashing_hip.h")) as f:
        return f.read()


def test_linkage_entry_points_declared_exported_and_bound():
    hdr = header()
    lib = ctypes.CDLL(dashing_amd.lib_path())
    for s in NAMES:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in api.SYMBOLS
    for m in ("linkage_threshold", "linkage_threshold_device", "linkage_tri"):
        assert callable(getattr(dashing_amd.Context, m))
    assert api.ABI_VERSION == 7 and api.abi_version() == 7  # entry points were only added
    added = hdr[hdr.index("only ADDED") : hdr.index("#define DSH_ABI_VERSION")]
    for s in NAMES:
        assert s in added, s
    for name, val in (("SINGLE", 0), ("COMPLETE", 1), ("AVERAGE", 2)):
        assert re.search(r"#define DSH_LINKAGE_%s %d\b" % (name, val), hdr)
        assert getattr(dashing_amd, "LINKAGE_" + name) == val


def test_the_header_states_the_contract():
    hdr = header()
    sec = hdr[hdr.index("average-linkage clusters at a threshold") : hdr.index("int dsh_linkage_tri(")]
    for phrase in ("within 2^-31 of t may be judged equal to t", "lexicographically smallest", "128-bit integers",
                   "internal: linkage step bound exceeded", "DSH_ENOMEM", "linkage_budget_bytes", "linkage_route",
                   "linkage_partition", "linkage_lds_max", "Not built", "dendrogram", "Ward"):
        assert phrase in sec, phrase
    cluster = hdr[hdr.index("clusters at a threshold: connected components") : hdr.index("int dsh_cluster_threshold(")]
    assert "linkages other than single" not in cluster
    opts = hdr[hdr.index("Options; returns") : hdr.index("int dsh_set_option")]
    for o in ("linkage_budget_bytes", "linkage_route", "linkage_partition", "linkage_lds_max"):
        assert '"%s"' % o in opts, o
    assert '"linkage_route"' in hdr[hdr.index("int dsh_set_option") : hdr.index("int dsh_get_info")]


def test_a_null_context_is_an_argument_error():
    lib = api.load_library()
    n = ctypes.c_uint64()
    assert lib.dsh_linkage_threshold(None, 2, 1, 31, 0.5, 1, None, ctypes.byref(n)) == -22
    assert lib.dsh_linkage_threshold_device(None, 2, 1, 31, 0.5, 1, None, ctypes.byref(n)) == -22
    assert lib.dsh_linkage_tri(None, 4, None, 0, 0.5, 1, None, ctypes.byref(n)) == -22


def test_header_with_the_linkage_section_is_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dashing_hip.h"\n'
                   "int main(void) { dsh_ctx *c = 0; uint64_t nc = 0; uint32_t lab[1]; float tri[1] = {0};\n"
                   "  return dsh_linkage_threshold(c, 2, 1, 31, 0.5f, DSH_LINKAGE_COMPLETE, lab, &nc) +\n"
                   "         dsh_linkage_threshold_device(c, 2, 1, 31, 0.5f, DSH_LINKAGE_AVERAGE, 0, &nc) +\n"
                   "         dsh_linkage_tri(c, 2, tri, 0, 0.5f, DSH_LINKAGE_SINGLE, lab, &nc); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
