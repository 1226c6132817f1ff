"""CPU checks of the derived-sketch entry points (dsh_fold*, dsh_upload_sketches_folded*, dsh_union_groups*): declared in
a header that is still plain C11, exported by the library, bound in Python, and added without a new ABI version."""
import ctypes
import os
import re
import subprocess

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dsh_fold", "dsh_fold_device", "dsh_upload_sketches_folded", "dsh_upload_sketches_folded_device", "dsh_union_groups",
         "dsh_union_groups_device"]


def test_derive_entry_points_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dashing_hip.h")) as f:
        hdr = f.read()
    lib = ctypes.CDLL(dashing_amd.lib_path())
    for s in NAMES:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in api.SYMBOLS
    for m in ("fold", "fold_device", "upload_folded", "upload_folded_device", "union_groups", "union_groups_device"):
        assert callable(getattr(dashing_amd.Context, m))
    assert api.ABI_VERSION == 7 and api.abi_version() == 7  # entry points were only added


def test_header_with_the_derive_section_is_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dashing_hip.h"\n'
                   "int main(void) { dsh_ctx *c = 0; uint64_t gp[2] = {0, 0}; return dsh_fold(c, 0, 0, 4, 0) + "
                   "dsh_union_groups(c, gp, 0, 1, 0) + dsh_upload_sketches_folded_device(c, 0, 14, 0, 0); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
