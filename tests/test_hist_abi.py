"""CPU checks of dsh_dist_histogram, dsh_dist_histogram_device and dsh_dist_rect_histogram: declared in a header that is
still plain C11 with the signatures of the contract, exported by the library, bound in Python, added without a new ABI
version; and the argument errors that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dsh_dist_histogram": 10, "dsh_dist_histogram_device": 10, "dsh_dist_rect_histogram": 12}


def header():
    with open(os.path.join(ROOT, "include", "dashing_hip.h")) as f:
        return f.read()


def test_entry_points_declared_exported_and_bound():
    hdr = header()
    lib = ctypes.CDLL(dashing_amd.lib_path())
    for s, nargs in NAMES.items():
        assert hasattr(lib, s), s
        assert s in api.SYMBOLS
        assert getattr(api.load_library(), s).argtypes is not None and len(getattr(api.load_library(), s).argtypes) == nargs, s
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int dsh_dist_histogram(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin, uint64_t row_end, "
            "const float *edges, uint32_t n_edges, const uint32_t *labels, uint64_t *counts_out);") in flat
    assert ("int dsh_dist_histogram_device(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin, uint64_t row_end, "
            "const float *edges, uint32_t n_edges, const uint32_t *labels, void *d_counts);") in flat
    assert ("int dsh_dist_rect_histogram(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t q_begin, uint64_t q_end, "
            "uint64_t r_begin, uint64_t r_end, const float *edges, uint32_t n_edges, const uint32_t *labels, "
            "uint64_t *counts_out);") in flat
    for m in ("dist_histogram", "dist_histogram_device", "dist_rect_histogram"):
        assert callable(getattr(dashing_amd.Context, m))
    assert callable(dashing_amd.histogram_hits)
    assert api.ABI_VERSION == 7 and api.abi_version() == 7  # entry points were only added
    added = hdr[hdr.index("only ADDED") : hdr.index("#define DSH_ABI_VERSION")]
    for s in NAMES:
        assert s in added, s
    assert re.search(r"#define DSH_HIST_MAX_EDGES 4096\b", hdr) and dashing_amd.HIST_MAX_EDGES == 4096
    section = hdr[hdr.index("value histograms of the triangle") : hdr.index("#define DSH_HIST_MAX_EDGES")]
    assert "Not built:" in section and "multi-GPU" in section and "quantiles" in section


def test_a_null_context_is_an_argument_error():
    lib = api.load_library()
    edges = np.array([0.25, 0.5], np.float32)
    out = np.zeros(8, np.uint64)
    lab = np.zeros(4, np.uint32)
    assert lib.dsh_dist_histogram(None, 2, 1, 31, 0, 4, edges.ctypes.data, 2, None, out.ctypes.data) == -22
    assert lib.dsh_dist_histogram(None, 2, 1, 31, 0, 4, edges.ctypes.data, 2, lab.ctypes.data, out.ctypes.data) == -22
    assert lib.dsh_dist_histogram_device(None, 2, 1, 31, 0, 4, edges.ctypes.data, 2, None, None) == -22
    assert lib.dsh_dist_rect_histogram(None, 2, 1, 31, 0, 2, 2, 4, edges.ctypes.data, 2, None, out.ctypes.data) == -22
    assert not out.any()


def test_header_with_the_histogram_section_is_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dashing_hip.h"\n'
                   "int main(void) { dsh_ctx *c = 0; const float e[2] = {0.f, 1.f}; const uint32_t lab[2] = {0, 0}; uint64_t cnt[8];\n"
                   "  return dsh_dist_histogram(c, 2, 1, 31, 0, 2, e, 2, lab, cnt) + dsh_dist_histogram_device(c, 2, 1, 31, 0, 2, e, 2, 0, 0)\n"
                   "       + dsh_dist_rect_histogram(c, 2, 1, 31, 0, 1, 1, 2, e, 2, lab, cnt) + (DSH_HIST_MAX_EDGES == 4096 ? 0 : 1); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
