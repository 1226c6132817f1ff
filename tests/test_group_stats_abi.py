"""CPU checks of dsh_group_stats and dsh_group_stats_device: declared in a header that is still plain C11 with the
signatures of the contract, exported by the library, bound in Python, added without a new ABI version; and the argument
errors that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dsh_group_stats", "dsh_group_stats_device"]


def header():
    with open(os.path.join(ROOT, "include", "dashing_hip.h")) as f:
        return f.read()


def test_entry_points_declared_exported_and_bound():
    hdr = header()
    lib = ctypes.CDLL(dashing_amd.lib_path())
    for s in NAMES:
        assert hasattr(lib, s), s
        assert s in api.SYMBOLS
        assert getattr(api.load_library(), s).argtypes is not None and len(getattr(api.load_library(), s).argtypes) == 9, s
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int dsh_group_stats(dsh_ctx *ctx, int estim, int result_type, int k, const uint32_t *labels, uint32_t *medoid_out, "
            "uint32_t *cnt_out, int64_t *sum_out, float *worst_out);") in flat
    assert ("int dsh_group_stats_device(dsh_ctx *ctx, int estim, int result_type, int k, const uint32_t *labels, void *d_medoid, "
            "void *d_cnt, void *d_sum, void *d_worst);") in flat
    for m in ("group_stats", "group_stats_device"):
        assert callable(getattr(dashing_amd.Context, m))
    assert api.ABI_VERSION == 7 and api.abi_version() == 7  # entry points were only added
    added = hdr[hdr.index("only ADDED") : hdr.index("#define DSH_ABI_VERSION")]
    for s in NAMES:
        assert s in added, s
    assert re.search(r"#define DSH_STATS_FRAC_BITS 30\b", hdr) and dashing_amd.STATS_FRAC_BITS == 30
    assert '"stats_route"' in hdr[hdr.index("Options; returns") : hdr.index("int dsh_set_option")]
    assert '"stats_route"' in hdr[hdr.index("int dsh_set_option") : hdr.index("int dsh_get_info")]


def test_a_null_context_is_an_argument_error():
    lib = api.load_library()
    lab = np.zeros(4, np.uint32)
    out = np.zeros(4, np.uint64)
    assert lib.dsh_group_stats(None, 2, 1, 31, lab.ctypes.data, out.ctypes.data, None, None, None) == -22
    assert lib.dsh_group_stats(None, 2, 1, 31, None, None, None, None, None) == -22
    assert lib.dsh_group_stats_device(None, 2, 1, 31, lab.ctypes.data, None, None, None, None) == -22


def test_the_result_type_derives_mean_and_diameter():
    lab = np.array([0, 0, 0, 3, 4, 4], np.uint32)
    cnt = np.array([2, 2, 1, 0, 1, 1], np.uint32)
    sm = np.array([3 << 29, 1 << 30, -(1 << 28), 0, 1 << 29, 1 << 29], np.int64)
    worst = np.array([0.25, 0.5, -0.25, np.nan, 0.5, 0.5], np.float32)
    med = np.array([0, 0, 0, 3, 4, 4], np.uint32)
    for descending, diam in ((True, [-0.25] * 3 + [np.nan, 0.5, 0.5]), (False, [0.5] * 3 + [np.nan, 0.5, 0.5])):
        r = dashing_amd.GroupStats(med, cnt, sm, worst, lab, descending)
        assert r.medoid is med and r.cnt is cnt and r.sum is sm and r.worst is worst and len(r) == 4
        assert np.array_equal(r.mean, [0.75, 0.5, -0.25, np.nan, 0.5, 0.5], equal_nan=True) and r.mean.dtype == np.float64
        assert np.array_equal(r.diameter, np.array(diam, np.float32), equal_nan=True) and r.diameter.dtype == np.float32


def test_header_with_the_stats_section_is_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dashing_hip.h"\n'
                   "int main(void) { dsh_ctx *c = 0; uint32_t med[2], cnt[2]; int64_t sum[2]; float worst[2]; const uint32_t lab[2] = {0, 0};\n"
                   "  return dsh_group_stats(c, 2, 1, 31, lab, med, cnt, sum, worst) + dsh_group_stats_device(c, 2, 1, 31, lab, 0, 0, 0, 0)\n"
                   "       + (DSH_STATS_FRAC_BITS == 30 ? 0 : 1); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
