"""CPU checks of dsh_union_curve, dsh_union_curve_device and dsh_curve_permutations: declared in a header that is still
plain C11 with the signatures of the contract, exported by the library, bound in Python, added without a new ABI version;
and the argument errors that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"dsh_union_curve": 7, "dsh_union_curve_device": 7, "dsh_curve_permutations": 4}


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
    assert ("int dsh_union_curve(dsh_ctx *ctx, int estim, const uint32_t *orders, uint64_t len, uint64_t n_orders, "
            "double *card_out, uint32_t *hist_out);") in flat
    assert ("int dsh_union_curve_device(dsh_ctx *ctx, int estim, const void *d_orders, uint64_t len, uint64_t n_orders, "
            "void *d_card, void *d_hist);") in flat
    assert "int dsh_curve_permutations(uint64_t n, uint64_t n_perm, uint64_t seed, uint32_t *out);" in flat
    for m in ("union_curve", "union_curve_device"):
        assert callable(getattr(dashing_amd.Context, m))
    assert callable(dashing_amd.curve_permutations)
    assert api.ABI_VERSION == 7 and api.abi_version() == 7  # entry points were only added
    added = hdr[hdr.index("only ADDED") : hdr.index("#define DSH_ABI_VERSION")]
    for s in NAMES:
        assert s in added, s
    assert re.search(r"#define DSH_CURVE_BINS 64\b", hdr) and dashing_amd.CURVE_BINS == 64
    section = hdr[hdr.index("union growth curves") : hdr.index("#define DSH_CURVE_BINS")]
    assert "Not built:" in section
    tail = section[section.index("Not built:") :]
    for word in ("multi-GPU", "second context", "--groups", "greedy"):
        assert word in tail, word
    for word in ("curve_segment", "curve_scratch_bytes", "untouched", "DSH_ESTATE", "DSH_ENOMEM"):
        assert word in section, word


def test_a_null_context_is_an_argument_error_and_writes_nothing():
    lib = api.load_library()
    order = np.arange(4, dtype=np.uint32)
    card = np.full(4, -7.0)
    hist = np.full(4 * 64, 0xC0DE, np.uint32)
    assert lib.dsh_union_curve(None, 2, order.ctypes.data, 4, 1, card.ctypes.data, hist.ctypes.data) == -22
    assert lib.dsh_union_curve(None, 2, order.ctypes.data, 0, 0, None, None) == -22
    assert lib.dsh_union_curve_device(None, 2, None, 4, 1, None, None) == -22
    assert (card == -7.0).all() and (hist == 0xC0DE).all()


def test_curve_permutations_argument_errors():
    lib = api.load_library()
    out = np.full(6, 0xC0DE, np.uint32)
    assert lib.dsh_curve_permutations(1 << 32, 1, 0, out.ctypes.data) == -22
    assert lib.dsh_curve_permutations(1 << 32, 0, 0, None) == -22
    assert lib.dsh_curve_permutations(3, 2, 0, None) == -22
    assert (out == 0xC0DE).all()
    # nothing to write: a NULL out is fine
    assert lib.dsh_curve_permutations(0, 5, 0, None) == 0 and lib.dsh_curve_permutations(5, 0, 0, None) == 0
    assert lib.dsh_curve_permutations(3, 2, 0, out.ctypes.data) == 0
    assert sorted(out[:3]) == [0, 1, 2] and sorted(out[3:]) == [0, 1, 2]
    try:
        dashing_amd.curve_permutations(1 << 32, 0, 0)
    except dashing_amd.DshError as e:
        assert e.code == -22
    else:
        raise AssertionError("n = 2^32 was accepted")


def test_header_with_the_curve_section_is_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dashing_hip.h"\n'
                   "int main(void) { dsh_ctx *c = 0; const uint32_t ord[2] = {0, 1}; double card[2]; uint32_t hist[2 * DSH_CURVE_BINS], perm[4];\n"
                   "  return dsh_union_curve(c, DSH_ESTIM_ERTL_MLE, ord, 2, 1, card, hist) + dsh_union_curve_device(c, 2, 0, 2, 1, 0, 0)\n"
                   "       + dsh_curve_permutations(2, 2, 11, perm) + (DSH_CURVE_BINS == 64 ? 0 : 1); }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
