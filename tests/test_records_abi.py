"""CPU checks of the per-record sketch entry points (dsh_sketch_records*): declared in the header, exported by the
library, bound in Python, and the ABI version that announces them."""
import ctypes
import os
import re

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dsh_sketch_records", "dsh_sketch_records_async", "dsh_sketch_records_device"]


def test_records_entry_points_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dashing_hip.h")) as f:
        hdr = f.read()
    lib = ctypes.CDLL(dashing_amd.lib_path())
    for s in NAMES:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in api.SYMBOLS
    for m in ("sketch_records", "sketch_records_async", "sketch_records_device"):
        assert callable(getattr(dashing_amd.Context, m))


def test_abi_version_announces_records():
    assert api.ABI_VERSION == 7
    assert api.abi_version() == 7
