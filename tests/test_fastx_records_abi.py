"""CPU checks of the device-parsed per-record sketch entry point (dsh_sketch_fastx_records): declared in the header,
exported by the library, bound in Python, and announced as an entry point that was only added (the ABI version stays)."""
import ctypes
import os
import re

import dashing_amd
from dashing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dsh_sketch_fastx_records"


def header():
    with open(os.path.join(ROOT, "include", "dashing_hip.h")) as f:
        return f.read()


def test_entry_point_declared_exported_and_bound():
    assert re.search(r"\bint %s\(" % NAME, header())
    assert hasattr(ctypes.CDLL(dashing_amd.lib_path()), NAME)
    assert NAME in api.SYMBOLS
    for m in ("sketch_fastx_records", "count_fastx_records"):
        assert callable(getattr(dashing_amd.Context, m))


def test_added_without_a_new_abi_version():
    assert api.ABI_VERSION == 7 and api.abi_version() == 7
    assert re.search(r"#define DSH_ABI_VERSION 7\b", header())
    added = re.search(r"only ADDED since(.*?)\*/", header(), re.S).group(1)
    assert re.search(r"\b%s\b" % NAME, added)
