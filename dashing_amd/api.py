"""ctypes binding of libdashing_hip.so (include/dashing_hip.h).

There is deliberately no CPU fallback here: if the shared library is missing, or no gfx950
device is visible, construction fails loudly.  (The CPU oracle lives in oracle/ and is test
infrastructure only -- nothing in this package imports it.)
"""
import collections
import ctypes as C
import math
import os
import re

import numpy as np

ESTIM_ORIGINAL, ESTIM_ERTL_IMPROVED, ESTIM_ERTL_MLE = 0, 1, 2
MASH_DIST, JI, FULL_MASH_DIST = 0, 1, 3  # bns::EmissionType, src/enums.h:13-23
SIZES, FULL_CONTAINMENT_DIST, CONTAINMENT_INDEX, CONTAINMENT_DIST = 2, 4, 5, 6
SYMMETRIC_CONTAINMENT_INDEX, SYMMETRIC_CONTAINMENT_DIST = 7, 8
GREEDY_FIRST, GREEDY_BEST = 0, 1  # assign_mode of dsh_greedy_extend* and dsh_dbscan_*
DBSCAN_NOISE, DBSCAN_BORDER, DBSCAN_CORE = 0, 1, 2  # DSH_DBSCAN_*: kind[] of dsh_dbscan_*
HIST_MAX_EDGES = 4096  # DSH_HIST_MAX_EDGES: the edges of one dsh_dist_histogram* call
CURVE_BINS = 64  # DSH_CURVE_BINS: the bins of a prefix's register histogram (union_curve)
LINKAGE_SINGLE, LINKAGE_COMPLETE, LINKAGE_AVERAGE = 0, 1, 2  # DSH_LINKAGE_*
STATS_FRAC_BITS = 30  # DSH_STATS_FRAC_BITS: sums of dsh_group_stats* are in units of 2^-30
# the measures for which a larger value is better (the others are the *_DIST forms; SIZES has no order)
SIMILARITY_TYPES = (JI, CONTAINMENT_INDEX, SYMMETRIC_CONTAINMENT_INDEX)
# the *_DIST forms: a smaller value is better and a threshold passes with v <= t; every other measure, SIZES included, ranks
# descending and passes with v >= t (measure_descending of the library)
DISTANCE_TYPES = (MASH_DIST, FULL_MASH_DIST, FULL_CONTAINMENT_DIST, CONTAINMENT_DIST, SYMMETRIC_CONTAINMENT_DIST)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# every symbol include/dashing_hip.h declares (tests check the .so exports all of them)
SYMBOLS = [
    "dsh_backend_name", "dsh_device_count", "dsh_create", "dsh_destroy", "dsh_last_error",
    "dsh_synchronize", "dsh_sketches_alloc", "dsh_upload_sketches", "dsh_download_sketches", "dsh_copy_sketches_device",
    "dsh_attach_device_sketches", "dsh_sketch_batch", "dsh_sketch_batch_async", "dsh_sketch_batch_device", "dsh_sketch_fastx_batch_async",
    "dsh_sketch_fastx_records",
    "dsh_sketch_records", "dsh_sketch_records_async", "dsh_sketch_records_device",
    "dsh_clear_sketches", "dsh_cardinalities", "dsh_dist_rows", "dsh_dist_rows_device",
    "dsh_dist_rows_async", "dsh_dist_rows_device_async", "dsh_wait", "dsh_wait_event",
    "dsh_event_record", "dsh_event_wait", "dsh_event_query",
    "dsh_comm_available", "dsh_comm_library", "dsh_comm_wait", "dsh_exchange_mode", "dsh_exchange_rows_device_async",
    "dsh_exchange_collect_async", "dsh_exchange_place_device", "dsh_exchange_probe_parts_async", "dsh_diag_spin_start", "dsh_diag_spin_stop", "dsh_abi_version", "dsh_preload", "dsh_comm_unique_id", "dsh_comm_init", "dsh_comm_destroy", "dsh_comm_rank", "dsh_collect_spans", "dsh_collect_spans_async",
    "dsh_allgather_device", "dsh_dist_collect", "dsh_range_parts", "dsh_dist_rows_parts_device_async", "dsh_collect_parts_async",
    "dsh_dist_rect", "dsh_knn", "dsh_dist_threshold", "dsh_dist_threshold_device", "dsh_dist_rect_threshold", "dsh_dist_pairs", "dsh_dist_pairs_device", "dsh_dist_pairs_csr",
    "dsh_cluster_threshold", "dsh_cluster_threshold_device", "dsh_cluster_pairs", "dsh_cluster_csr",
    "dsh_greedy_threshold", "dsh_greedy_threshold_device", "dsh_greedy_extend", "dsh_greedy_extend_device",
    "dsh_group_stats", "dsh_group_stats_device",
    "dsh_dist_histogram", "dsh_dist_histogram_device", "dsh_dist_rect_histogram",
    "dsh_linkage_threshold", "dsh_linkage_threshold_device", "dsh_linkage_tri",
    "dsh_mst", "dsh_mst_tri", "dsh_mst_linkage",
    "dsh_dbscan_threshold", "dsh_dbscan_threshold_device", "dsh_dbscan_tri", "dsh_degree_threshold", "dsh_degree_threshold_device",
    "dsh_union_curve", "dsh_union_curve_device", "dsh_curve_permutations",
    "dsh_fold", "dsh_fold_device", "dsh_upload_sketches_folded", "dsh_upload_sketches_folded_device", "dsh_union_groups", "dsh_union_groups_device", "dsh_shard_plan", "dsh_dist_shard_device", "dsh_unpermute_device", "dsh_unpermute_staged_device", "dsh_unpermute_blocks_device", "dsh_tri_span", "dsh_tri_index", "dsh_partition_rows", "dsh_balance_rows", "dsh_balance_rowsets", "dsh_rowsets_from_bounds", "dsh_rowsets_rank", "dsh_alloc_host", "dsh_free_host",
    "dsh_set_profiling", "dsh_last_kernel_ms", "dsh_last_part_info", "dsh_finalize_phase_cycles", "dsh_set_option", "dsh_get_info", "dsh_stream",
]


ERANGE = -34  # DSH_ERANGE: dist_threshold_device's capacity was too small (the exception carries n_hits)
_NAME = re.compile(rb"[^ \t\n\v\f\r]*")  # a record's kseq name: the bytes behind '>' / '@' up to the first isspace byte


class DshError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("dashing_hip error %d: %s" % (code, msg))
        self.code = code


def lib_path():
    return os.path.join(_HERE, "libdashing_hip.so")


def _preload_torch_hip_runtime():
    """A process must hold ONE HIP runtime.  The PyTorch wheel brings its own libamdhip64.so (SONAME libamdhip64.so.7, the
    name libdashing_hip.so asks for); if this library were loaded first it would pull in /opt/rocm's copy and a later
    `import torch` would add the wheel's next to it -- torch then finds no GPU.  So when a torch installation exists and
    is not loaded yet, its runtime is loaded first (tests and bench.py use torch for device buffers; a C++ host never
    comes here)."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """Load libdashing_hip.so (built in-tree by __graft_entry__.build() / csrc/Makefile)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C dashing_amd/csrc` (there is no CPU fallback)" % path)
    _preload_torch_hip_runtime()
    lib = C.CDLL(path)
    if int(lib.dsh_abi_version()) != ABI_VERSION:  # (a stale in-tree .so: shifted arguments, not link errors)
        raise ImportError("%s has ABI version %d, this binding was written against %d: rebuild (make -C dashing_amd/csrc)" % (path, lib.dsh_abi_version(), ABI_VERSION))
    u64, i32, vp = C.c_uint64, C.c_int, C.c_void_p
    lib.dsh_backend_name.restype = C.c_char_p
    lib.dsh_device_count.restype = i32
    lib.dsh_create.argtypes = [i32, C.POINTER(vp)]
    lib.dsh_destroy.argtypes = [vp]
    lib.dsh_destroy.restype = None
    lib.dsh_last_error.argtypes = [vp]
    lib.dsh_last_error.restype = C.c_char_p
    lib.dsh_synchronize.argtypes = [vp]
    lib.dsh_sketches_alloc.argtypes = [vp, u64, i32]
    lib.dsh_upload_sketches.argtypes = [vp, vp, u64, u64]
    lib.dsh_download_sketches.argtypes = [vp, u64, u64, vp]
    lib.dsh_copy_sketches_device.argtypes = [vp, u64, u64, vp]
    lib.dsh_attach_device_sketches.argtypes = [vp, vp, u64, i32]
    lib.dsh_sketch_batch.argtypes = [vp, vp, vp, C.c_uint32, u64, i32, i32, vp]
    lib.dsh_sketch_batch_async.argtypes = [vp, vp, vp, C.c_uint32, u64, i32, i32]
    lib.dsh_sketch_fastx_batch_async.argtypes = [vp, vp, vp, vp, C.c_uint32, u64, i32, i32, vp]
    lib.dsh_sketch_fastx_records.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, i32, i32, vp, vp, vp]
    lib.dsh_sketch_batch_device.argtypes = [vp, vp, vp, C.c_uint32, u64, i32, i32]
    lib.dsh_sketch_records.argtypes = [vp, vp, vp, C.c_uint32, u64, i32, i32, vp]
    lib.dsh_sketch_records_async.argtypes = [vp, vp, vp, C.c_uint32, u64, i32, i32]
    lib.dsh_sketch_records_device.argtypes = [vp, vp, vp, C.c_uint32, u64, i32, i32]
    lib.dsh_clear_sketches.argtypes = [vp, u64, u64]
    lib.dsh_cardinalities.argtypes = [vp, i32, vp]
    lib.dsh_dist_rows.argtypes = [vp, i32, i32, i32, u64, u64, vp]
    lib.dsh_dist_rows_device.argtypes = [vp, i32, i32, i32, u64, u64, vp]
    lib.dsh_dist_rows_async.argtypes = [vp, i32, i32, i32, u64, u64, vp]
    lib.dsh_dist_rows_device_async.argtypes = [vp, i32, i32, i32, u64, u64, vp]
    lib.dsh_wait.argtypes = [vp]
    lib.dsh_wait_event.argtypes = [vp, vp]
    lib.dsh_event_record.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.dsh_event_wait.argtypes = [vp, u64]
    lib.dsh_event_query.argtypes = [vp, u64, C.POINTER(i32)]
    lib.dsh_comm_unique_id.argtypes = [vp]
    lib.dsh_comm_available.argtypes = []
    lib.dsh_comm_library.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(i32)]
    lib.dsh_comm_wait.argtypes = [vp]
    lib.dsh_exchange_mode.argtypes = [u64, vp, i32, C.c_uint32, i32, C.POINTER(i32), C.POINTER(C.c_uint32), C.POINTER(u64)]
    lib.dsh_exchange_rows_device_async.argtypes = [vp, i32, i32, i32, vp, i32, C.c_uint32, i32, vp]
    lib.dsh_exchange_collect_async.argtypes = [vp, u64, vp, C.c_uint32, vp, vp, i32]
    lib.dsh_exchange_place_device.argtypes = [vp, vp, i32, C.c_uint32, i32, vp, vp]
    lib.dsh_exchange_probe_parts_async.argtypes = [vp, u64, vp, i32, C.c_uint32, i32, vp, vp]
    lib.dsh_diag_spin_start.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.dsh_diag_spin_stop.argtypes = [vp]
    lib.dsh_abi_version.argtypes = []
    lib.dsh_abi_version.restype = C.c_int
    lib.dsh_balance_rowsets.argtypes = [u64, C.c_uint32, i32, i32, i32, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.dsh_rowsets_from_bounds.argtypes = [vp, C.c_uint32, vp]
    lib.dsh_rowsets_rank.argtypes = [u64, vp, C.c_uint32, vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(u64), C.POINTER(u64)]
    lib.dsh_finalize_phase_cycles.argtypes = [vp, vp]
    lib.dsh_last_part_info.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.dsh_comm_init.argtypes = [vp, vp, i32, i32]
    lib.dsh_comm_destroy.argtypes = [vp]
    lib.dsh_comm_rank.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    lib.dsh_collect_spans.argtypes = [vp, u64, vp, vp, vp, i32]
    lib.dsh_collect_spans_async.argtypes = [vp, u64, vp, vp, vp, i32]
    lib.dsh_allgather_device.argtypes = [vp, vp, u64, vp]
    lib.dsh_dist_collect.argtypes = [vp, i32, i32, i32, vp, i32, vp]
    lib.dsh_range_parts.argtypes = [u64, u64, u64, C.c_uint32, vp, C.POINTER(C.c_uint32)]
    lib.dsh_dist_rows_parts_device_async.argtypes = [vp, i32, i32, i32, u64, u64, vp, C.c_uint32]
    lib.dsh_collect_parts_async.argtypes = [vp, u64, vp, C.c_uint32, vp, vp, i32]
    lib.dsh_dist_rect.argtypes = [vp, i32, i32, i32, u64, u64, u64, u64, vp]
    lib.dsh_knn.argtypes = [vp, i32, i32, i32, u64, u64, u64, u64, C.c_uint32, vp, vp]
    lib.dsh_dist_threshold.argtypes = [vp, i32, i32, i32, u64, u64, C.c_float, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    lib.dsh_dist_threshold_device.argtypes = [vp, i32, i32, i32, u64, u64, C.c_float, vp, vp, vp, u64, C.POINTER(u64)]
    lib.dsh_dist_rect_threshold.argtypes = [vp, i32, i32, i32, u64, u64, u64, u64, C.c_float, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    lib.dsh_dist_pairs.argtypes = [vp, i32, vp, C.c_uint32, i32, vp, vp, u64, vp]
    lib.dsh_dist_pairs_device.argtypes = [vp, i32, vp, C.c_uint32, i32, vp, vp, u64, vp]
    lib.dsh_dist_pairs_csr.argtypes = [vp, i32, vp, C.c_uint32, i32, u64, u64, vp, vp, vp]
    # derived sketches and clusters: bound by name, so that a library built before they existed still loads (calling one then fails)
    for name, args in (("dsh_fold", [vp, u64, u64, i32, vp]), ("dsh_fold_device", [vp, u64, u64, i32, vp]),
                       ("dsh_upload_sketches_folded", [vp, vp, i32, u64, u64]),
                       ("dsh_upload_sketches_folded_device", [vp, vp, i32, u64, u64]),
                       ("dsh_union_groups", [vp, vp, vp, u64, vp]), ("dsh_union_groups_device", [vp, vp, vp, u64, vp]),
                       ("dsh_cluster_threshold", [vp, i32, i32, i32, C.c_float, vp, C.POINTER(u64)]),
                       ("dsh_cluster_threshold_device", [vp, i32, i32, i32, C.c_float, vp, C.POINTER(u64)]),
                       ("dsh_cluster_pairs", [vp, u64, vp, vp, u64, vp, vp, C.POINTER(u64)]),
                       ("dsh_cluster_csr", [vp, u64, u64, u64, vp, vp, vp, vp, C.POINTER(u64)]),
                       ("dsh_greedy_threshold", [vp, i32, i32, i32, C.c_float, vp, C.POINTER(u64)]),
                       ("dsh_greedy_threshold_device", [vp, i32, i32, i32, C.c_float, vp, C.POINTER(u64)]),
                       ("dsh_greedy_extend", [vp, i32, i32, i32, C.c_float, i32, u64, vp, vp, C.POINTER(u64)]),
                       ("dsh_greedy_extend_device", [vp, i32, i32, i32, C.c_float, i32, u64, vp, vp, C.POINTER(u64)]),
                       ("dsh_group_stats", [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
                       ("dsh_group_stats_device", [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
                       ("dsh_dist_histogram", [vp, i32, i32, i32, u64, u64, vp, C.c_uint32, vp, vp]),
                       ("dsh_dist_histogram_device", [vp, i32, i32, i32, u64, u64, vp, C.c_uint32, vp, vp]),
                       ("dsh_dist_rect_histogram", [vp, i32, i32, i32, u64, u64, u64, u64, vp, C.c_uint32, vp, vp]),
                       ("dsh_linkage_threshold", [vp, i32, i32, i32, C.c_float, i32, vp, C.POINTER(u64)]),
                       ("dsh_linkage_threshold_device", [vp, i32, i32, i32, C.c_float, i32, vp, C.POINTER(u64)]),
                       ("dsh_linkage_tri", [vp, u64, vp, i32, C.c_float, i32, vp, C.POINTER(u64)]),
                       ("dsh_mst", [vp, i32, i32, i32, C.c_float, vp, vp, vp, C.POINTER(u64), vp]),
                       ("dsh_mst_tri", [vp, u64, vp, i32, C.c_float, vp, vp, vp, C.POINTER(u64), vp]),
                       ("dsh_mst_linkage", [u64, vp, vp, vp, u64, vp, vp, vp, vp]),
                       ("dsh_dbscan_threshold", [vp, i32, i32, i32, C.c_float, C.c_uint32, i32, vp, vp, vp, C.POINTER(u64), C.POINTER(u64)]),
                       ("dsh_dbscan_threshold_device", [vp, i32, i32, i32, C.c_float, C.c_uint32, i32, vp, vp, vp, C.POINTER(u64), C.POINTER(u64)]),
                       ("dsh_dbscan_tri", [vp, u64, vp, i32, C.c_float, C.c_uint32, i32, vp, vp, vp, C.POINTER(u64), C.POINTER(u64)]),
                       ("dsh_degree_threshold", [vp, i32, i32, i32, C.c_float, vp]),
                       ("dsh_degree_threshold_device", [vp, i32, i32, i32, C.c_float, vp]),
                       ("dsh_union_curve", [vp, i32, vp, u64, u64, vp, vp]), ("dsh_union_curve_device", [vp, i32, vp, u64, u64, vp, vp]),
                       ("dsh_curve_permutations", [u64, u64, u64, vp])):
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes = args
    lib.dsh_shard_plan.argtypes = [vp, i32, C.c_uint32, vp]
    lib.dsh_dist_shard_device.argtypes = [vp, i32, i32, i32, C.c_uint32, C.c_uint32, vp]
    lib.dsh_unpermute_device.argtypes = [vp, vp, vp]
    lib.dsh_unpermute_staged_device.argtypes = [vp, vp, u64, C.c_uint32, vp]
    lib.dsh_unpermute_blocks_device.argtypes = [vp, vp, vp, C.c_uint32, vp]
    lib.dsh_tri_span.argtypes = [u64, u64, u64]
    lib.dsh_tri_span.restype = u64
    lib.dsh_tri_index.argtypes = [u64, u64, u64]
    lib.dsh_tri_index.restype = u64
    lib.dsh_partition_rows.argtypes = [u64, C.c_uint32, C.c_uint32, vp]
    lib.dsh_balance_rows.argtypes = [u64, C.c_uint32, vp]
    lib.dsh_alloc_host.argtypes = [C.c_size_t]
    lib.dsh_alloc_host.restype = vp
    lib.dsh_free_host.argtypes = [vp]
    lib.dsh_free_host.restype = None
    lib.dsh_set_profiling.argtypes = [vp, i32]
    lib.dsh_last_kernel_ms.argtypes = [vp, vp, vp, vp, vp]
    lib.dsh_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    lib.dsh_get_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    lib.dsh_stream.argtypes = [vp]
    lib.dsh_stream.restype = vp
    _LIB = lib
    return lib


def backend_name():
    return load_library().dsh_backend_name().decode()


ABI_VERSION = 7  # include/dashing_hip.h DSH_ABI_VERSION this binding was written against


def abi_version():
    return int(load_library().dsh_abi_version())


def device_count():
    return int(load_library().dsh_device_count())


def comm_unique_id():
    """128 bytes (an ncclUniqueId) created by RCCL inside the library: rank 0 makes it, every rank passes it to
    Context.comm_init.  Raises if RCCL cannot be loaded."""
    buf = C.create_string_buffer(128)
    rc = load_library().dsh_comm_unique_id(buf)
    if rc:
        raise DshError(rc, "dsh_comm_unique_id (RCCL not available?)")
    return buf.raw


def comm_available():
    """True if librccl can be loaded by the library in this process (local check, no communication)"""
    return load_library().dsh_comm_available() == 0


def comm_library():
    """(resolved path of the loaded librccl -- or the loader's error text --, ncclGetVersion code or 0)"""
    buf = C.create_string_buffer(1024)
    v = C.c_int(0)
    load_library().dsh_comm_library(buf, len(buf), C.byref(v))
    return buf.value.decode(errors="replace"), int(v.value)


class RowSets:
    """A partition of the triangle's rows over the ranks as a row-set table (include/dashing_hip.h): row segments with
    owners.  `table` is the uint64 array the C-ABI takes; rows(r) the segments of rank r, pairs(r) / tiles(r) its work."""

    def __init__(self, n, table):
        self.n = int(n)
        self.table = np.ascontiguousarray(table, np.uint64)
        self.world = int(self.table[0])

    def _rank(self, r):
        segs = np.zeros(2 * max(int(self.table[1]), 1), np.uint64)
        ns, pairs, tiles = C.c_uint32(), C.c_uint64(), C.c_uint64()
        rc = load_library().dsh_rowsets_rank(self.n, self.table.ctypes.data, r, segs.ctypes.data, len(segs) // 2, C.byref(ns),
                                             C.byref(pairs), C.byref(tiles))
        if rc:
            raise DshError(rc, "dsh_rowsets_rank: malformed row-set table")
        return [(int(segs[2 * i]), int(segs[2 * i + 1])) for i in range(ns.value)], int(pairs.value), int(tiles.value)

    def rows(self, r):
        return self._rank(r)[0]

    def pairs(self, r):
        return self._rank(r)[1]

    def tiles(self, r):
        return self._rank(r)[2]

    def describe(self):
        return [{"rank": r, "rows": self.rows(r), "pairs": self.pairs(r), "tiles": self.tiles(r)} for r in range(self.world)]


def balance_rowsets(n, world, prep_permille=-1, dst=-1, dst_bonus_permille=-1):
    """Main ranges + top-up tile rows from the bottom of the triangle, one row set per rank (dsh_balance_rowsets); dst >= 0:
    the rank that receives the others' rows takes a bonus of work (it sends nothing)."""
    lib = load_library()
    words = C.c_uint32()
    rc = lib.dsh_balance_rowsets(n, world, prep_permille, dst, dst_bonus_permille, None, 0, C.byref(words))
    if rc:
        raise DshError(rc, "dsh_balance_rowsets")
    tab = np.zeros(words.value, np.uint64)
    rc = lib.dsh_balance_rowsets(n, world, prep_permille, dst, dst_bonus_permille, tab.ctypes.data, len(tab), C.byref(words))
    if rc:
        raise DshError(rc, "dsh_balance_rowsets")
    return RowSets(n, tab)


def rowsets_from_bounds(n, bounds):
    """contiguous row ranges bounds[world + 1] as a row-set table (dsh_rowsets_from_bounds)"""
    b = np.ascontiguousarray(bounds, np.uint64)
    tab = np.zeros(3 + 2 * (len(b) - 1), np.uint64)
    rc = load_library().dsh_rowsets_from_bounds(b.ctypes.data, len(b) - 1, tab.ctypes.data)
    if rc:
        raise DshError(rc, "dsh_rowsets_from_bounds")
    return RowSets(n, tab)


def _table(n, rows):
    """the C-ABI table of `rows`: a RowSets, or contiguous bounds [world + 1]"""
    return (rows if isinstance(rows, RowSets) else rowsets_from_bounds(n, rows)).table


def exchange_mode(n, rows, rank, nparts, dst=0, want_floats=False):
    """(rowsorted, parts[, floats of the rank's buffer]) of rank `rank` under dsh_exchange_* (dsh_exchange_mode); `rows` is a
    RowSets or contiguous bounds"""
    t = _table(n, rows)
    rs, k, fl = C.c_int(), C.c_uint32(), C.c_uint64()
    rc = load_library().dsh_exchange_mode(n, t.ctypes.data, rank, nparts, dst, C.byref(rs), C.byref(k), C.byref(fl))
    if rc:
        raise DshError(rc, "dsh_exchange_mode")
    return (bool(rs.value), int(k.value), int(fl.value)) if want_floats else (bool(rs.value), int(k.value))


def range_parts(n, rb, re, nparts):
    """row boundaries of the parts dsh_dist_rows_parts_device_async cuts [rb, re) into (may be fewer than nparts)"""
    b = np.zeros(nparts + 1, np.uint64)
    k = C.c_uint32()
    rc = load_library().dsh_range_parts(n, rb, re, nparts, b.ctypes.data, C.byref(k))
    if rc:
        raise DshError(rc, "dsh_range_parts")
    return [int(x) for x in b[: k.value + 1]]


def tri_span(n, rb, re):
    return int(load_library().dsh_tri_span(n, rb, re))


def tri_index(n, i, j):
    return int(load_library().dsh_tri_index(n, i, j))


def partition_rows(n, nparts, align=128):
    """Host-only helper shared with the C++ CLI: contiguous row ranges of near-equal pair count."""
    b = np.zeros(nparts + 1, np.uint64)
    rc = load_library().dsh_partition_rows(n, nparts, align, b.ctypes.data)
    if rc:
        raise DshError(rc, "dsh_partition_rows")
    return [int(x) for x in b]


def balance_rows(n, nparts):
    """Tile-aligned row ranges, one per rank, minimising the largest tile count (dsh_balance_rows)."""
    b = np.zeros(nparts + 1, np.uint64)
    rc = load_library().dsh_balance_rows(n, nparts, b.ctypes.data)
    if rc:
        raise DshError(rc, "dsh_balance_rows")
    return [int(x) for x in b]


def histogram_hits(counts, result_type):
    """Per edge b of a dist_histogram result (counts of shape (planes, n_edges + 2) or (n_edges + 2,)), the n_hits that
    dist_threshold over the same rows gives at threshold = edges[b]: for the *_DIST forms (DISTANCE_TYPES) the sum of the
    classes 0 .. b, for every other measure -- the similarities and SIZES, which the library ranks descending -- the sum of
    the classes b + 1 .. n_edges.  The NaN class (the last) passes no threshold.  uint64 of shape (planes, n_edges), or
    (n_edges,) for one-dimensional counts."""
    if isinstance(result_type, bool) or result_type not in range(9):
        raise ValueError("unsupported result_type %r" % (result_type,))
    c = np.asarray(counts, np.uint64)
    if c.ndim not in (1, 2) or c.shape[-1] < 3:
        raise ValueError("counts holds n_edges + 2 classes per plane")
    body = c[..., :-1]  # without the NaN class
    if result_type in DISTANCE_TYPES:
        return np.cumsum(body, axis=-1, dtype=np.uint64)[..., :-1]
    return np.cumsum(body[..., ::-1], axis=-1, dtype=np.uint64)[..., ::-1][..., 1:]


def curve_permutations(n, n_perm, seed):
    """uint32 [n_perm][n]: the permutations of 0 .. n - 1 that dsh_curve_permutations draws (a pure function of n, seed
    and the row: the CLI's --curve-permutations orders)"""
    fn = getattr(load_library(), "dsh_curve_permutations", None)
    if fn is None:
        raise DshError(-22, "%s does not export dsh_curve_permutations: rebuild it" % lib_path())
    out = np.zeros((int(n_perm), int(n)), np.uint32)
    rc = fn(int(n), int(n_perm), int(seed) & 0xFFFFFFFFFFFFFFFF, out.ctypes.data)
    if rc:
        raise DshError(rc, "dsh_curve_permutations(n=%d, n_perm=%d)" % (n, n_perm))
    return out


def mst_linkage(n, lhs, rhs, val):
    """(za, zb, zv, zsize): the sorted edge list of Context.mst / mst_tri as a merge table in scipy's Z convention -- leaves
    0 .. n - 1, step s joins the current clusters of lhs[s] and rhs[s] into cluster n + s; za < zb.  Pure host."""
    lhs, rhs = np.ascontiguousarray(lhs, np.uint32).reshape(-1), np.ascontiguousarray(rhs, np.uint32).reshape(-1)
    val = np.ascontiguousarray(val, np.float32).reshape(-1)
    if not lhs.size == rhs.size == val.size:
        raise ValueError("lhs, rhs and val hold one entry per edge")
    m = lhs.size
    za, zb, zv, zsize = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.float32), np.zeros(m, np.uint32)
    ptr = [a.ctypes.data if m else None for a in (lhs, rhs, val, za, zb, zv, zsize)]
    rc = load_library().dsh_mst_linkage(int(n), ptr[0], ptr[1], ptr[2], m, *ptr[3:])
    if rc:
        raise DshError(rc, "dsh_mst_linkage: an edge names a node outside [0, n) or the list is not a forest")
    return za, zb, zv, zsize


class GroupStats(collections.namedtuple("GroupStats", "medoid cnt sum worst")):
    """what Context.group_stats returns: per slot the medoid of its group (uint32), the included pairs with its group
    (uint32), the sum of their values in units of 2^-STATS_FRAC_BITS (int64) and the worst of them (float32, NaN where
    cnt == 0); .mean and .diameter are derived on the host"""

    def __new__(cls, medoid, cnt, sum, worst, labels, descending):
        self = super().__new__(cls, medoid, cnt, sum, worst)
        self.labels, self.descending = labels, bool(descending)
        return self

    @property
    def mean(self):
        """float64 [n]: the mean value of each slot to its group, NaN where cnt == 0"""
        out = np.full(self.cnt.shape, np.nan)
        ok = self.cnt > 0
        out[ok] = self.sum[ok] / self.cnt[ok] / float(1 << STATS_FRAC_BITS)
        return out

    @property
    def diameter(self):
        """float32 [n]: per slot the worst value inside its group (the worst `worst` of its members; NaN: none)"""
        acc = np.full(self.worst.shape, np.nan, np.float32)
        (np.fmin if self.descending else np.fmax).at(acc, self.labels, self.worst)  # (fmin / fmax pass over NaN)
        return acc[self.labels]


class PinnedArray:
    """numpy view of page-locked host memory (dsh_alloc_host); keep the object alive while in use."""

    def __init__(self, n, dtype=np.float32):
        self._lib = load_library()
        nbytes = max(int(n), 1) * np.dtype(dtype).itemsize
        self._p = self._lib.dsh_alloc_host(nbytes)
        if not self._p:
            raise MemoryError("dsh_alloc_host(%d) failed" % nbytes)
        buf = (C.c_char * nbytes).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dtype, count=max(int(n), 1))

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.dsh_free_host(self._p)
            self._p = None


class Context:
    """One GPU.  Mirrors the call sequence of dist_sketch_and_cmp (src/sketch_and_cmp.h:268-417):
    allocate N sketches, fill them (sketch_batch / upload), cardinalities, all-pairs rows."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.dsh_create(device, C.byref(h))
        if rc:
            raise DshError(rc, "dsh_create(device=%d) failed (no gfx950 device?)" % device)
        self._h = h
        self.n = 0
        self.p = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dsh_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc:
            raise DshError(rc, self._lib.dsh_last_error(self._h).decode())

    # ---- sketch matrix
    def alloc(self, n, p):
        self._ck(self._lib.dsh_sketches_alloc(self._h, n, p))
        self.n, self.p = n, p

    def upload(self, regs, first_slot=0):
        regs = np.ascontiguousarray(regs, np.uint8)
        assert regs.ndim == 2 and regs.shape[1] == (1 << self.p)
        self._ck(self._lib.dsh_upload_sketches(self._h, regs.ctypes.data, first_slot, regs.shape[0]))

    def set_sketches(self, regs):
        regs = np.ascontiguousarray(regs, np.uint8)
        n, m = regs.shape
        self.alloc(n, int(m).bit_length() - 1)
        self.upload(regs)

    def attach_device(self, data_ptr, n, p):
        self._ck(self._lib.dsh_attach_device_sketches(self._h, C.c_void_p(data_ptr), n, p))
        self.n, self.p = n, p

    def download(self, first_slot=0, n=None):
        n = self.n - first_slot if n is None else n
        out = np.zeros((n, 1 << self.p), np.uint8)
        self._ck(self._lib.dsh_download_sketches(self._h, first_slot, n, out.ctypes.data))
        return out

    def copy_sketches_device(self, out_ptr, first_slot=0, n=None):
        n = self.n - first_slot if n is None else n
        self._ck(self._lib.dsh_copy_sketches_device(self._h, first_slot, n, C.c_void_p(out_ptr)))

    def clear(self, first_slot=0, n=None):
        n = self.n - first_slot if n is None else n
        self._ck(self._lib.dsh_clear_sketches(self._h, first_slot, n))

    # ---- derived sketches (fold to a lower p, union by groups)
    def _derive(self, name):
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise DshError(-22, "%s does not export %s: rebuild it" % (lib_path(), name))
        return fn

    def fold(self, new_p, first_slot=0, n=None):
        """rows [first_slot, first_slot + n) folded to precision new_p: uint8 [n][2^new_p]"""
        n = self.n - first_slot if n is None else n
        out = np.zeros((n, 1 << max(int(new_p), 0)), np.uint8)
        self._ck(self._derive("dsh_fold")(self._h, first_slot, n, new_p, out.ctypes.data))
        return out

    def fold_device(self, out_ptr, new_p, first_slot=0, n=None):
        n = self.n - first_slot if n is None else n
        self._ck(self._derive("dsh_fold_device")(self._h, first_slot, n, new_p, C.c_void_p(out_ptr)))

    def upload_folded(self, regs, src_p=None, first_slot=0):
        """host rows at precision src_p >= p (default: from regs.shape[1]), folded on the device into the slots"""
        regs = np.ascontiguousarray(regs, np.uint8)
        assert regs.ndim == 2
        if src_p is None:
            src_p = int(regs.shape[1]).bit_length() - 1
        assert regs.shape[1] == (1 << src_p)
        self._ck(self._derive("dsh_upload_sketches_folded")(self._h, regs.ctypes.data, src_p, first_slot, regs.shape[0]))

    def upload_folded_device(self, ptr, src_p, n, first_slot=0):
        self._ck(self._derive("dsh_upload_sketches_folded_device")(self._h, C.c_void_p(ptr), src_p, first_slot, n))

    @staticmethod
    def _groups(group_ptr, members):
        gp = np.ascontiguousarray(group_ptr, np.uint64).reshape(-1)
        mem = np.ascontiguousarray(members, np.uint32).reshape(-1)
        assert gp.size >= 1 and (gp.size == 1 or int(gp[-1]) <= mem.size)
        return gp, mem

    def union_groups(self, group_ptr, members):
        """uint8 [n_groups][2^p]: row g = element-wise max of the resident rows members[group_ptr[g]:group_ptr[g + 1]]"""
        gp, mem = self._groups(group_ptr, members)
        out = np.zeros((gp.size - 1, 1 << self.p), np.uint8)
        self._ck(self._derive("dsh_union_groups")(self._h, gp.ctypes.data, mem.ctypes.data, gp.size - 1, out.ctypes.data))
        return out

    def union_groups_device(self, out_ptr, group_ptr, members):
        gp, mem = self._groups(group_ptr, members)
        self._ck(self._derive("dsh_union_groups_device")(self._h, gp.ctypes.data, mem.ctypes.data, gp.size - 1, C.c_void_p(out_ptr)))

    # ---- union growth curves
    def union_curve(self, orders, estim=ESTIM_ERTL_MLE, want_hist=False):
        """float64 [n_orders][len]: entry [o][i] = the estimate of the union of the resident rows orders[o][0 .. i]; with
        want_hist also uint32 [n_orders][len][64], the register histograms of those unions.  A 1-D order gives 1-D results."""
        ords = np.ascontiguousarray(orders, np.uint32)
        assert ords.ndim in (1, 2)
        flat = ords.reshape(1, -1) if ords.ndim == 1 else ords
        n_orders, length = flat.shape
        card = np.zeros((n_orders, length), np.float64)
        hist = np.zeros((n_orders, length, CURVE_BINS), np.uint32) if want_hist else None
        self._ck(self._derive("dsh_union_curve")(self._h, estim, flat.ctypes.data, length, n_orders, card.ctypes.data,
                                                 hist.ctypes.data if want_hist else None))
        if ords.ndim == 1:
            card, hist = card[0], (hist[0] if want_hist else None)
        return (card, hist) if want_hist else card

    def union_curve_device(self, orders_ptr, length, n_orders, card_ptr, hist_ptr=None, estim=ESTIM_ERTL_MLE):
        self._ck(self._derive("dsh_union_curve_device")(self._h, estim, C.c_void_p(orders_ptr), length, n_orders, C.c_void_p(card_ptr),
                                                        C.c_void_p(hist_ptr) if hist_ptr else None))

    # ---- sketch waist
    def sketch_batch(self, seq, genome_off, first_slot=0, k=31, canon=True, want_regs=True):
        seq = np.ascontiguousarray(seq, np.uint8)
        off = np.ascontiguousarray(genome_off, np.uint64)
        ng = off.size - 1
        out = np.zeros((ng, 1 << self.p), np.uint8) if want_regs else None
        self._ck(self._lib.dsh_sketch_batch(
            self._h, seq.ctypes.data if seq.size else None, off.ctypes.data, ng, first_slot, k,
            int(bool(canon)), out.ctypes.data if want_regs else None))
        return out

    def sketch_batch_async(self, seq_pinned, genome_off, first_slot=0, k=31, canon=True):
        """seq_pinned: numpy view of PinnedArray memory; complete after wait()"""
        off = np.ascontiguousarray(genome_off, np.uint64)
        self._ck(self._lib.dsh_sketch_batch_async(
            self._h, seq_pinned.ctypes.data, off.ctypes.data, off.size - 1, first_slot, k, int(bool(canon))))

    def sketch_fastx_batch(self, files, first_slot=0, k=31, canon=True):
        """files: one bytes object per genome, the raw text of a plain FASTA file (dsh_sketch_fastx_batch_async: the
        parse runs on the device).  Returns the per-genome status words (0 = decoded and sketched; != 0 = refused, nothing
        sketched: not plain FASTA) after waiting."""
        ng = len(files)
        off = np.zeros(ng + 1, np.uint64)
        lens = np.array([len(f) for f in files], np.uint64)
        for g in range(ng):
            off[g + 1] = off[g] + ((int(lens[g]) + 1 + 31) & ~31)
        raw = np.full(max(int(off[-1]), 1), 0x4E, np.uint8)
        for g, f in enumerate(files):
            raw[int(off[g]): int(off[g]) + len(f)] = np.frombuffer(f, np.uint8)
        status = np.zeros(max(ng, 1), np.uint32)
        self._ck(self._lib.dsh_sketch_fastx_batch_async(
            self._h, raw.ctypes.data, off.ctypes.data, lens.ctypes.data, ng, first_slot, k, int(bool(canon)), status.ctypes.data))
        self.wait()
        return status[:ng]

    @staticmethod
    def _fastx_regions(files):
        """the raw buffer of the fastx entry points: every file in a region of its own that starts on a multiple of 32"""
        ng = len(files)
        off = np.zeros(ng + 1, np.uint64)
        lens = np.array([len(f) for f in files], np.uint64).reshape(ng)
        for g in range(ng):
            off[g + 1] = off[g] + ((int(lens[g]) + 1 + 31) & ~31)
        raw = np.full(max(int(off[-1]), 1), 0x4E, np.uint8)
        for g, f in enumerate(files):
            raw[int(off[g]): int(off[g]) + len(f)] = np.frombuffer(f, np.uint8)
        return raw, off, lens

    def sketch_fastx_records(self, files, slot_ptr=None, k=31, canon=True):
        """Per-record sketches of raw FASTA / FASTQ texts, parsed on the device (dsh_sketch_fastx_records).  files: one
        bytes object per file; slot_ptr[len(files) + 1]: file f owns the rows [slot_ptr[f], slot_ptr[f + 1]), its record
        r goes to row slot_ptr[f] + r.  Returns (status, n_rec, names): status[f] != 0 = refused (no row written, n_rec[f] =
        0: parse it on the host and use sketch_records), n_rec[f] = the file's records, names = one bytes object per slot
        of the span (b"" for the slots of a refused file).  slot_ptr None: count only -- nothing is sketched, names is
        None, and no matrix is needed.  A count that differs from its span raises DshError with code ERANGE, the
        complete counts in its attribute n_rec and the status words in status; no row was written."""
        nf = len(files)
        raw, off, lens = self._fastx_regions(files)
        status = np.zeros(max(nf, 1), np.uint32)
        n_rec = np.zeros(max(nf, 1), np.uint64)
        sp = hdr = None
        if slot_ptr is not None:
            sp = np.ascontiguousarray(slot_ptr, np.uint64).reshape(-1)
            assert sp.size == nf + 1
            hdr = np.zeros(max(int(sp[-1]) - int(sp[0]), 1) if sp[-1] >= sp[0] else 1, np.uint64)
        rc = self._lib.dsh_sketch_fastx_records(
            self._h, raw.ctypes.data, off.ctypes.data, lens.ctypes.data, nf, sp.ctypes.data if sp is not None else None, k,
            int(bool(canon)), status.ctypes.data, n_rec.ctypes.data, hdr.ctypes.data if hdr is not None else None)
        if rc == ERANGE:
            err = DshError(rc, self._lib.dsh_last_error(self._h).decode())
            err.n_rec, err.status = n_rec[:nf].copy(), status[:nf].copy()
            raise err
        self._ck(rc)
        if sp is None:
            return status[:nf], n_rec[:nf], None
        buf = raw.tobytes()
        names = [b""] * (int(sp[-1]) - int(sp[0]))
        for f in range(nf):
            end = int(off[f]) + int(lens[f])
            for r in range(int(n_rec[f])):
                e = int(sp[f]) - int(sp[0]) + r
                names[e] = _NAME.match(buf, int(hdr[e]) + 1, end).group()
        return status[:nf], n_rec[:nf], names

    def count_fastx_records(self, files):
        """(status, n_rec) of sketch_fastx_records in count-only mode: the early refusals and every file's record count"""
        status, n_rec, _ = self.sketch_fastx_records(files, None)
        return status, n_rec

    def sketch_batch_device(self, seq_ptr, genome_off, first_slot=0, k=31, canon=True):
        off = np.ascontiguousarray(genome_off, np.uint64)
        self._ck(self._lib.dsh_sketch_batch_device(
            self._h, C.c_void_p(seq_ptr), off.ctypes.data, off.size - 1, first_slot, k, int(bool(canon))))

    # ---- per-record sketches (dsh_sketch_records*): record r = seq[rec_off[r]:rec_off[r+1]], no separators, its row is
    # OVERWRITTEN with the record's own registers (all zero for a record shorter than k)
    def sketch_records(self, seq, rec_off, first_slot=0, k=31, canon=True, want_regs=True):
        seq = np.ascontiguousarray(seq, np.uint8)
        off = np.ascontiguousarray(rec_off, np.uint64)
        nr = off.size - 1
        out = np.zeros((nr, 1 << self.p), np.uint8) if want_regs else None
        self._ck(self._lib.dsh_sketch_records(
            self._h, seq.ctypes.data if seq.size else None, off.ctypes.data, nr, first_slot, k,
            int(bool(canon)), out.ctypes.data if want_regs else None))
        return out

    def sketch_records_async(self, seq_pinned, rec_off, first_slot=0, k=31, canon=True):
        """seq_pinned: numpy view of PinnedArray memory; complete after wait()"""
        off = np.ascontiguousarray(rec_off, np.uint64)
        self._ck(self._lib.dsh_sketch_records_async(
            self._h, seq_pinned.ctypes.data, off.ctypes.data, off.size - 1, first_slot, k, int(bool(canon))))

    def sketch_records_device(self, seq_ptr, rec_off, first_slot=0, k=31, canon=True):
        off = np.ascontiguousarray(rec_off, np.uint64)
        self._ck(self._lib.dsh_sketch_records_device(
            self._h, C.c_void_p(seq_ptr), off.ctypes.data, off.size - 1, first_slot, k, int(bool(canon))))

    # ---- compare waist
    def cardinalities(self, estim=ESTIM_ERTL_MLE):
        out = np.zeros(max(self.n, 1), np.float64)
        self._ck(self._lib.dsh_cardinalities(self._h, estim, out.ctypes.data))
        return out[: self.n]

    def dist_rows(self, row_begin=0, row_end=None, estim=ESTIM_ERTL_MLE, result_type=JI, k=31, out=None):
        row_end = self.n if row_end is None else row_end
        span = tri_span(self.n, row_begin, row_end)
        if out is None:
            out = np.zeros(max(span, 1), np.float32)
        self._ck(self._lib.dsh_dist_rows(self._h, estim, result_type, k, row_begin, row_end, out.ctypes.data))
        return out[:span]

    def dist_rows_device(self, out_ptr, row_begin=0, row_end=None, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        row_end = self.n if row_end is None else row_end
        self._ck(self._lib.dsh_dist_rows_device(self._h, estim, result_type, k, row_begin, row_end, C.c_void_p(out_ptr)))

    def dist_rows_async(self, out_pinned, row_begin=0, row_end=None, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """enqueue rows -> `out_pinned` (numpy view of PinnedArray memory); valid after wait()"""
        row_end = self.n if row_end is None else row_end
        assert out_pinned.size >= tri_span(self.n, row_begin, row_end)
        self._ck(self._lib.dsh_dist_rows_async(self._h, estim, result_type, k, row_begin, row_end, out_pinned.ctypes.data))

    def dist_rows_device_async(self, out_ptr, row_begin=0, row_end=None, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        row_end = self.n if row_end is None else row_end
        self._ck(self._lib.dsh_dist_rows_device_async(self._h, estim, result_type, k, row_begin, row_end, C.c_void_p(out_ptr)))

    def wait(self):
        self._ck(self._lib.dsh_wait(self._h))

    def event_record(self):
        """ticket marking everything enqueued on this context so far"""
        t = C.c_uint64()
        self._ck(self._lib.dsh_event_record(self._h, C.byref(t)))
        return int(t.value)

    def event_wait(self, ticket):
        self._ck(self._lib.dsh_event_wait(self._h, ticket))

    def event_done(self, ticket):
        d = C.c_int()
        self._ck(self._lib.dsh_event_query(self._h, ticket, C.byref(d)))
        return bool(d.value)

    def wait_event(self, hip_event):
        """order the ctx stream after a caller event (e.g. torch.cuda.Event().cuda_event, recorded on torch's stream)"""
        self._ck(self._lib.dsh_wait_event(self._h, C.c_void_p(hip_event)))

    def dist_rect(self, q_begin, q_end, r_begin, r_end, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        out = np.zeros((max(q_end - q_begin, 0), max(r_end - r_begin, 0)), np.float32)
        buf = out if out.size else np.zeros(1, np.float32)
        self._ck(self._lib.dsh_dist_rect(self._h, estim, result_type, k, q_begin, q_end, r_begin, r_end, buf.ctypes.data))
        return out

    def knn(self, nn, q_begin=0, q_end=None, r_begin=0, r_end=None, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        q_end = self.n if q_end is None else q_end
        r_end = self.n if r_end is None else r_end
        nq = max(q_end - q_begin, 0)
        idx = np.zeros((nq, nn), np.uint32)
        val = np.zeros((nq, nn), np.float32)
        if nq and nn:
            self._ck(self._lib.dsh_knn(self._h, estim, result_type, k, q_begin, q_end, r_begin, r_end, nn,
                                       idx.ctypes.data, val.ctypes.data))
        return idx, val

    # ---- thresholded output (CSR of the pairs that pass; include/dashing_hip.h has the contract)
    def _take_hits(self, colp, valp, nh):
        """numpy copies of the library-allocated col/val, which are released here"""
        try:
            col = np.ctypeslib.as_array(C.cast(colp, C.POINTER(C.c_uint32)), (nh,)).copy() if nh else np.zeros(0, np.uint32)
            val = np.ctypeslib.as_array(C.cast(valp, C.POINTER(C.c_float)), (nh,)).copy() if nh else np.zeros(0, np.float32)
        finally:
            self._lib.dsh_free_host(colp)
            self._lib.dsh_free_host(valp)
        return col, val

    def dist_threshold(self, threshold, row_begin=0, row_end=None, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """(row_ptr uint64 [rows + 1], col uint32, val float32): the pairs (i, j > i) of rows [row_begin, row_end) whose
        value passes `threshold` (similarities v >= t, distances v <= t), rows and columns ascending"""
        row_end = self.n if row_end is None else min(row_end, self.n)
        rows = max(row_end - row_begin, 0)
        row_ptr = np.zeros(rows + 1, np.uint64)
        colp, valp, nh = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._ck(self._lib.dsh_dist_threshold(self._h, estim, result_type, k, row_begin, row_end, threshold,
                                              row_ptr.ctypes.data, C.byref(colp), C.byref(valp), C.byref(nh)))
        col, val = self._take_hits(colp, valp, int(nh.value))
        return row_ptr, col, val

    def dist_threshold_count(self, threshold, row_begin=0, row_end=None, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """row_ptr alone (counts only: nothing is emitted)"""
        row_end = self.n if row_end is None else min(row_end, self.n)
        row_ptr = np.zeros(max(row_end - row_begin, 0) + 1, np.uint64)
        nh = C.c_uint64()
        self._ck(self._lib.dsh_dist_threshold(self._h, estim, result_type, k, row_begin, row_end, threshold,
                                              row_ptr.ctypes.data, None, None, C.byref(nh)))
        return row_ptr

    def dist_threshold_device(self, row_ptr_ptr, col_ptr, val_ptr, cap, threshold, row_begin=0, row_end=None,
                              estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """device buffers of the caller (row_ptr [rows + 1] uint64, col / val of `cap` entries); returns n_hits.  If the
        hits do not fit, raises DshError with code ERANGE and the true count in its attribute n_hits: row_ptr is complete
        and the first `cap` hits are written."""
        row_end = self.n if row_end is None else row_end
        nh = C.c_uint64()
        rc = self._lib.dsh_dist_threshold_device(self._h, estim, result_type, k, row_begin, row_end, threshold,
                                                 C.c_void_p(row_ptr_ptr), C.c_void_p(col_ptr), C.c_void_p(val_ptr), cap, C.byref(nh))
        if rc:
            err = DshError(rc, self._lib.dsh_last_error(self._h).decode())
            if rc == ERANGE:
                err.n_hits = int(nh.value)
            raise err
        return int(nh.value)

    def dist_rect_threshold(self, threshold, q_begin, q_end, r_begin, r_end, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """as dist_threshold for the rectangle of dist_rect: one row per query, col = reference slot"""
        row_ptr = np.zeros(max(q_end - q_begin, 0) + 1, np.uint64)
        colp, valp, nh = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._ck(self._lib.dsh_dist_rect_threshold(self._h, estim, result_type, k, q_begin, q_end, r_begin, r_end, threshold,
                                                   row_ptr.ctypes.data, C.byref(colp), C.byref(valp), C.byref(nh)))
        col, val = self._take_hits(colp, valp, int(nh.value))
        return row_ptr, col, val

    # ---- an explicit list of pairs (include/dashing_hip.h has the contract)
    @staticmethod
    def _types(result_types):
        return np.ascontiguousarray(np.atleast_1d(np.asarray(result_types, np.int32)).reshape(-1))

    def dist_pairs(self, lhs, rhs, result_types=(JI,), estim=ESTIM_ERTL_MLE, k=31):
        """float32 [n_types][n_pairs]: out[t][x] = result_cmp(lhs = sketch lhs[x], rhs = sketch rhs[x], result_types[t]),
        bit for bit the value of dist_rows at (i = rhs, j = lhs > i) and of dist_rect at [query = rhs][reference = lhs]"""
        lhs = np.ascontiguousarray(lhs, np.uint32).reshape(-1)
        rhs = np.ascontiguousarray(rhs, np.uint32).reshape(-1)
        if lhs.size != rhs.size:
            raise ValueError("lhs and rhs differ in length")
        ty = self._types(result_types)
        out = np.zeros((ty.size, lhs.size), np.float32)
        self._ck(self._lib.dsh_dist_pairs(self._h, estim, ty.ctypes.data, ty.size, k, lhs.ctypes.data, rhs.ctypes.data,
                                          lhs.size, out.ctypes.data))
        return out

    def dist_pairs_device(self, lhs_ptr, rhs_ptr, n_pairs, out_ptr, result_types=(JI,), estim=ESTIM_ERTL_MLE, k=31):
        """device buffers of the caller: lhs / rhs uint32 [n_pairs], out float32 [n_types][n_pairs]"""
        ty = self._types(result_types)
        self._ck(self._lib.dsh_dist_pairs_device(self._h, estim, ty.ctypes.data, ty.size, k, C.c_void_p(lhs_ptr),
                                                 C.c_void_p(rhs_ptr), n_pairs, C.c_void_p(out_ptr)))

    def dist_pairs_csr(self, row_ptr, col, row_begin=0, result_types=(JI,), estim=ESTIM_ERTL_MLE, k=31):
        """the hits of dist_threshold / dist_rect_threshold again: hit h of row r is (lhs = col[h], rhs = row_begin + r);
        float32 [n_types][n_hits]"""
        row_ptr = np.ascontiguousarray(row_ptr, np.uint64).reshape(-1)
        col = np.ascontiguousarray(col, np.uint32).reshape(-1)
        if row_ptr.size < 1:
            raise ValueError("row_ptr holds rows + 1 entries")
        rows = row_ptr.size - 1
        nh = int(row_ptr[-1]) - int(row_ptr[0])
        if nh > 0 and int(row_ptr[-1]) > col.size:
            raise ValueError("col is shorter than row_ptr says")
        ty = self._types(result_types)
        out = np.zeros((ty.size, max(nh, 0)), np.float32)
        self._ck(self._lib.dsh_dist_pairs_csr(self._h, estim, ty.ctypes.data, ty.size, k, row_begin, rows, row_ptr.ctypes.data,
                                              col.ctypes.data, out.ctypes.data))
        return out

    # ---- clusters: connected components on the device (include/dashing_hip.h has the contract)
    def cluster_threshold(self, threshold, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """(labels uint32 [n], n_clusters): labels[x] = the smallest slot of x's connected component in the graph of the
        hits of dist_threshold(threshold, ...) over all rows"""
        labels = np.zeros(self.n, np.uint32)
        nc = C.c_uint64()
        self._ck(self._derive("dsh_cluster_threshold")(self._h, estim, result_type, k, threshold, labels.ctypes.data, C.byref(nc)))
        return labels, int(nc.value)

    def cluster_threshold_device(self, labels_ptr, threshold, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """labels into the caller's device buffer (uint32 [n]); returns n_clusters"""
        nc = C.c_uint64()
        self._ck(self._derive("dsh_cluster_threshold_device")(self._h, estim, result_type, k, threshold, C.c_void_p(labels_ptr), C.byref(nc)))
        return int(nc.value)

    # ---- single-, complete- and average-linkage clusters at a threshold (include/dashing_hip.h has the contract)
    _LINKAGES = {"single": LINKAGE_SINGLE, "complete": LINKAGE_COMPLETE, "average": LINKAGE_AVERAGE}

    @classmethod
    def _linkage(cls, linkage):
        """a name, or the number as it is (the library refuses an unknown one)"""
        if isinstance(linkage, str):
            if linkage not in cls._LINKAGES:
                raise ValueError("linkage is 'single', 'complete' or 'average', got %r" % (linkage,))
            return cls._LINKAGES[linkage]
        return int(linkage)

    def linkage_threshold(self, threshold, linkage="complete", estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """(labels uint32 [n], n_clusters): labels[x] = the smallest slot of x's cluster after agglomerating, best pair
        first, while a pair of clusters passes the threshold under the linkage"""
        labels = np.zeros(self.n, np.uint32)
        nc = C.c_uint64()
        self._ck(self._derive("dsh_linkage_threshold")(self._h, estim, result_type, k, threshold, self._linkage(linkage),
                                                       labels.ctypes.data if labels.size else None, C.byref(nc)))
        return labels, int(nc.value)

    def linkage_threshold_device(self, labels_ptr, threshold, linkage="complete", estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """labels into the caller's device buffer (uint32 [n]); returns n_clusters"""
        nc = C.c_uint64()
        self._ck(self._derive("dsh_linkage_threshold_device")(self._h, estim, result_type, k, threshold, self._linkage(linkage),
                                                              C.c_void_p(labels_ptr), C.byref(nc)))
        return int(nc.value)

    def linkage_tri(self, n_nodes, tri, threshold, linkage, descending=False):
        """(labels, n_clusters) for a caller's values: tri holds n_nodes (n_nodes - 1) / 2 float32 in dsh_tri_index order
        (np.triu_indices(n_nodes, 1)).  Needs no sketches."""
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1)
        n_nodes = int(n_nodes)
        if n_nodes >= 0 and tri.size != n_nodes * (n_nodes - 1) // 2:
            raise ValueError("tri holds n_nodes (n_nodes - 1) / 2 values")
        labels = np.zeros(max(n_nodes, 0), np.uint32)
        nc = C.c_uint64()
        self._ck(self._derive("dsh_linkage_tri")(self._h, n_nodes, tri.ctypes.data if tri.size else None, 1 if descending else 0,
                                                 threshold, self._linkage(linkage), labels.ctypes.data if labels.size else None,
                                                 C.byref(nc)))
        return labels, int(nc.value)

    # ---- the minimum spanning tree of the pair values: the single-linkage dendrogram (include/dashing_hip.h has the contract)
    def _mst(self, name, n, head, descending, cutoff, labels):
        if cutoff is None:  # no cutoff: every value that is not NaN is an edge
            cutoff = -np.inf if descending else np.inf
        m = max(n - 1, 0)
        lhs, rhs, val = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.float32)
        lab = np.zeros(n, np.uint32) if labels else None
        ne = C.c_uint64()
        self._ck(self._derive(name)(self._h, *head, cutoff, lhs.ctypes.data if m else None, rhs.ctypes.data if m else None,
                                    val.ctypes.data if m else None, C.byref(ne), lab.ctypes.data if labels and n else None))
        e = int(ne.value)
        return (lhs[:e], rhs[:e], val[:e]) + ((lab,) if labels else ())

    def mst(self, cutoff=None, estim=ESTIM_ERTL_MLE, result_type=JI, k=31, labels=False):
        """(lhs, rhs, val[, labels]): the best spanning forest of the pairs whose value passes `cutoff` (None: all that are not
        NaN), edges lhs < rhs sorted best first -- better value, then smaller lhs, then smaller rhs; labels = what
        cluster_threshold(cutoff) gives"""
        return self._mst("dsh_mst", self.n, (estim, result_type, k), result_type not in DISTANCE_TYPES, cutoff, labels)

    def mst_tri(self, tri, descending, cutoff=None, labels=False, n_nodes=None):
        """the same for a caller's values: tri holds n (n - 1) / 2 float32 in dsh_tri_index order (np.triu_indices(n, 1)); n is
        taken from its size (n_nodes tells one node from none: both have an empty triangle).  Needs no sketches."""
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1)
        n = (1 + math.isqrt(1 + 8 * tri.size)) // 2 if tri.size else 0
        if n_nodes is not None:
            n = int(n_nodes)
        if n < 0 or n * (n - 1) // 2 != tri.size:
            raise ValueError("tri holds n (n - 1) / 2 values")
        return self._mst("dsh_mst_tri", n, (n, tri.ctypes.data if tri.size else None, 1 if descending else 0), descending, cutoff, labels)

    # ---- density clusters at a threshold and the degrees of the threshold graph (include/dashing_hip.h has the contract)
    @staticmethod
    def _dbscan_args(min_pts, assign):
        mode = {"first": GREEDY_FIRST, "best": GREEDY_BEST}.get(assign, assign)
        if mode not in (GREEDY_FIRST, GREEDY_BEST) or isinstance(mode, bool):
            raise ValueError("assign is 'first' or 'best', got %r" % (assign,))
        min_pts = int(min_pts)
        if not 0 <= min_pts <= 0xFFFFFFFF:  # (0 is the library's to refuse)
            raise ValueError("min_pts is a uint32")
        return min_pts, mode

    def _dbscan(self, name, n, head, threshold, min_pts, assign):
        min_pts, mode = self._dbscan_args(min_pts, assign)
        labels, kind, degree = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        nc, nn = C.c_uint64(), C.c_uint64()
        self._ck(self._derive(name)(self._h, *head, threshold, min_pts, mode, labels.ctypes.data if n else None,
                                    kind.ctypes.data if n else None, degree.ctypes.data if n else None, C.byref(nc), C.byref(nn)))
        return labels, kind, degree, int(nc.value), int(nn.value)

    def dbscan_threshold(self, threshold, min_pts, assign="first", estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """(labels uint32 [n], kind uint8 [n], degree uint32 [n], n_clusters, n_noise): DBSCAN over the graph of the hits of
        dist_threshold(threshold, ...).  x is a core (DBSCAN_CORE) iff degree[x] + 1 >= min_pts; the clusters are the components
        of the core-core edges, labelled with their smallest core; a non-core with a core neighbour is a border and goes to the
        smallest ("first") or the best-valued ("best"; ties to the smallest) of them; the rest is noise, labelled with itself"""
        return self._dbscan("dsh_dbscan_threshold", self.n, (estim, result_type, k), threshold, min_pts, assign)

    def dbscan_threshold_device(self, labels_ptr, threshold, min_pts, assign="first", kind_ptr=None, degree_ptr=None,
                                estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """labels (uint32 [n]) and, where given, kind (uint8 [n]) and degree (uint32 [n]) into the caller's device buffers;
        returns (n_clusters, n_noise)"""
        min_pts, mode = self._dbscan_args(min_pts, assign)
        nc, nn = C.c_uint64(), C.c_uint64()
        self._ck(self._derive("dsh_dbscan_threshold_device")(self._h, estim, result_type, k, threshold, min_pts, mode, C.c_void_p(labels_ptr),
                                                             C.c_void_p(kind_ptr), C.c_void_p(degree_ptr), C.byref(nc), C.byref(nn)))
        return int(nc.value), int(nn.value)

    def dbscan_tri(self, tri, descending, threshold, min_pts, assign="first", n_nodes=None):
        """the same for a caller's values: tri holds n (n - 1) / 2 float32 in dsh_tri_index order (np.triu_indices(n, 1)); n is
        taken from its size (n_nodes tells one node from none: both have an empty triangle).  Needs no sketches."""
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1)
        n = (1 + math.isqrt(1 + 8 * tri.size)) // 2 if tri.size else 0
        if n_nodes is not None:
            n = int(n_nodes)
        if n < 0 or n * (n - 1) // 2 != tri.size:
            raise ValueError("tri holds n (n - 1) / 2 values")
        return self._dbscan("dsh_dbscan_tri", n, (n, tri.ctypes.data if tri.size else None, 1 if descending else 0), threshold, min_pts, assign)

    def degree_threshold(self, threshold, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """degree uint32 [n]: how many hits of dist_threshold(threshold, ...) each slot is an end of"""
        degree = np.zeros(self.n, np.uint32)
        self._ck(self._derive("dsh_degree_threshold")(self._h, estim, result_type, k, threshold, degree.ctypes.data if degree.size else None))
        return degree

    def degree_threshold_device(self, degree_ptr, threshold, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """the degrees into the caller's device buffer (uint32 [n])"""
        self._ck(self._derive("dsh_degree_threshold_device")(self._h, estim, result_type, k, threshold, C.c_void_p(degree_ptr)))

    # ---- greedy representatives in slot order (include/dashing_hip.h has the contract)
    def greedy_threshold(self, threshold, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """(labels uint32 [n], n_reps): x is a representative (labels[x] == x) iff no earlier representative hits it in
        the graph of the hits of dist_threshold(threshold, ...); every other slot gets its smallest such representative"""
        labels = np.zeros(self.n, np.uint32)
        nr = C.c_uint64()
        self._ck(self._derive("dsh_greedy_threshold")(self._h, estim, result_type, k, threshold, labels.ctypes.data, C.byref(nr)))
        return labels, int(nr.value)

    def greedy_threshold_device(self, labels_ptr, threshold, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """labels into the caller's device buffer (uint32 [n]); returns n_reps"""
        nr = C.c_uint64()
        self._ck(self._derive("dsh_greedy_threshold_device")(self._h, estim, result_type, k, threshold, C.c_void_p(labels_ptr), C.byref(nr)))
        return int(nr.value)

    # ---- the same behind a labelling of the first slots; first or best representative
    @staticmethod
    def _extend_args(first_new, labels_in, assign):
        mode = {"first": GREEDY_FIRST, "best": GREEDY_BEST}.get(assign, assign)
        if mode not in (GREEDY_FIRST, GREEDY_BEST) or isinstance(mode, bool):
            raise ValueError("assign is 'first' or 'best', got %r" % (assign,))
        if first_new < 0:
            raise ValueError("first_new is negative")
        li = None
        if labels_in is not None:
            li = np.ascontiguousarray(labels_in, np.uint32).reshape(-1)
            if li.size != first_new:
                raise ValueError("labels_in holds one label per slot below first_new")
        # (first_new > 0 without labels_in, and labels_in of length 0 with first_new == 0: the library's own rule decides)
        return mode, li, (li.ctypes.data if li is not None and li.size else None)

    def greedy_extend(self, threshold, first_new=0, labels_in=None, assign="first", estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """(labels uint32 [n], n_reps): the slots below first_new keep labels_in (their representatives are taken as
        given), every later slot is a representative iff no representative before it hits it, else it goes to the smallest
        ("first") or to the best-valued ("best"; ties to the smallest) representative that hits it"""
        mode, li, lip = self._extend_args(first_new, labels_in, assign)
        labels = np.zeros(self.n, np.uint32)
        nr = C.c_uint64()
        self._ck(self._derive("dsh_greedy_extend")(self._h, estim, result_type, k, threshold, mode, first_new, lip,
                                                   labels.ctypes.data if labels.size else None, C.byref(nr)))
        return labels, int(nr.value)

    def greedy_extend_device(self, labels_ptr, threshold, first_new=0, labels_in=None, assign="first", estim=ESTIM_ERTL_MLE,
                             result_type=JI, k=31):
        """labels into the caller's device buffer (uint32 [n]); labels_in stays a host array; returns n_reps"""
        mode, li, lip = self._extend_args(first_new, labels_in, assign)
        nr = C.c_uint64()
        self._ck(self._derive("dsh_greedy_extend_device")(self._h, estim, result_type, k, threshold, mode, first_new, lip,
                                                          C.c_void_p(labels_ptr), C.byref(nr)))
        return int(nr.value)

    # ---- statistics of a labelling: counts, sums, worst values, medoids (include/dashing_hip.h has the contract)
    _ROUTES = {"auto": -1, "dense": 0, "pairs": 1}

    def _stats_call(self, name, labels, estim, result_type, k, route, ptrs):
        if route not in self._ROUTES:
            raise ValueError("route is 'auto', 'dense' or 'pairs', got %r" % (route,))
        lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
        if lab.size != self.n:
            raise ValueError("labels holds one label per sketch")
        # "auto" leaves the context's "stats_route" option as it is; a named route holds for this call alone
        if route != "auto":
            self.set_option("stats_route", self._ROUTES[route])
        try:
            self._ck(self._derive(name)(self._h, estim, result_type, k, lab.ctypes.data if lab.size else None, *ptrs))
        finally:
            if route != "auto":
                self.set_option("stats_route", -1)
        return lab

    def group_stats(self, labels, estim=ESTIM_ERTL_MLE, result_type=JI, k=31, route="auto"):
        """GroupStats(medoid, cnt, sum, worst) of the groups of equal labels (any values < n), with .mean and .diameter.
        No result depends on route ('auto' | 'dense' | 'pairs')."""
        n = self.n
        med, cnt, sm, worst = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int64), np.zeros(n, np.float32)
        lab = self._stats_call("dsh_group_stats", labels, estim, result_type, k, route,
                               [a.ctypes.data if n else None for a in (med, cnt, sm, worst)])
        return GroupStats(med, cnt, sm, worst, lab, result_type in SIMILARITY_TYPES)

    def group_stats_device(self, labels, medoid_ptr, cnt_ptr, sum_ptr, worst_ptr, estim=ESTIM_ERTL_MLE, result_type=JI, k=31,
                           route="auto"):
        """the same into the caller's device buffers (uint32, uint32, int64, float32, [n] each; 0 / None: not wanted);
        labels stays a host array"""
        self._stats_call("dsh_group_stats_device", labels, estim, result_type, k, route,
                         [C.c_void_p(p) if p else None for p in (medoid_ptr, cnt_ptr, sum_ptr, worst_ptr)])

    # ---- value histograms over caller-given edges (include/dashing_hip.h has the contract)
    _NO_LABELS = np.zeros(1, np.uint32)  # what an empty labelling points at: two planes are asked for, nothing is read

    def _hist_args(self, edges, labels):
        """(edges float32, their pointer, labels pointer or None, planes)"""
        e = np.ascontiguousarray(edges, np.float32).reshape(-1)
        if labels is None:
            return e, (e.ctypes.data if e.size else None), None, None, 1
        lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
        if lab.size != self.n:
            raise ValueError("labels holds one label per sketch")
        keep = lab if lab.size else self._NO_LABELS
        return e, (e.ctypes.data if e.size else None), keep, keep.ctypes.data, 2

    def dist_histogram(self, edges, row_begin=0, row_end=None, labels=None, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """uint64 (planes, n_edges + 2): how many values of dist_rows over rows [row_begin, row_end) fall into each class of
        the strictly increasing float32 `edges` -- class(v) = the number of edges that pass v as a threshold would
        (similarities e <= v, distances e < v), NaN the last class.  labels (one per slot): plane 0 counts the pairs with
        equal labels, plane 1 the others; without labels one plane.  histogram_hits() turns it into hit counts per edge."""
        row_end = self.n if row_end is None else row_end
        e, ep, _keep, labp, planes = self._hist_args(edges, labels)
        out = np.zeros((planes, e.size + 2), np.uint64)
        self._ck(self._derive("dsh_dist_histogram")(self._h, estim, result_type, k, row_begin, row_end, ep, e.size, labp, out.ctypes.data))
        return out

    def dist_histogram_device(self, counts_ptr, edges, row_begin=0, row_end=None, labels=None, estim=ESTIM_ERTL_MLE, result_type=JI,
                              k=31):
        """the same into the caller's device buffer (uint64 [planes][n_edges + 2], 8-byte aligned, overwritten); edges and
        labels stay host arrays"""
        row_end = self.n if row_end is None else row_end
        e, ep, _keep, labp, _ = self._hist_args(edges, labels)
        self._ck(self._derive("dsh_dist_histogram_device")(self._h, estim, result_type, k, row_begin, row_end, ep, e.size, labp,
                                                           C.c_void_p(counts_ptr) if counts_ptr else None))

    def dist_rect_histogram(self, edges, q_begin, q_end, r_begin, r_end, labels=None, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """as dist_histogram for the values of dist_rect (query slots x reference slots, self pairs included)"""
        e, ep, _keep, labp, planes = self._hist_args(edges, labels)
        out = np.zeros((planes, e.size + 2), np.uint64)
        self._ck(self._derive("dsh_dist_rect_histogram")(self._h, estim, result_type, k, q_begin, q_end, r_begin, r_end, ep, e.size,
                                                         labp, out.ctypes.data))
        return out

    @staticmethod
    def _labels_in(n_nodes, labels_in):
        if labels_in is None:
            return None
        li = np.ascontiguousarray(labels_in, np.uint32).reshape(-1)
        if li.size != n_nodes:
            raise ValueError("labels_in holds one label per node")
        return li

    def cluster_pairs(self, n_nodes, lhs, rhs, labels_in=None):
        """(labels, n_clusters) of the graph on n_nodes nodes with the edges (lhs[x], rhs[x]); labels_in: an earlier
        labelling to continue from.  Needs no sketches."""
        lhs = np.ascontiguousarray(lhs, np.uint32).reshape(-1)
        rhs = np.ascontiguousarray(rhs, np.uint32).reshape(-1)
        if lhs.size != rhs.size:
            raise ValueError("lhs and rhs differ in length")
        li = self._labels_in(n_nodes, labels_in)
        labels = np.zeros(max(int(n_nodes), 0), np.uint32)
        nc = C.c_uint64()
        self._ck(self._derive("dsh_cluster_pairs")(self._h, n_nodes, lhs.ctypes.data, rhs.ctypes.data, lhs.size,
                                                   None if li is None else li.ctypes.data, labels.ctypes.data, C.byref(nc)))
        return labels, int(nc.value)

    def cluster_csr(self, n_nodes, row_ptr, col, row_begin=0, labels_in=None):
        """as cluster_pairs for the hits of dist_threshold / dist_rect_threshold: hit h of row r is the edge
        (row_begin + r, col[h])"""
        row_ptr = np.ascontiguousarray(row_ptr, np.uint64).reshape(-1)
        col = np.ascontiguousarray(col, np.uint32).reshape(-1)
        if row_ptr.size < 1:
            raise ValueError("row_ptr holds rows + 1 entries")
        if int(row_ptr[-1]) > int(row_ptr[0]) and int(row_ptr[-1]) > col.size:
            raise ValueError("col is shorter than row_ptr says")
        li = self._labels_in(n_nodes, labels_in)
        labels = np.zeros(max(int(n_nodes), 0), np.uint32)
        nc = C.c_uint64()
        self._ck(self._derive("dsh_cluster_csr")(self._h, n_nodes, row_begin, row_ptr.size - 1, row_ptr.ctypes.data, col.ctypes.data,
                                                 None if li is None else li.ctypes.data, labels.ctypes.data, C.byref(nc)))
        return labels, int(nc.value)

    # ---- multi-GPU shards (sorted-order spans + one un-permute)
    def shard_plan(self, nshards, estim=ESTIM_ERTL_MLE):
        off = np.zeros(nshards + 1, np.uint64)
        self._ck(self._lib.dsh_shard_plan(self._h, estim, nshards, off.ctypes.data))
        return [int(x) for x in off]

    def dist_shard_device(self, out_ptr, shard, nshards, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        self._ck(self._lib.dsh_dist_shard_device(self._h, estim, result_type, k, shard, nshards, C.c_void_p(out_ptr)))

    def unpermute_device(self, sorted_ptr, out_ptr):
        self._ck(self._lib.dsh_unpermute_device(self._h, C.c_void_p(sorted_ptr), C.c_void_p(out_ptr)))

    def unpermute_staged_device(self, stage_ptr, stride, nshards, out_ptr):
        self._ck(self._lib.dsh_unpermute_staged_device(self._h, C.c_void_p(stage_ptr), stride, nshards, C.c_void_p(out_ptr)))

    def unpermute_blocks_device(self, stage_ptr, block_off, out_ptr):
        off = np.ascontiguousarray(block_off, np.uint64)
        self._ck(self._lib.dsh_unpermute_blocks_device(self._h, C.c_void_p(stage_ptr), off.ctypes.data, off.size, C.c_void_p(out_ptr)))

    # ---- multi-GPU exchange over RCCL inside the library (all traffic on the ctx stream)
    def comm_init(self, unique_id, rank, world):
        self._ck(self._lib.dsh_comm_init(self._h, unique_id, rank, world))

    def comm_destroy(self):
        self._ck(self._lib.dsh_comm_destroy(self._h))

    def last_part_info(self):
        """[(ready_ms, bytes)] of the parts of the last call with parts under profiling (dsh_last_part_info)"""
        k = C.c_uint32()
        self._ck(self._lib.dsh_last_part_info(self._h, None, None, 0, C.byref(k)))
        ms, fl = np.zeros(max(k.value, 1), np.float64), np.zeros(max(k.value, 1), np.uint64)
        self._ck(self._lib.dsh_last_part_info(self._h, ms.ctypes.data, fl.ctypes.data, k.value, C.byref(k)))
        return [(float(ms[q]), 4 * int(fl[q])) for q in range(k.value)]

    def finalize_phase_cycles(self):
        """per-phase cycle sums of the last call with the option finalize_timing (dsh_finalize_phase_cycles)"""
        out = np.zeros(16, np.uint64)
        self._ck(self._lib.dsh_finalize_phase_cycles(self._h, out.ctypes.data))
        return [int(x) for x in out]

    # (`rows` below: a RowSets -- balance_rowsets() -- or contiguous bounds [world + 1])
    def exchange_rows_device_async(self, out_ptr, rows, rank, nparts, dst=0, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        t = _table(self.n, rows)
        self._ck(self._lib.dsh_exchange_rows_device_async(self._h, estim, result_type, k, t.ctypes.data, rank, nparts, dst, C.c_void_p(out_ptr)))

    def exchange_collect_async(self, n, rows, nparts, local_ptr, final_ptr, dst=0):
        t = _table(n, rows)
        self._ck(self._lib.dsh_exchange_collect_async(self._h, n, t.ctypes.data, nparts, C.c_void_p(local_ptr), C.c_void_p(final_ptr), dst))

    def exchange_place_device(self, rows, src, nparts, src_local_ptr, final_ptr, dst=0):
        t = _table(self.n, rows)
        self._ck(self._lib.dsh_exchange_place_device(self._h, t.ctypes.data, src, nparts, dst, C.c_void_p(src_local_ptr), C.c_void_p(final_ptr)))

    def exchange_probe_parts_async(self, n, rows, rank, nparts, local_ptr, probe_ptr, dst=0):
        """behind every part's gate a copy KERNEL of the part's share of the rank's buffer into `probe` (diagnostic)"""
        t = _table(n, rows)
        self._ck(self._lib.dsh_exchange_probe_parts_async(self._h, n, t.ctypes.data, rank, nparts, dst, C.c_void_p(local_ptr), C.c_void_p(probe_ptr)))

    def diag_spin_start(self, nblocks, threads=256, lds_bytes=16384, max_ms=2000):
        self._ck(self._lib.dsh_diag_spin_start(self._h, nblocks, threads, lds_bytes, max_ms))

    def diag_spin_stop(self):
        self._ck(self._lib.dsh_diag_spin_stop(self._h))

    def comm_wait(self):
        """dsh_wait with a deadline on the RCCL traffic (DSH_COMM_TIMEOUT_S): an error instead of a hang"""
        self._ck(self._lib.dsh_comm_wait(self._h))

    def comm_rank(self):
        r, w = C.c_int(), C.c_int()
        rc = self._lib.dsh_comm_rank(self._h, C.byref(r), C.byref(w))
        return (r.value, w.value) if rc == 0 else None

    def collect_spans(self, n, bounds, local_ptr, final_ptr, dst=0, wait=True):
        b = np.ascontiguousarray(bounds, np.uint64)
        f = self._lib.dsh_collect_spans if wait else self._lib.dsh_collect_spans_async
        self._ck(f(self._h, n, b.ctypes.data, C.c_void_p(local_ptr), C.c_void_p(final_ptr), dst))

    def dist_rows_parts_device_async(self, out_ptr, row_begin, row_end, nparts, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        self._ck(self._lib.dsh_dist_rows_parts_device_async(self._h, estim, result_type, k, row_begin, row_end, C.c_void_p(out_ptr), nparts))

    def collect_parts_async(self, n, bounds, nparts, local_ptr, final_ptr, dst=0):
        b = np.ascontiguousarray(bounds, np.uint64)
        self._ck(self._lib.dsh_collect_parts_async(self._h, n, b.ctypes.data, nparts, C.c_void_p(local_ptr), C.c_void_p(final_ptr), dst))

    def allgather_device(self, send_ptr, bytes_per_rank, recv_ptr):
        self._ck(self._lib.dsh_allgather_device(self._h, C.c_void_p(send_ptr), bytes_per_rank, C.c_void_p(recv_ptr)))

    def dist_collect(self, bounds, dst=0, estim=ESTIM_ERTL_MLE, result_type=JI, k=31):
        """this rank's rows computed, every span delivered to `dst`; returns the packed matrix there, None elsewhere.
        bounds = None: the library partitions the rows itself (balanced row sets, the pipelined exchange pair)"""
        b = None if bounds is None else np.ascontiguousarray(bounds, np.uint64)
        me = self.comm_rank()
        out = None
        if me is None or me[0] == dst:
            out = np.zeros(max(tri_span(self.n, 0, self.n), 1), np.float32)
        self._ck(self._lib.dsh_dist_collect(self._h, estim, result_type, k, None if b is None else b.ctypes.data, dst,
                                            out.ctypes.data if out is not None else None))
        return None if out is None else out[: tri_span(self.n, 0, self.n)]

    # ---- misc
    def synchronize(self):
        self._ck(self._lib.dsh_synchronize(self._h))

    def set_profiling(self, on=True):
        self._ck(self._lib.dsh_set_profiling(self._h, int(on)))

    def last_kernel_ms(self):
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        self._ck(self._lib.dsh_last_kernel_ms(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return {"pair_ms": a.value, "finalize_ms": b.value, "prepare_ms": c.value, "pair_launches": n.value}

    def set_option(self, name, value):
        self._ck(self._lib.dsh_set_option(self._h, name.encode(), int(value)))

    def info(self, name):
        v = C.c_int64()
        self._ck(self._lib.dsh_get_info(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    @property
    def stream(self):
        return self._lib.dsh_stream(self._h)
