"""ctypes binding of libgoleft_depth.so (include/goleft_depth.h).

Fails loudly when the HIP library is missing: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(HERE, "libgoleft_depth.so")


class GdParams(C.Structure):
    _fields_ = [("window_size", C.c_int32), ("min_mapq", C.c_int32), ("min_cov", C.c_int32),
                ("max_mean_depth", C.c_int32), ("flag_mask", C.c_uint32),
                ("max_span_hint", C.c_int32), ("step", C.c_int64)]


class GdBatch(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("flag", C.c_void_p), ("mapq", C.c_void_p),
                ("cigar_off", C.c_void_p), ("cigar", C.c_void_p),
                ("reads_cap", C.c_size_t), ("ops_cap", C.c_size_t), ("slot", C.c_int32)]


class GdRun(C.Structure):
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("cls", C.c_int32)]


class GdIndexcovDims(C.Structure):
    _fields_ = [("n_tiles", C.c_int64), ("n_cells", C.c_int64), ("m", C.c_int64), ("m_pad", C.c_int64),
                ("n_samples", C.c_int32), ("n_refs", C.c_int32)]


class GdIndexCounts(C.Structure):
    _fields_ = [("records", C.c_int64), ("range_records", C.c_int64), ("runs", C.c_int64), ("n_no_coor", C.c_int64),
                ("resume", C.c_uint64), ("slices", C.c_int32), ("guesses", C.c_int32), ("rounds", C.c_int32),
                ("reserved", C.c_int32)]


class GdIndexRun(C.Structure):
    _fields_ = [("ref", C.c_int32), ("bin", C.c_uint32), ("beg", C.c_uint64), ("end", C.c_uint64)]


class GdIndexRef(C.Structure):
    _fields_ = [("first_beg", C.c_uint64), ("last_end", C.c_uint64), ("n_mapped", C.c_uint64), ("n_unmapped", C.c_uint64)]


class GdStats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_ops", C.c_uint64), ("n_ref_bases", C.c_uint64),
                ("n_windows", C.c_uint64), ("n_tiles", C.c_uint64), ("n_runs", C.c_uint64),
                ("tile_positions", C.c_int32), ("lookback", C.c_int32),
                ("max_span_seen", C.c_int32), ("reruns", C.c_int32),
                ("path", C.c_int32), ("n_slow_tiles", C.c_int32), ("n_canonical_ops", C.c_uint64),
                ("tile_kernel", C.c_int32), ("reserved_", C.c_int32), ("n_deletions", C.c_uint64)]


# every symbol include/goleft_depth.h declares: (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "gd_strerror": (C.c_char_p, [C.c_int]),
    "gd_abi_version": (C.c_int, []),
    "gd_abi_revision": (C.c_int, []),
    "gd_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "gd_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "gd_destroy": (None, [_P]),
    "gd_last_error": (C.c_char_p, [_P]),
    "gd_set_stream": (C.c_int, [_P, _P]),
    "gd_set_params": (C.c_int, [_P, C.POINTER(GdParams)]),
    "gd_default_params": (C.c_int, [C.POINTER(GdParams)]),
    "gd_set_path": (C.c_int, [_P, C.c_int]),
    "gd_set_outputs": (C.c_int, [_P, C.c_uint]),
    "gd_set_contigs": (C.c_int, [_P, C.c_int, _P]),
    "gd_select_contigs": (C.c_int, [_P, C.c_int, _P]),
    "gd_acquire": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.POINTER(GdBatch)]),
    "gd_check_commits": (C.c_int, [_P]),
    "gd_get_option": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    "gd_commit": (C.c_int, [_P, C.POINTER(GdBatch), C.c_int32, C.c_size_t, C.c_size_t]),
    "gd_reserve": (C.c_int, [_P, C.c_int32, C.c_size_t, C.c_size_t]),
    "gd_push": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_size_t, C.c_size_t]),
    "gd_adopt_device": (C.c_int, [_P, C.c_int32, C.POINTER(GdBatch), C.c_size_t, C.c_size_t]),
    "gd_reset": (C.c_int, [_P]),
    "gd_compute": (C.c_int, [_P]),
    "gd_compute_launch": (C.c_int, [_P]),
    "gd_compute_finish": (C.c_int, [_P]),
    "gd_perbase": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P]),
    "gd_windows": (C.c_int, [_P, C.c_int32, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gd_callable": (C.c_int, [_P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gd_region_windows": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P, _P, C.c_size_t,
                                    C.POINTER(C.c_size_t)]),
    "gd_region_callable": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P, C.c_size_t,
                                     C.POINTER(C.c_size_t)]),
    "gd_regions": (C.c_int, [_P, C.c_size_t, _P, _P, _P, _P, _P, C.c_size_t, _P, _P, C.c_size_t, _P]),
    "gd_depthwed": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, _P, _P, _P, _P, C.c_size_t,
                              C.POINTER(C.c_size_t)]),
    "gd_depthwed_device": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "gd_seq_load": (C.c_int, [_P, _P, C.c_int64]),
    "gd_seq_stats": (C.c_int, [_P, C.c_size_t, _P, _P, _P, _P, _P]),
    "gd_seq_stats_ex": (C.c_int, [_P, C.c_size_t, _P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    "gd_md_flags": (C.c_int, [_P, C.c_int, _P, C.c_int32, C.c_int32, _P, _P, C.c_size_t]),
    "gd_md_begin": (C.c_int, [_P, C.c_int64]),
    "gd_md_accumulate": (C.c_int, [_P, C.c_int, _P, C.c_int32]),
    "gd_md_finish": (C.c_int, [_P, C.c_int32, _P, _P, C.c_size_t]),
    "gd_md_load_flags": (C.c_int, [_P, _P, _P, C.c_int64]),
    "gd_md_blocks": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gd_md_sums_group": (C.c_int, [_P, C.c_int, _P, C.c_size_t, _P, _P, _P]),
    "gd_md_sums": (C.c_int, [_P, C.c_size_t, _P, _P, _P]),
    "gd_inflate_bgzf": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "gd_ingest_bgzf": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_size_t, C.c_uint64, _P, C.c_size_t,
                                 C.POINTER(C.c_uint64)]),
    "gd_bgzf_members": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, _P, _P, _P, _P, C.POINTER(C.c_size_t)]),
    "gd_ingest_begin": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_size_t, _P, _P, _P, _P, _P]),
    "gd_ingest_feed": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_ingest_feed_fd": (C.c_int, [_P, C.c_int, C.c_uint64, C.c_size_t]),
    "gd_ingest_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_covstats_begin": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "gd_covstats_decode": (C.c_int, [_P, C.c_uint64, _P, C.c_size_t, C.c_int, _P]),
    "gd_covstats_histogram": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    "gd_index_begin": (C.c_int, [_P, C.c_int32, _P, C.c_uint64, C.c_uint64]),
    "gd_index_begin_csi": (C.c_int, [_P, C.c_int32, _P, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32]),
    "gd_index_decode": (C.c_int, [_P, C.c_int, _P]),
    "gd_index_result": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P, C.c_size_t, C.POINTER(C.c_size_t), _P,
                                  C.POINTER(C.c_uint64)]),
    "gd_index_windows": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_index_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_indexcov_upload": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "gd_indexcov_get_dims": (C.c_int, [_P, _P, _P, _P, _P]),
    "gd_indexcov_medians": (C.c_int, [_P, _P]),
    "gd_indexcov_depths": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_indexcov_set_depths": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_indexcov_compute": (C.c_int, [_P, C.c_int]),
    "gd_indexcov_cells": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "gd_indexcov_slots": (C.c_int, [_P, _P]),
    "gd_indexcov_counters": (C.c_int, [_P, _P]),
    "gd_indexcov_cn": (C.c_int, [_P, _P]),
    "gd_indexcov_pca8": (C.c_int, [_P, _P]),
    "gd_indexcov_gram": (C.c_int, [_P, _P]),
    "gd_indexcov_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_indexsplit_begin": (C.c_int, [_P, C.c_int32, _P]),
    "gd_indexsplit_add": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    "gd_indexsplit_sums": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_indexsplit_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_crai_sizes": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.c_size_t]),
    "gd_emdepth": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P, _P, _P]),
    "gd_emdepth_cells": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P, _P, _P, _P]),
    "gd_emdepth_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_emcnv_begin": (C.c_int, [_P, C.c_int]),
    "gd_emcnv_add": (C.c_int, [_P, _P, C.c_size_t, _P, _P, _P]),
    "gd_emcnv_add_cells": (C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, _P]),
    "gd_emcnv_finish": (C.c_int, [_P, _P, _P]),
    "gd_emcnv_read": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gd_emcnv_end": (C.c_int, [_P]),
    "gd_emcnv_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_sample_medians": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P]),
    "gd_sample_medians_cells": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P]),
    "gd_sample_medians_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_chunk_debias": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, C.c_double, _P, _P, _P, C.POINTER(C.c_size_t), _P,
                                  C.c_size_t]),
    "gd_chunk_debias_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_chunk_debias_cells": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, C.c_double, _P, _P, C.POINTER(C.c_size_t), _P,
                                        C.c_size_t]),
    "gd_moving_debias": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, C.c_int, _P, _P]),
    "gd_moving_debias_cells": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, C.c_int, _P]),
    "gd_moving_debias_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_svd_debias": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, _P, _P]),
    "gd_svd_debias_cells": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, _P, _P]),
    "gd_svd_debias_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, _P, _P]),
    "gd_svd_debias_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_svd_debias_scaled": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, _P, _P, _P]),
    "gd_svd_debias_scaled_cells": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, _P, _P, _P]),
    "gd_svd_debias_scaled_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, _P, _P, _P]),
    "gd_cnveval": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, C.c_double, _P]),
    "gd_cnveval_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_perbase_runs": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, C.c_int, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gd_perbase_runs_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_depth_hist": (C.c_int, [_P, C.c_size_t, _P, _P, _P, C.c_int32, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gd_region_bins": (C.c_int, [_P, C.c_size_t, _P, _P, _P, C.c_int, _P, _P]),
    "gd_dist_timing": (C.c_int, [_P, _P, C.c_size_t]),
    "gd_device_scale": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "gd_sample_medians_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P]),
    "gd_emdepth_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P, _P, _P]),
    "gd_emcnv_add_device": (C.c_int, [_P, _P, C.c_size_t, _P, _P, _P]),
    "gd_ingest_finish": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_uint64)]),
    "gd_ingest_decode": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_uint64)]),
    "gd_ingest_decode_part": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_size_t, C.c_uint64, C.c_uint, C.c_double,
                              C.POINTER(C.c_uint64)]),
    "gd_ingest_release": (C.c_int, [_P]),
    "gd_ingest_abort": (C.c_int, [_P]),
    "gd_host_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "gd_host_free": (C.c_int, [_P, _P]),
    "gd_device_perbase": (C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "gd_device_windows": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "gd_window_offset": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "gd_device_runs": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "gd_set_option": (C.c_int, [_P, C.c_int, C.c_int64]),
    "gd_drop_derived": (C.c_int, [_P]),
    "gd_rebuild_derived": (C.c_int, [_P]),
    "gd_set_export": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "gd_wait_event": (C.c_int, [_P, _P]),
    "gd_get_stats": (C.c_int, [_P, C.POINTER(GdStats)]),
    "gd_set_profiling": (C.c_int, [_P, C.c_int]),
    "gd_kernel_ms": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    "gd_comm_unique_id": (C.c_int, [_P, C.c_size_t]),
    "gd_comm_library": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]),
    "gd_comm_init": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t]),
    "gd_comm_destroy": (C.c_int, [_P]),
    "gd_gather_export": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int]),
    "gd_gather_wait": (C.c_int, [_P]),
    "gd_device_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "gd_device_free": (C.c_int, [_P, _P]),
    "gd_device_read": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "gd_compute_timing": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int]),
}

_LIB = None


def build(force: bool = False) -> str:
    """Compile everything in-tree for gfx950 (hipcc cross-compiles without a GPU):
    libgoleft_depth.so (HIP engine), libgoleft_host.so (C++ host), goleft-depth (CLI)."""
    src_dir = os.path.join(HERE, "csrc")
    subprocess.check_call(["make", "-s", "-C", src_dir, "all"] + (["-B"] if force else []))
    return SO_PATH


def load():
    """Load the library; raises (never falls back) when it is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.environ.get("GOLEFT_DEPTH_SO") or SO_PATH      # (measurement: a kernel variant built beside the product library)
    if not os.path.exists(so):
        raise ImportError(
            "goleft_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % so)
    lib = C.CDLL(so)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)   # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib
