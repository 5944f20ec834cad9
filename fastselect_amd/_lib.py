"""ctypes binding of ``libfastselect_amd.so`` (C ABI: ``include/fastselect_amd.h``).

The shared library holds both the hand-written HIP kernels (gfx950) and the
native CPU backend.  It is loaded eagerly when the package is imported: if it
is missing, importing ``fastselect_amd`` fails loudly -- there is no Python or
PyTorch fallback for the scoring path.

Each ``*_score`` function here replaces one reference host caller
(``_multisurf_{cpu,gpu}_host_caller`` MultiSURF.py:147-162/256-270,
``_relieff_{cpu,gpu}_host_caller`` ReliefF.py:127-134/222-236,
``_surf_{cpu,gpu}_host_caller`` SURF.py:117-128/198-218): plain numpy arrays
in, float32 scores already divided by n out.
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfastselect_amd.so")

FS_OK, FS_EINVAL, FS_ENODEV, FS_EOOM, FS_EHIP, FS_ENOTSUP = 0, -1, -2, -3, -4, -5
BACKEND_CPU, BACKEND_GPU = 0, 1

_f32p = ctypes.POINTER(ctypes.c_float)
_f64p = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_i64 = ctypes.c_int64
_int = ctypes.c_int
_vp = ctypes.c_void_p

# every symbol include/fastselect_amd.h declares (checked by tests/test_abi.py)
EXPORTED = (
    "fs_version", "fs_last_error", "fs_device_count", "fs_device_cache_release",
    "fs_stage_x", "fs_stage_x_device", "fs_stage_x_cast", "fs_unstage_x", "fs_all_finite",
    "fs_host_alloc", "fs_host_free",
    "fs_column_stats", "fs_multisurf_score", "fs_multisurf_last_guard", "fs_multisurf_score_rows",
    "fs_relieff_score", "fs_surf_score", "fs_relieff_score_rows", "fs_surf_score_rows",
    "fs_plan_create", "fs_plan_create_relieff", "fs_plan_create_surf", "fs_plan_score", "fs_plan_set_features",
    "fs_plan_pass1", "fs_plan_select", "fs_plan_pass2", "fs_plan_decision_guard", "fs_plan_set_rows",
    "fs_plan_ref_mask_words", "fs_plan_ref_masks", "fs_plan_ref_pass2", "fs_plan_ref_sums",
    "fs_plan_ref_temp",
    "fs_plan_info", "fs_plan_set_shard", "fs_multisurf_shards", "fs_plan_calibration", "fs_plan_calibration_ex", "fs_plan_weighted_pairs", "fs_plan_kernel_ms",
    "fs_plan_destroy", "fs_multisurf_score_devices", "fs_relieff_score_devices",
    "fs_surf_score_devices", "fs_set_accumulation", "fs_get_accumulation", "fs_test_hook",
    "fs_multisurf_score_ex", "fs_relieff_score_ex", "fs_surf_score_ex",
    "fs_mdr_scan", "fs_mdr_scan_labels", "fs_mdr_labels_last_timing", "fs_mdr_combinations",
    "fs_mdr_unrank", "fs_mdr_scan_top", "fs_mdr_top_last_timing",
    "fs_mi_matrices", "fs_mi_last_timing",
    "fs_cfs_create", "fs_cfs_relevance", "fs_cfs_search", "fs_cfs_row", "fs_cfs_search_matrix",
    "fs_cfs_last_timing", "fs_cfs_destroy",
    "fs_mrmr_select", "fs_mrmr_search_matrix", "fs_mrmr_last_timing",
    "fs_jmi_select", "fs_jmi_rows", "fs_jmi_search_matrix", "fs_jmi_last_timing",
    "fs_pair_screen", "fs_pair_screen_last_timing",
    "fs_pair_screen_labels", "fs_pair_labels_last_timing",
    "fs_plan_stir", "fs_stir_statistics", "fs_stir_statistics_ex", "fs_plan_stir_kernel_ms",
    "fs_plan_score_stir",
    "fs_plan_score_labels", "fs_multisurf_score_labels", "fs_plan_labels_kernel_ms",
    "fs_plan_relieff_score_labels", "fs_relieff_score_labels", "fs_plan_relieff_labels_info",
    "fs_plan_relieff_labels_kernel_ms",
    "fs_plan_surf_score_labels", "fs_surf_score_labels", "fs_plan_surf_labels_info",
    "fs_plan_surf_labels_kernel_ms",
    "fs_plan_score_targets", "fs_rrelieff_scores", "fs_rrelieff_score",
    "fs_plan_targets_kernel_ms",
    "fs_plan_star_split", "fs_plan_set_star_split", "fs_multisurf_last_star_split",
)


def _share_hip_runtime_with_torch() -> None:
    """Load PyTorch's HIP runtime before ours when PyTorch is installed.

    PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7, the
    same SONAME as /opt/rocm's).  Whichever copy is mapped first is the one
    both libraries bind to; if ours came first, torch would map a second HIP
    runtime and fail with "No HIP GPUs are available".  Importing torch first
    gives the process exactly one HIP runtime shared by torch (device memory,
    streams, RCCL via torch.distributed) and the Relief kernels.
    """
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def _load() -> ctypes.CDLL:
    _share_hip_runtime_with_torch()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"fastselect_amd native library not found at {LIB_PATH}; build it with "
            "`make -C fastselect_amd/csrc` (or __graft_entry__.build()).")
    lib = ctypes.CDLL(LIB_PATH)
    lib.fs_version.restype = ctypes.c_char_p
    lib.fs_last_error.restype = ctypes.c_char_p
    lib.fs_device_count.restype = _int
    lib.fs_device_cache_release.restype = _int
    lib.fs_multisurf_last_guard.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_int)]
    lib.fs_multisurf_last_guard.restype = _int
    lib.fs_stage_x.argtypes = [_int, _vp, _int, _i64, _i64, ctypes.POINTER(ctypes.c_uint64)]
    lib.fs_stage_x.restype = _int
    lib.fs_host_alloc.argtypes = [ctypes.c_uint64, ctypes.POINTER(_vp)]
    lib.fs_host_alloc.restype = _int
    lib.fs_host_free.argtypes = [_vp]
    lib.fs_host_free.restype = _int
    lib.fs_stage_x_device.argtypes = [_int, _vp, _vp, _int, _i64, _i64,
                                      ctypes.POINTER(ctypes.c_uint64)]
    lib.fs_stage_x_device.restype = _int
    lib.fs_stage_x_cast.argtypes = [_int, _vp, _int, _i64, _i64, _int, _vp, ctypes.POINTER(_int),
                                    ctypes.POINTER(ctypes.c_uint64)]
    lib.fs_stage_x_cast.restype = _int
    lib.fs_unstage_x.argtypes = [ctypes.c_uint64]
    lib.fs_unstage_x.restype = _int
    lib.fs_all_finite.argtypes = [_vp, _int, _i64, _i64, _int, ctypes.POINTER(_int)]
    lib.fs_all_finite.restype = _int
    lib.fs_column_stats.argtypes = [_int, _int, _vp, _int, _i64, _i64, _i64, _vp, _vp, _i64p]
    lib.fs_multisurf_score.argtypes = [_int, _int, _f32p, _i64, _i64, _f64p, _f32p, _i64p, _i64,
                                       _int, _u8p, _int, _f32p]
    lib.fs_multisurf_score_rows.argtypes = [_int, _int, _f32p, _i64, _i64, _f64p, _f32p, _i64p,
                                            _i64, _int, _u8p, _int, _i64, _i64, _f64p]
    lib.fs_plan_set_rows.argtypes = [_vp, _i64, _i64]
    lib.fs_relieff_score.argtypes = [_int, _int, _f32p, _i64, _i64, _i32p, _f32p, _u8p, _i64,
                                     _f32p, _i64, _int, _f32p]
    lib.fs_surf_score.argtypes = [_int, _int, _f64p, _i64, _i64, _i32p, _f32p, _int, _u8p, _int,
                                  _f32p]
    # the _ex calls: the same arguments plus the accumulation mode before the output
    lib.fs_multisurf_score_ex.argtypes = list(lib.fs_multisurf_score.argtypes[:-1]) + [_int, _f32p]
    lib.fs_relieff_score_ex.argtypes = list(lib.fs_relieff_score.argtypes[:-1]) + [_int, _f32p]
    lib.fs_surf_score_ex.argtypes = list(lib.fs_surf_score.argtypes[:-1]) + [_int, _f32p]
    lib.fs_relieff_score_rows.argtypes = [_int, _int, _f32p, _i64, _i64, _i32p, _f32p, _u8p,
                                          _i64, _f32p, _i64, _int, _i64, _i64, _f64p]
    lib.fs_surf_score_rows.argtypes = [_int, _int, _f64p, _i64, _i64, _i32p, _f32p, _int, _u8p,
                                       _int, _i64, _i64, _f64p]
    _ip = ctypes.POINTER(_int)
    lib.fs_multisurf_score_devices.argtypes = [_ip, _int, _f32p, _i64, _i64, _f64p, _f32p, _i64p,
                                               _i64, _int, _u8p, _int, _i64, _i64, _f64p]
    lib.fs_relieff_score_devices.argtypes = [_ip, _int, _f32p, _i64, _i64, _i32p, _f32p, _u8p,
                                             _i64, _f32p, _i64, _int, _i64, _i64, _f64p]
    lib.fs_surf_score_devices.argtypes = [_ip, _int, _f64p, _i64, _i64, _i32p, _f32p, _int, _u8p,
                                          _int, _i64, _i64, _f64p]
    lib.fs_plan_create.argtypes = [ctypes.POINTER(_vp), _int, _int, _f32p, _i64, _i64, _f64p,
                                   _f32p, _i64p, _i64, _int, _u8p, _int, _int, _int,
                                   ctypes.c_uint64]
    lib.fs_plan_create_relieff.argtypes = [ctypes.POINTER(_vp), _int, _int, _f32p, _i64, _i64,
                                           _i32p, _f32p, _u8p, _i64, _f32p, _i64, _i64, _i64,
                                           _int, ctypes.c_uint64]
    lib.fs_plan_create_surf.argtypes = [ctypes.POINTER(_vp), _int, _int, _f64p, _i64, _i64,
                                        _i32p, _f32p, _int, _u8p, _i64, _i64, _int,
                                        ctypes.c_uint64]
    lib.fs_plan_score.argtypes = [_vp, _vp]
    lib.fs_plan_score_stir.argtypes = [_vp, _vp, _vp, _vp]
    lib.fs_plan_set_features.argtypes = [_vp, _i64p, _i64]
    lib.fs_plan_pass1.argtypes = [_vp, _vp]
    lib.fs_plan_select.argtypes = [_vp, _vp, _vp]
    lib.fs_plan_pass2.argtypes = [_vp, _vp, _vp]
    lib.fs_plan_stir.argtypes = [_vp, _vp]
    lib.fs_stir_statistics.argtypes = [_f64p, _i64, ctypes.c_double, ctypes.c_double, _f64p,
                                       _f64p, _f64p, ctypes.POINTER(ctypes.c_double)]
    lib.fs_stir_statistics_ex.argtypes = list(lib.fs_stir_statistics.argtypes) + [_f64p]
    lib.fs_plan_stir_kernel_ms.argtypes = [_vp, _int]
    lib.fs_plan_stir_kernel_ms.restype = ctypes.c_double
    lib.fs_plan_score_labels.argtypes = [_vp, _i32p, _i64, _vp]
    lib.fs_plan_score_labels.restype = _int
    lib.fs_multisurf_score_labels.argtypes = [_int, _int, _f32p, _i64, _i64, _i32p, _i64, _f32p,
                                              _i64p, _i64, _u8p, _int, _f32p]
    lib.fs_multisurf_score_labels.restype = _int
    lib.fs_plan_labels_kernel_ms.argtypes = [_vp, _int]
    lib.fs_plan_labels_kernel_ms.restype = ctypes.c_double
    lib.fs_plan_relieff_score_labels.argtypes = [_vp, _i32p, _i64, _vp]
    lib.fs_plan_relieff_score_labels.restype = _int
    lib.fs_relieff_score_labels.argtypes = [_int, _int, _f32p, _i64, _i64, _i32p, _i64, _f32p,
                                            _u8p, _i64, _int, _f32p]
    lib.fs_relieff_score_labels.restype = _int
    lib.fs_plan_relieff_labels_info.argtypes = [_vp, _i64p]
    lib.fs_plan_relieff_labels_info.restype = _int
    lib.fs_plan_relieff_labels_kernel_ms.argtypes = [_vp, _int]
    lib.fs_plan_relieff_labels_kernel_ms.restype = ctypes.c_double
    lib.fs_plan_surf_score_labels.argtypes = [_vp, _i32p, _i64, _vp]
    lib.fs_plan_surf_score_labels.restype = _int
    lib.fs_surf_score_labels.argtypes = [_int, _int, _f64p, _i64, _i64, _i32p, _i64, _f32p,
                                         _u8p, _int, _int, _f32p]
    lib.fs_surf_score_labels.restype = _int
    lib.fs_plan_surf_labels_info.argtypes = [_vp, _i64p]
    lib.fs_plan_surf_labels_info.restype = _int
    lib.fs_plan_surf_labels_kernel_ms.argtypes = [_vp, _int]
    lib.fs_plan_surf_labels_kernel_ms.restype = ctypes.c_double
    lib.fs_plan_score_targets.argtypes = [_vp, _f64p, _i64, _vp, _vp, _vp]
    lib.fs_plan_score_targets.restype = _int
    lib.fs_rrelieff_scores.argtypes = [_f64p, _f64p, ctypes.c_double, ctypes.c_double, _i64, _f32p]
    lib.fs_rrelieff_scores.restype = _int
    lib.fs_rrelieff_score.argtypes = [_int, _int, _f32p, _i64, _i64, _f64p, _i64, _f32p, _u8p,
                                      _i64, _int, _f32p]
    lib.fs_rrelieff_score.restype = _int
    lib.fs_plan_targets_kernel_ms.argtypes = [_vp, _int]
    lib.fs_plan_targets_kernel_ms.restype = ctypes.c_double
    lib.fs_plan_decision_guard.argtypes = [_vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(_int)]
    lib.fs_plan_ref_mask_words.argtypes = [_vp, _i64p]
    lib.fs_plan_ref_masks.argtypes = [_vp, _vp, _i64]
    lib.fs_plan_ref_pass2.argtypes = [_vp, _vp, _vp, _i64, _i64]
    lib.fs_plan_ref_sums.argtypes = [_vp, _vp, _vp]
    lib.fs_plan_ref_temp.argtypes = [_vp]
    lib.fs_plan_info.argtypes = [_vp, _i64p, _f64p, _i64p]
    lib.fs_plan_calibration.argtypes = [_vp, _f64p]
    lib.fs_plan_calibration_ex.argtypes = [_vp, _f64p, _int]
    lib.fs_plan_calibration_ex.restype = _int
    lib.fs_plan_set_shard.argtypes = [_vp, _int, _int]
    lib.fs_multisurf_shards.argtypes = [_int, _i64, _i64, _int, ctypes.POINTER(_int)]
    lib.fs_plan_weighted_pairs.argtypes = [_vp, _i64p]
    lib.fs_plan_star_split.argtypes = [_vp, ctypes.POINTER(_int)]
    lib.fs_plan_star_split.restype = _int
    lib.fs_plan_set_star_split.argtypes = [_vp, _int]
    lib.fs_plan_set_star_split.restype = _int
    lib.fs_multisurf_last_star_split.argtypes = [ctypes.POINTER(_int)]
    lib.fs_multisurf_last_star_split.restype = _int
    lib.fs_plan_kernel_ms.argtypes = [_vp, _int]
    lib.fs_plan_kernel_ms.restype = ctypes.c_double
    lib.fs_plan_destroy.argtypes = [_vp]
    lib.fs_set_accumulation.argtypes = [_int, ctypes.POINTER(_int)]
    lib.fs_set_accumulation.restype = _int
    lib.fs_get_accumulation.argtypes = []
    lib.fs_get_accumulation.restype = _int
    lib.fs_test_hook.argtypes = [ctypes.c_char_p, _i64]
    lib.fs_test_hook.restype = _int
    lib.fs_mdr_scan.argtypes = [_int, _int, _u8p, _i64, _i64, _u8p, _int, _i32p, _int, _int, _f32p,
                                _i64p, _f32p]
    lib.fs_mdr_scan.restype = _int
    lib.fs_mdr_scan_labels.argtypes = [_int, _int, _u8p, _i64, _i64, _u8p, _int, _int, _i32p, _int,
                                       _int, _f32p, _i64p, _f32p]
    lib.fs_mdr_scan_labels.restype = _int
    lib.fs_mdr_labels_last_timing.argtypes = [_f64p]
    lib.fs_mdr_labels_last_timing.restype = _int
    lib.fs_mdr_scan_top.argtypes = [_int, _int, _u8p, _i64, _i64, _u8p, _int, _i32p, _int, _int,
                                    _int, _f32p, _i64p]
    lib.fs_mdr_scan_top.restype = _int
    lib.fs_mdr_top_last_timing.argtypes = [_f64p]
    lib.fs_mdr_top_last_timing.restype = _int
    lib.fs_mdr_combinations.argtypes = [_i64, _int, _i64p]
    lib.fs_mdr_combinations.restype = _int
    lib.fs_mdr_unrank.argtypes = [_i64, _int, _i64, _i32p]
    lib.fs_mdr_unrank.restype = _int
    lib.fs_mi_matrices.argtypes = [_int, _int, _u8p, _u8p, _i64, _i64, _int, _int, _int, _f64p,
                                   _f64p, _i32p]
    lib.fs_mi_matrices.restype = _int
    lib.fs_mi_last_timing.argtypes = [_f64p]
    lib.fs_mi_last_timing.restype = _int
    lib.fs_cfs_create.argtypes = [ctypes.POINTER(_vp), _int, _int, _u8p, _u8p, _i64, _i64, _int,
                                  _int]
    lib.fs_cfs_relevance.argtypes = [_vp, _f32p]
    lib.fs_cfs_search.argtypes = [_vp, ctypes.c_double, _i64p, _i64p, _f64p]
    lib.fs_cfs_row.argtypes = [_vp, _i64, _f32p]
    lib.fs_cfs_search_matrix.argtypes = [_int, _int, _f32p, _f32p, _i64, ctypes.c_double, _i64p,
                                         _i64p, _f64p]
    lib.fs_cfs_last_timing.argtypes = [_f64p]
    lib.fs_cfs_destroy.argtypes = [_vp]
    for name in ("fs_cfs_create", "fs_cfs_relevance", "fs_cfs_search", "fs_cfs_row",
                 "fs_cfs_search_matrix", "fs_cfs_last_timing", "fs_cfs_destroy"):
        getattr(lib, name).restype = _int
    lib.fs_mrmr_select.argtypes = [_int, _int, _u8p, _u8p, _i64, _i64, _int, _int, _int, _i64, _int,
                                   _f64p, _i64p, _f64p]
    lib.fs_mrmr_search_matrix.argtypes = [_int, _int, _f64p, _f64p, _i64, _int, _i64, _i64p]
    lib.fs_mrmr_last_timing.argtypes = [_f64p]
    for name in ("fs_mrmr_select", "fs_mrmr_search_matrix", "fs_mrmr_last_timing"):
        getattr(lib, name).restype = _int
    lib.fs_jmi_select.argtypes = list(lib.fs_mrmr_select.argtypes)
    lib.fs_jmi_rows.argtypes = [_int, _int, _u8p, _u8p, _i64, _i64, _int, _int, _i64p, _i64, _int,
                                _f64p]
    lib.fs_jmi_search_matrix.argtypes = list(lib.fs_mrmr_search_matrix.argtypes)
    lib.fs_jmi_last_timing.argtypes = [_f64p]
    for name in ("fs_jmi_select", "fs_jmi_rows", "fs_jmi_search_matrix", "fs_jmi_last_timing"):
        getattr(lib, name).restype = _int
    lib.fs_pair_screen.argtypes = [_int, _int, _u8p, _u8p, _i64, _i64, _int, _int, _int, _i64, _int,
                                   _f64p, _f64p, _i64p, _i64p, _f64p]
    lib.fs_pair_screen.restype = _int
    lib.fs_pair_screen_last_timing.argtypes = [_f64p]
    lib.fs_pair_screen_last_timing.restype = _int
    lib.fs_pair_screen_labels.argtypes = [_int, _int, _u8p, _u8p, _int, _i64, _i64, _int, _int,
                                          _int, _int, _f64p, _i64p, _i64p, _f64p]
    lib.fs_pair_screen_labels.restype = _int
    lib.fs_pair_labels_last_timing.argtypes = [_f64p]
    lib.fs_pair_labels_last_timing.restype = _int
    for name in ("fs_column_stats", "fs_multisurf_score", "fs_multisurf_score_rows",
                 "fs_plan_set_rows", "fs_relieff_score", "fs_surf_score",
                 "fs_relieff_score_rows", "fs_surf_score_rows", "fs_plan_create",
                 "fs_plan_create_relieff", "fs_plan_create_surf", "fs_plan_score", "fs_plan_set_features", "fs_plan_pass1", "fs_plan_select",
                 "fs_plan_pass2", "fs_plan_decision_guard", "fs_plan_ref_mask_words", "fs_plan_ref_masks",
                 "fs_plan_ref_pass2", "fs_plan_ref_sums", "fs_plan_ref_temp", "fs_plan_info", "fs_plan_set_shard", "fs_multisurf_shards", "fs_plan_calibration", "fs_plan_weighted_pairs",
                 "fs_plan_destroy", "fs_multisurf_score_devices", "fs_relieff_score_devices",
                 "fs_surf_score_devices", "fs_multisurf_score_ex", "fs_relieff_score_ex",
                 "fs_surf_score_ex", "fs_plan_stir", "fs_stir_statistics", "fs_stir_statistics_ex",
                 "fs_plan_score_stir"):
        getattr(lib, name).restype = _int
    return lib


_lib = _load()


def lib() -> ctypes.CDLL:
    return _lib


def version() -> str:
    return _lib.fs_version().decode()


@contextlib.contextmanager
def staged_x(backend, x, device=0):
    """One upload of X for a whole fit on the GPU backend (fs_stage_x): the
    column statistics and the scoring call that receive this same array read
    the device copy.  ``x`` must be C-contiguous float32 / float64 and stay
    unchanged inside the block; other backends pass through."""
    if backend != "gpu" or x.dtype not in (np.float32, np.float64) or \
            not x.flags.c_contiguous or x.ndim != 2 or x.size == 0:
        yield
        return
    h = ctypes.c_uint64(0)
    if _lib.fs_stage_x(int(device), x.ctypes.data, int(x.dtype == np.float64), x.shape[0],
                       x.shape[1], ctypes.byref(h)) != 0:
        # staging is only an optimisation: without device room for the extra
        # copy the calls upload X themselves (and report their own errors)
        yield
        return
    try:
        yield
    finally:
        _lib.fs_unstage_x(h)


def stage_x_cast(x, n_jobs=-1, device=0):
    """``x`` (C-contiguous float64 or float32 matrix) cast / copied to
    float32 by fs_stage_x_cast: returns (x32, finite, handle) -- the cast
    array (pinned host memory when possible), whether every value of it is finite, and the handle of its
    device copy on ``device`` (0: not staged; release with ``unstaged``)."""
    out = pinned_empty(x.shape, np.float32)
    if out is None:
        out = np.empty(x.shape, dtype=np.float32)
    fin = _int(0)
    h = ctypes.c_uint64(0)
    check(_lib.fs_stage_x_cast(int(device), x.ctypes.data, int(x.dtype == np.float64),
                               x.shape[0], x.shape[1], int(n_jobs), out.ctypes.data,
                               ctypes.byref(fin), ctypes.byref(h)))
    return out, bool(fin.value), int(h.value)


@contextlib.contextmanager
def unstaged(handle):
    """Release a device copy staged by stage_x_cast (handle 0: nothing) when
    the block ends."""
    try:
        yield
    finally:
        if handle:
            _lib.fs_unstage_x(ctypes.c_uint64(handle))


def pinned_empty(shape, dtype):
    """An uninitialised C-contiguous array in pinned host memory from the
    library's block cache (fs_host_alloc), returned to the cache when the
    array is collected; None when no GPU is visible or pinning fails."""
    import weakref
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dtype.itemsize
    if nbytes == 0 or not gpu_available():
        return None
    p = _vp()
    if _lib.fs_host_alloc(ctypes.c_uint64(nbytes), ctypes.byref(p)) != 0 or not p.value:
        return None
    buf = (ctypes.c_char * nbytes).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
    fin = weakref.finalize(buf, _lib.fs_host_free, _vp(p.value))
    fin.atexit = False  # at exit the block goes with the process (no HIP call then)
    return arr


def multisurf_shards(n: int, p: int, world: int = 1, device: int = 0) -> int:
    """Tile shards per device that fit a MultiSURF job (fs_multisurf_shards)."""
    v = _int(1)
    check(_lib.fs_multisurf_shards(int(device), int(n), int(p), int(world), ctypes.byref(v)))
    return int(v.value)


@contextlib.contextmanager
def staged_device_x(x, x_device_ptr, device=0):
    """Register a device copy of the host array ``x`` that the caller holds
    (``x_device_ptr``: n x p, same dtype, row-major) for the calls inside the
    block (fs_stage_x_device): the column statistics and the plans given
    ``x`` read it instead of uploading X."""
    h = ctypes.c_uint64(0)
    check(_lib.fs_stage_x_device(int(device), x.ctypes.data, _vp(int(x_device_ptr)),
                                 int(x.dtype == np.float64), x.shape[0], x.shape[1],
                                 ctypes.byref(h)))
    try:
        yield
    finally:
        _lib.fs_unstage_x(h)


def all_finite(x, n_jobs=-1) -> bool:
    """No NaN and no infinity in a C-contiguous float32 / float64 matrix
    (fs_all_finite, host threads)."""
    f = _int(0)
    check(_lib.fs_all_finite(x.ctypes.data, int(x.dtype == np.float64), x.shape[0],
                             int(np.prod(x.shape[1:])), int(n_jobs), ctypes.byref(f)))
    return bool(f.value)


def host_threads(n_jobs=-1) -> int:
    """The native library's thread count for ``n_jobs`` (fs_prep.cpp
    hardware_threads): n_jobs > 0 as given, else the CPUs of this process's
    affinity mask, capped by OMP_NUM_THREADS when set."""
    if n_jobs is not None and n_jobs > 0:
        return int(n_jobs)
    try:
        hw = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        hw = os.cpu_count() or 1
    cap = os.environ.get("OMP_NUM_THREADS", "")
    if cap.isdigit() and 0 < int(cap) < hw:
        hw = int(cap)
    return max(1, hw)


def release_device_cache() -> None:
    """Free the device blocks kept between fits (fs_device_cache_release)."""
    _lib.fs_device_cache_release()


def multisurf_last_guard():
    """(risk, rerun) of this thread's last GPU MultiSURF one-shot call
    (fs_multisurf_last_guard): the 16-bit decision risk (-1 when not
    evaluated) and whether the call scored again on 32-bit operands."""
    risk = ctypes.c_double(-1.0)
    rerun = _int(0)
    _lib.fs_multisurf_last_guard(ctypes.byref(risk), ctypes.byref(rerun))
    return float(risk.value), bool(rerun.value)


def multisurf_last_star_split() -> int:
    """The star form this thread's last GPU MultiSURF one-shot call ran in
    (fs_multisurf_last_star_split): 1 = the star split, 0 = dense star
    weights or no star, -1 = no such call yet.  A ``devices=`` call decides
    it once for all its devices."""
    v = _int(-1)
    check(_lib.fs_multisurf_last_star_split(ctypes.byref(v)))
    return int(v.value)


def device_count() -> int:
    """Number of visible HIP devices (0 when none)."""
    return int(_lib.fs_device_count())


def gpu_available() -> bool:
    return device_count() > 0


def check(rc: int) -> None:
    """Map a C return code to the Python exception the estimators raise."""
    if rc == FS_OK:
        return
    msg = _lib.fs_last_error().decode(errors="replace")
    if rc == FS_EINVAL:
        raise ValueError(msg)
    if rc == FS_EOOM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


ACCUM_MODES = {"fast": 0, "reference": 1}


def accumulation_code(mode: str) -> int:
    """FS_ACCUM_FAST / FS_ACCUM_REFERENCE for the estimators' ``accumulation``
    parameter ('fast' or 'reference'); ValueError for anything else."""
    if not isinstance(mode, str) or mode not in ACCUM_MODES:
        raise ValueError(f"accumulation must be 'fast' or 'reference'; got {mode!r}")
    return ACCUM_MODES[mode]


@contextlib.contextmanager
def accumulation(mode: str = "fast"):
    """The calling thread's accumulation mode for the native calls (and plan
    creations) inside the block (fs_set_accumulation), restored afterwards.
    'reference' replays the reference's float32 per-sample sums and column
    sums (MultiSURF.py:198-253, ReliefF.py:181-220) bit for bit."""
    code = accumulation_code(mode)
    prev = _int(0)
    check(_lib.fs_set_accumulation(code, ctypes.byref(prev)))
    try:
        yield
    finally:
        _lib.fs_set_accumulation(prev.value, None)


def set_test_hook(name: str, value: int = 1) -> None:
    """TEST-ONLY (fs_test_hook): override one internal choice of the library
    process-wide; ``set_test_hook("reset")`` restores every default."""
    check(_lib.fs_test_hook(name.encode(), int(value)))


@contextlib.contextmanager
def test_hooks(**hooks):
    """TEST-ONLY: the given fs_test_hook overrides inside the block, every
    default restored afterwards."""
    try:
        for k, v in hooks.items():
            set_test_hook(k, int(v))
        yield
    finally:
        set_test_hook("reset")


def _p(a: np.ndarray, t):
    return a.ctypes.data_as(t)


def _backend_code(backend: str) -> int:
    if backend == "gpu":
        return BACKEND_GPU
    if backend == "cpu":
        return BACKEND_CPU
    raise ValueError("backend must be 'cpu' or 'gpu' at the native boundary")


GPU_STATS_MAX_CAP = 8191


def column_stats(backend, x, count_cap, device=0):
    """Column minima, maxima and distinct-value counts (capped at
    ``count_cap + 1``) of a float32 / float64 matrix (``fs_column_stats``):
    the ``x.min(0)``, ``x.max(0)`` and ``np.unique(x[:, f]).size`` of the
    reference's fit() (MultiSURF.py:141-144, 409-420)."""
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    n, p = x.shape
    mn = np.empty(p, dtype=x.dtype)
    mx = np.empty(p, dtype=x.dtype)
    nd = np.empty(p, dtype=np.int64)
    check(_lib.fs_column_stats(_backend_code(backend), int(device), x.ctypes.data,
                               int(x.dtype == np.float64), n, p, int(count_cap), mn.ctypes.data,
                               mx.ctypes.data, _p(nd, _i64p)))
    return mn, mx, nd


def _devices_arg(devices):
    d = np.ascontiguousarray(devices, dtype=np.int32)
    return d, _p(d, ctypes.POINTER(_int)), int(d.size)


def _multi(backend, devices):
    """The *_devices entry point applies: GPU backend and more than one
    device ordinal (one ordinal is the plain call on that device)."""
    return backend == "gpu" and devices is not None and len(devices) > 1


def multisurf_score(backend, x, y, recip, feat_idx, use_star, is_discrete, n_jobs=-1, device=0,
                    rows=None, devices=None):
    """Drop-in for ``_multisurf_{cpu,gpu}_host_caller`` (MultiSURF.py:147-162, 256-270).

    rows=(begin, end): float64 score sums of those focal samples only
    (``fs_multisurf_score_rows``) instead of float32 scores / n.
    devices=[d0, d1, ...] (GPU backend): one host thread per entry
    (``fs_multisurf_score_devices``); one entry = ``device``.
    """
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, p = x.shape
    yv = np.ascontiguousarray(y, dtype=np.float64)
    rc_ = np.ascontiguousarray(recip, dtype=np.float32)
    isd = np.ascontiguousarray(is_discrete, dtype=np.uint8)
    fidx = None if feat_idx is None else np.ascontiguousarray(feat_idx, dtype=np.int64)
    n_kept = p if fidx is None else fidx.size
    if devices is not None and not _multi(backend, devices):
        device = int(devices[0])
    if _multi(backend, devices):
        _keep, dp, nd = _devices_arg(devices)
        lo, hi = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
        sums = np.zeros(n_kept, dtype=np.float64)
        check(_lib.fs_multisurf_score_devices(dp, nd, _p(x, _f32p), n, p, _p(yv, _f64p),
                                              _p(rc_, _f32p),
                                              None if fidx is None else _p(fidx, _i64p), n_kept,
                                              int(bool(use_star)), _p(isd, _u8p), int(n_jobs),
                                              lo, hi, _p(sums, _f64p)))
        return sums if rows is not None else (sums / n).astype(np.float32)
    if rows is not None:
        sums = np.zeros(n_kept, dtype=np.float64)
        check(_lib.fs_multisurf_score_rows(_backend_code(backend), int(device), _p(x, _f32p), n, p,
                                           _p(yv, _f64p), _p(rc_, _f32p),
                                           None if fidx is None else _p(fidx, _i64p), n_kept,
                                           int(bool(use_star)), _p(isd, _u8p), int(n_jobs),
                                           int(rows[0]), int(rows[1]), _p(sums, _f64p)))
        return sums
    out = np.zeros(n_kept, dtype=np.float32)
    check(_lib.fs_multisurf_score(_backend_code(backend), int(device), _p(x, _f32p), n, p,
                                  _p(yv, _f64p), _p(rc_, _f32p),
                                  None if fidx is None else _p(fidx, _i64p), n_kept,
                                  int(bool(use_star)), _p(isd, _u8p), int(n_jobs),
                                  _p(out, _f32p)))
    return out


def _labels_arg(labels, n):
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim == 1:
        lab = lab.reshape(1, -1)
    if lab.ndim != 2 or lab.shape[1] != n:
        raise ValueError(f"labels must have shape (B, {n}); got {lab.shape}")
    return lab


def multisurf_score_labels(backend, x, labels, recip, is_discrete, feat_idx=None, n_jobs=-1,
                           device=0):
    """MultiSURF scores of B labellings of the same samples in one call
    (``fs_multisurf_score_labels``): distances, thresholds and near sets do
    not depend on the labels, so they are computed once and every labelling
    only re-weighs the near pairs.  ``labels``: (B, n) integers, compared by
    equality only.  Returns (B, n_kept) float32; row b is the score vector of
    ``multisurf_score`` with labelling b as y (CPU backend: bit for bit)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, p = x.shape
    lab = _labels_arg(labels, n)
    rc_ = np.ascontiguousarray(recip, dtype=np.float32)
    isd = np.ascontiguousarray(is_discrete, dtype=np.uint8)
    fidx = None if feat_idx is None else np.ascontiguousarray(feat_idx, dtype=np.int64)
    n_kept = p if fidx is None else fidx.size
    out = np.zeros((lab.shape[0], n_kept), dtype=np.float32)
    check(_lib.fs_multisurf_score_labels(_backend_code(backend), int(device), _p(x, _f32p), n, p,
                                         _p(lab, _i32p), lab.shape[0], _p(rc_, _f32p),
                                         None if fidx is None else _p(fidx, _i64p), n_kept,
                                         _p(isd, _u8p), int(n_jobs), _p(out, _f32p)))
    return out


def relieff_score_labels(backend, x, labels, recip, is_discrete, k, n_jobs=-1, device=0):
    """ReliefF scores of B labellings of the same samples in one call
    (``fs_relieff_score_labels``): the distance pass does not read the labels,
    so it runs once, and every labelling only selects its neighbours and
    updates.  ``labels``: (B, n) integer class codes in [0, 64); the priors of a
    labelling are its class shares.  Returns (B, p) float32; row b is the score
    vector of ``relieff_score`` with labelling b as y (CPU backend: bit for
    bit)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, p = x.shape
    lab = _labels_arg(labels, n)
    rc_ = np.ascontiguousarray(recip, dtype=np.float32)
    isd = np.ascontiguousarray(is_discrete, dtype=np.uint8)
    out = np.zeros((lab.shape[0], p), dtype=np.float32)
    check(_lib.fs_relieff_score_labels(_backend_code(backend), int(device), _p(x, _f32p), n, p,
                                       _p(lab, _i32p), lab.shape[0], _p(rc_, _f32p),
                                       _p(isd, _u8p), int(k), int(n_jobs), _p(out, _f32p)))
    return out


def surf_score_labels(backend, x, labels, recip, is_discrete, use_star=False, n_jobs=-1, device=0):
    """SURF / SURF* scores of B labellings of the same samples in one call
    (``fs_surf_score_labels``): the near sets do not read the labels, so
    distances and means run once and every labelling only re-weighs the near
    pairs (SURF*: and walks each sorted column).  ``labels``: (B, n) integers,
    compared by equality only (GPU, SURF*: codes in [0, 8)).  Returns (B, p)
    float32; row b is the score vector of ``surf_score`` with labelling b as y
    (CPU backend: bit for bit)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, p = x.shape
    lab = _labels_arg(labels, n)
    rc_ = np.ascontiguousarray(recip, dtype=np.float32)
    isd = np.ascontiguousarray(is_discrete, dtype=np.uint8)
    out = np.zeros((lab.shape[0], p), dtype=np.float32)
    check(_lib.fs_surf_score_labels(_backend_code(backend), int(device), _p(x, _f64p), n, p,
                                    _p(lab, _i32p), lab.shape[0], _p(rc_, _f32p), _p(isd, _u8p),
                                    int(bool(use_star)), int(n_jobs), _p(out, _f32p)))
    return out


def _targets_arg(targets, n):
    t = np.ascontiguousarray(targets, dtype=np.float64)
    if t.ndim == 1:
        t = t.reshape(1, -1)
    if t.ndim != 2 or t.shape[1] != n:
        raise ValueError(f"targets must have shape (B, {n}); got {t.shape}")
    return t


def rrelieff_scores(s_a, s_ca, s_c, n_pairs):
    """The RReliefF epilogue (``fs_rrelieff_scores``) per target: float32
    scores (B, n_kept) from S_A (n_kept), S_CA (B, n_kept), S_C (B) and the
    number of pairs M = rows * k."""
    s_a = np.ascontiguousarray(s_a, dtype=np.float64)
    s_ca = np.ascontiguousarray(s_ca, dtype=np.float64).reshape(-1, s_a.size)
    s_c = np.ascontiguousarray(s_c, dtype=np.float64).reshape(-1)
    out = np.zeros(s_ca.shape, dtype=np.float32)
    for b in range(s_ca.shape[0]):
        check(_lib.fs_rrelieff_scores(_p(s_a, _f64p), _p(s_ca[b], _f64p), float(s_c[b]),
                                      float(n_pairs), s_a.size, _p(out[b], _f32p)))
    return out


def rrelieff_score(backend, x, targets, recip, is_discrete, k, n_jobs=-1, device=0):
    """RReliefF scores of B continuous targets of the same samples in one call
    (``fs_rrelieff_score``): the neighbours (the k nearest of all) do not read
    the target, so distances and selection run once and a target only adds a
    weight per (sample, neighbour) pair.  ``targets``: (B, n) or (n,) float64,
    finite.  Returns (B, p) float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, p = x.shape
    t = _targets_arg(targets, n)
    rc_ = np.ascontiguousarray(recip, dtype=np.float32)
    isd = np.ascontiguousarray(is_discrete, dtype=np.uint8)
    out = np.zeros((t.shape[0], p), dtype=np.float32)
    check(_lib.fs_rrelieff_score(_backend_code(backend), int(device), _p(x, _f32p), n, p,
                                 _p(t, _f64p), t.shape[0], _p(rc_, _f32p), _p(isd, _u8p), int(k),
                                 int(n_jobs), _p(out, _f32p)))
    return out


def relieff_score(backend, x, y_enc, recip, is_discrete, k, class_probs, n_jobs=-1, device=0,
                  rows=None, devices=None):
    """Drop-in for ``_relieff_{cpu,gpu}_host_caller`` (ReliefF.py:127-134, 222-236).

    rows=(begin, end): float64 score sums of those focal samples only
    (``fs_relieff_score_rows``, row sharding) instead of float32 scores / n.
    devices: as ``multisurf_score`` (``fs_relieff_score_devices``).
    """
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, p = x.shape
    ye = np.ascontiguousarray(y_enc, dtype=np.int32)
    rc_ = np.ascontiguousarray(recip, dtype=np.float32)
    isd = np.ascontiguousarray(is_discrete, dtype=np.uint8)
    cp = np.ascontiguousarray(class_probs, dtype=np.float32)
    if devices is not None and not _multi(backend, devices):
        device = int(devices[0])
    if _multi(backend, devices):
        _keep, dp, nd = _devices_arg(devices)
        lo, hi = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
        sums = np.zeros(p, dtype=np.float64)
        check(_lib.fs_relieff_score_devices(dp, nd, _p(x, _f32p), n, p, _p(ye, _i32p),
                                            _p(rc_, _f32p), _p(isd, _u8p), int(k), _p(cp, _f32p),
                                            cp.size, int(n_jobs), lo, hi, _p(sums, _f64p)))
        return sums if rows is not None else (sums / n).astype(np.float32)
    args = (_backend_code(backend), int(device), _p(x, _f32p), n, p, _p(ye, _i32p),
            _p(rc_, _f32p), _p(isd, _u8p), int(k), _p(cp, _f32p), cp.size, int(n_jobs))
    if rows is not None:
        out = np.zeros(p, dtype=np.float64)
        check(_lib.fs_relieff_score_rows(*args, int(rows[0]), int(rows[1]), _p(out, _f64p)))
        return out
    out = np.zeros(p, dtype=np.float32)
    check(_lib.fs_relieff_score(*args, _p(out, _f32p)))
    return out


def surf_score(backend, x, y, recip, use_star, is_discrete, n_jobs=-1, device=0, rows=None,
               devices=None):
    """Drop-in for ``_surf_{cpu,gpu}_host_caller`` (SURF.py:117-128, 198-218).

    rows=(begin, end): float64 score sums of those focal samples only
    (``fs_surf_score_rows``, row sharding) instead of float32 scores / n.
    devices: as ``multisurf_score`` (``fs_surf_score_devices``).
    """
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, p = x.shape
    yi = np.ascontiguousarray(y, dtype=np.int32)
    rc_ = np.ascontiguousarray(recip, dtype=np.float32)
    isd = np.ascontiguousarray(is_discrete, dtype=np.uint8)
    if devices is not None and not _multi(backend, devices):
        device = int(devices[0])
    if _multi(backend, devices):
        _keep, dp, nd = _devices_arg(devices)
        lo, hi = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
        sums = np.zeros(p, dtype=np.float64)
        check(_lib.fs_surf_score_devices(dp, nd, _p(x, _f64p), n, p, _p(yi, _i32p),
                                         _p(rc_, _f32p), int(bool(use_star)), _p(isd, _u8p),
                                         int(n_jobs), lo, hi, _p(sums, _f64p)))
        return sums if rows is not None else (sums / n).astype(np.float32)
    args = (_backend_code(backend), int(device), _p(x, _f64p), n, p, _p(yi, _i32p),
            _p(rc_, _f32p), int(bool(use_star)), _p(isd, _u8p), int(n_jobs))
    if rows is not None:
        out = np.zeros(p, dtype=np.float64)
        check(_lib.fs_surf_score_rows(*args, int(rows[0]), int(rows[1]), _p(out, _f64p)))
        return out
    out = np.zeros(p, dtype=np.float32)
    check(_lib.fs_surf_score(*args, _p(out, _f32p)))
    return out


class Plan:
    """A sharded MultiSURF plan (``fs_plan_*``) for one rank.

    Exchange buffers (rowstats[3n], counts[2n], scores[n_kept], float64) are
    passed by address: device pointers for the GPU backend, host pointers for
    the CPU backend (see ``fastselect_amd.parallel``).
    """

    def __init__(self, backend, x, y, recip, is_discrete, use_star=False, feat_idx=None,
                 rank=0, world=1, n_jobs=-1, device=0, stream=0, _handle=None):
        if _handle is not None:  # built by RowsPlan
            return
        x = np.ascontiguousarray(x, dtype=np.float32)
        self.n, self.p = x.shape
        yv = np.ascontiguousarray(y, dtype=np.float64)
        rc_ = np.ascontiguousarray(recip, dtype=np.float32)
        isd = np.ascontiguousarray(is_discrete, dtype=np.uint8)
        fidx = None if feat_idx is None else np.ascontiguousarray(feat_idx, dtype=np.int64)
        self.n_kept = self.p if fidx is None else fidx.size
        self.backend = backend
        self._h = _vp()
        check(_lib.fs_plan_create(ctypes.byref(self._h), _backend_code(backend), int(device),
                                  _p(x, _f32p), self.n, self.p, _p(yv, _f64p), _p(rc_, _f32p),
                                  None if fidx is None else _p(fidx, _i64p), self.n_kept,
                                  int(bool(use_star)), _p(isd, _u8p), int(rank), int(world),
                                  int(n_jobs), ctypes.c_uint64(int(stream))))

    def set_features(self, feat_idx) -> None:
        """Score another feature subset of the resident samples next
        (``fs_plan_set_features``); pass2 then returns len(feat_idx) sums."""
        fidx = None if feat_idx is None else np.ascontiguousarray(feat_idx, dtype=np.int64)
        self.n_kept = self.p if fidx is None else fidx.size
        check(_lib.fs_plan_set_features(self._h, None if fidx is None else _p(fidx, _i64p),
                                        self.n_kept))

    def pass1(self, rowstats_ptr: int) -> None:
        check(_lib.fs_plan_pass1(self._h, _vp(rowstats_ptr)))

    def select(self, rowstats_ptr: int, counts_ptr: int) -> None:
        check(_lib.fs_plan_select(self._h, _vp(rowstats_ptr), _vp(counts_ptr)))

    def pass2(self, counts_ptr: int, scores_ptr: int) -> None:
        check(_lib.fs_plan_pass2(self._h, _vp(counts_ptr), _vp(scores_ptr)))

    def stir(self, sums_ptr: int) -> None:
        """This plan's STIR partial sums into sums[4 * n_kept] (``fs_plan_stir``:
        S1H, S2H, S1M, S2M per kept feature), after ``select``."""
        check(_lib.fs_plan_stir(self._h, _vp(sums_ptr)))

    def stir_kernel_ms(self, which: int) -> float:
        """HIP-event time of the last ``stir``'s multiplicity (0) / score (1)
        kernels over its chunks, or (2) of the last ``RowsPlan.score_stir``'s
        k_rf_stir (``fs_plan_stir_kernel_ms``; -1: unavailable)."""
        return float(_lib.fs_plan_stir_kernel_ms(self._h, int(which)))

    def score_labels(self, labels, scores_ptr: int) -> None:
        """The score sums of the (B, n) int32 host labellings on this plan's
        decisions into scores[B * n_kept] (``fs_plan_score_labels``), after
        ``select``; scores in the memory space ``pass2`` writes to."""
        lab = _labels_arg(labels, self.n)
        check(_lib.fs_plan_score_labels(self._h, _p(lab, _i32p), lab.shape[0], _vp(scores_ptr)))

    def labels_kernel_ms(self, which: int) -> float:
        """HIP-event time of the last ``score_labels``' record (0), counts and
        weights (1) or score (2) kernels (``fs_plan_labels_kernel_ms``; -1: unavailable)."""
        return float(_lib.fs_plan_labels_kernel_ms(self._h, int(which)))

    def ref_mask_words(self) -> int:
        """int64 words of the reference-order decision masks (``fs_plan_ref_mask_words``)."""
        w = _i64(0)
        check(_lib.fs_plan_ref_mask_words(self._h, ctypes.byref(w)))
        return int(w.value)

    def ref_masks(self, masks_ptr: int, words: int) -> None:
        """This rank's tile decisions into the zeroed masks (``fs_plan_ref_masks``)."""
        check(_lib.fs_plan_ref_masks(self._h, _vp(masks_ptr), _i64(words)))

    def ref_pass2(self, masks_ptr: int, counts_ptr: int, row_begin: int, row_end: int) -> None:
        """Reference-order chains of the focal rows [row_begin, row_end) into
        the plan's temp rows (``fs_plan_ref_pass2``)."""
        check(_lib.fs_plan_ref_pass2(self._h, _vp(masks_ptr), _vp(counts_ptr), _i64(row_begin),
                                     _i64(row_end)))

    def ref_sums(self, init_ptr: int, sums_ptr: int) -> None:
        """float32 column sums of the temp rows continuing init (0 = none)
        into sums (``fs_plan_ref_sums``)."""
        check(_lib.fs_plan_ref_sums(self._h, _vp(init_ptr or None), _vp(sums_ptr)))

    def decision_guard(self, rowstats_ptr: int, counts_ptr: int, scores_ptr: int):
        """(risk, switched) of the 16-bit decision check after a step whose
        exchange vectors are all-reduced (``fs_plan_decision_guard``);
        switched: the plan now runs on 32-bit operands -- run the step again."""
        risk = ctypes.c_double(-1.0)
        sw = _int(0)
        check(_lib.fs_plan_decision_guard(self._h, _vp(rowstats_ptr), _vp(counts_ptr),
                                          _vp(scores_ptr), ctypes.byref(risk), ctypes.byref(sw)))
        return float(risk.value), bool(sw.value)

    def set_rows(self, begin: int, end: int) -> None:
        """Score only the focal samples [begin, end) in the next pass2
        (``fs_plan_set_rows``; MultiSURF plans)."""
        check(_lib.fs_plan_set_rows(self._h, int(begin), int(end)))

    def info(self):
        """(owned tiles, pair-feature evaluations per step, pairs refined last step)."""
        tiles = ctypes.c_int64(0)
        pfe = ctypes.c_double(0.0)
        ref = ctypes.c_int64(0)
        check(_lib.fs_plan_info(self._h, ctypes.byref(tiles), ctypes.byref(pfe),
                                ctypes.byref(ref)))
        return int(tiles.value), float(pfe.value), int(ref.value)

    def set_shard(self, rank: int, world: int) -> None:
        """Re-target to the pair tiles of shard (rank, world) (fs_plan_set_shard)."""
        check(_lib.fs_plan_set_shard(self._h, int(rank), int(world)))

    def star_split(self) -> int:
        """The plan's star form (``fs_plan_star_split``): 1 = near pairs in
        pass 2 and the far part from per-column terms, 0 = dense star weights
        -- and 0 for every plan that never splits (no star, reference-order
        accumulation, ReliefF, the CPU backend).  The plans that share a
        MultiSURF* job must all be in one form."""
        v = _int(0)
        check(_lib.fs_plan_star_split(self._h, ctypes.byref(v)))
        return int(v.value)

    def set_star_split(self, split) -> None:
        """Put the plan into the star form its job agreed on
        (``fs_plan_set_star_split``), before the first ``pass1``.  ValueError
        when the split is asked of a plan that cannot take it."""
        check(_lib.fs_plan_set_star_split(self._h, int(bool(split))))

    def calibration(self) -> dict:
        """Refinement-band calibration of the current layout (fs_plan_calibration)."""
        v = (ctypes.c_double * 8)()
        m = _lib.fs_plan_calibration_ex(self._h, v, 8)
        check(min(m, 0))
        return {"q16": bool(v[0]), "rms": v[1], "max": v[2], "model_sigma": v[3],
                "band_vs_model": v[4], "guard": v[5] in (1.0, 2.0), "row_guard": v[5] == 2.0,
                "surf_f64": v[5] == 3.0, "row_bias_vs_limit": v[6], "SC": v[7]}

    def weighted_pairs(self) -> int:
        """Owned pairs with a non-zero weight in the last pass 2 (-1: not counted)."""
        v = ctypes.c_int64(-1)
        check(_lib.fs_plan_weighted_pairs(self._h, ctypes.byref(v)))
        return int(v.value)

    def kernel_ms(self, which: int) -> float:
        return float(_lib.fs_plan_kernel_ms(self._h, int(which)))

    def close(self) -> None:
        if self._h:
            _lib.fs_plan_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stir_statistics(sums, n_hit_pairs, n_miss_pairs):
    """The STIR epilogue (``fs_stir_statistics``) on the summed (4, n_kept)
    float64 sums with |H| and |M|: returns (hit_mean, miss_mean, t, df), the
    first three float64 arrays of n_kept.  ValueError when |H| < 2 or
    |M| < 2."""
    return stir_statistics_ex(sums, n_hit_pairs, n_miss_pairs)[:4]


def stir_statistics_ex(sums, n_hit_pairs, n_miss_pairs):
    """``stir_statistics`` and the pooled deviation sp per feature
    (``fs_stir_statistics_ex``): (hit_mean, miss_mean, t, df, pooled_sd)."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[0] != 4:
        raise ValueError(f"sums must have shape (4, n_kept); got {sums.shape}")
    k = sums.shape[1]
    hm, mm, t, sp = (np.zeros(k, dtype=np.float64) for _ in range(4))
    df = ctypes.c_double(0.0)
    check(_lib.fs_stir_statistics_ex(_p(sums, _f64p), k, float(n_hit_pairs), float(n_miss_pairs),
                                     _p(hm, _f64p), _p(mm, _f64p), _p(t, _f64p),
                                     ctypes.byref(df), _p(sp, _f64p)))
    return hm, mm, t, float(df.value), sp


class RowsPlan(Plan):
    """A ReliefF or SURF plan (``fs_plan_create_relieff`` / ``_surf``): X
    resident, focal samples ``rows``; ``score(ptr)`` writes the float64 score
    sums of those samples for the current feature subset (``set_features``)."""

    def __init__(self, backend, algo, x, y, recip, is_discrete, k=3, class_probs=None,
                 use_star=False, rows=None, n_jobs=-1, device=0, stream=0):
        super().__init__(None, None, None, None, None, _handle=True)
        self.backend = backend
        self.algo = algo
        self._h = _vp()
        rc_ = np.ascontiguousarray(recip, dtype=np.float32)
        isd = np.ascontiguousarray(is_discrete, dtype=np.uint8)
        yi = np.ascontiguousarray(y, dtype=np.int32)
        if algo == "relieff":
            x = np.ascontiguousarray(x, dtype=np.float32)
            self.n, self.p = x.shape
            lo, hi = (0, self.n) if rows is None else rows
            cp = np.ascontiguousarray(class_probs, dtype=np.float32)
            check(_lib.fs_plan_create_relieff(
                ctypes.byref(self._h), _backend_code(backend), int(device), _p(x, _f32p), self.n,
                self.p, _p(yi, _i32p), _p(rc_, _f32p), _p(isd, _u8p), int(k), _p(cp, _f32p),
                cp.size, int(lo), int(hi), int(n_jobs), ctypes.c_uint64(int(stream))))
        elif algo == "surf":
            x = np.ascontiguousarray(x, dtype=np.float64)
            self.n, self.p = x.shape
            lo, hi = (0, self.n) if rows is None else rows
            check(_lib.fs_plan_create_surf(
                ctypes.byref(self._h), _backend_code(backend), int(device), _p(x, _f64p), self.n,
                self.p, _p(yi, _i32p), _p(rc_, _f32p), int(bool(use_star)), _p(isd, _u8p),
                int(lo), int(hi), int(n_jobs), ctypes.c_uint64(int(stream))))
        else:
            raise ValueError(f"unknown algorithm {algo!r}")
        self.n_kept = self.p

    def score(self, sums_ptr: int) -> None:
        check(_lib.fs_plan_score(self._h, _vp(sums_ptr)))

    def score_stir(self, sums_ptr: int, stir_ptr: int, counts_ptr: int) -> None:
        """``score`` of a ReliefF plan and, over the same neighbour lists, the
        STIR sums into stir[4 * n_kept] (S1H, S2H, S1M, S2M per kept feature)
        and |H|, |M| into counts[2] (``fs_plan_score_stir``); all three in the
        memory space ``score`` writes to.  ``stir_kernel_ms(2)`` is the STIR
        kernel's time of the last call on the GPU."""
        check(_lib.fs_plan_score_stir(self._h, _vp(sums_ptr or None), _vp(stir_ptr or None),
                                      _vp(counts_ptr or None)))

    def score_labels(self, labels, scores_ptr: int) -> None:
        """The ReliefF score sums of the (B, n) int32 host labellings (class
        codes in [0, 64)) into scores[B * n_kept]
        (``fs_plan_relieff_score_labels``): pass 1 once, then selection and
        update per labelling; scores in the memory space ``score`` writes to.
        The plan's own labels are put back."""
        lab = _labels_arg(labels, self.n)
        check(_lib.fs_plan_relieff_score_labels(self._h, _p(lab, _i32p), lab.shape[0],
                                                _vp(scores_ptr or None)))

    def labels_info(self):
        """(fast-route labellings, general-route labellings, overflow reruns,
        candidate depth) of the last ``score_labels``
        (``fs_plan_relieff_labels_info``)."""
        v = np.zeros(4, dtype=np.int64)
        check(_lib.fs_plan_relieff_labels_info(self._h, _p(v, _i64p)))
        return tuple(int(q) for q in v)

    def labels_kernel_ms(self, which: int) -> float:
        """HIP-event time of the last ``score_labels``: 0 / 1 / 2 the candidate
        prefix, walk and score kernels, 3 the general route's selection and
        update (``fs_plan_relieff_labels_kernel_ms``; -1: unavailable)."""
        return float(_lib.fs_plan_relieff_labels_kernel_ms(self._h, int(which)))

    def surf_score_labels(self, labels, scores_ptr: int) -> None:
        """The SURF / SURF* score sums (as the plan's ``use_star``) of the
        (B, n) int32 host labellings into scores[B * n_kept]
        (``fs_plan_surf_score_labels``): distances, means and the near pairs
        once, then weights and score per chunk of labellings; scores in the
        memory space ``score`` writes to.  A later ``score`` is unchanged."""
        lab = _labels_arg(labels, self.n)
        check(_lib.fs_plan_surf_score_labels(self._h, _p(lab, _i32p), lab.shape[0],
                                             _vp(scores_ptr or None)))

    def surf_labels_info(self):
        """(weighted pairs listed, near sides, chunks walked, 1 if the star
        walk ran) of the last ``surf_score_labels``
        (``fs_plan_surf_labels_info``)."""
        v = np.zeros(4, dtype=np.int64)
        check(_lib.fs_plan_surf_labels_info(self._h, _p(v, _i64p)))
        return tuple(int(q) for q in v)

    def surf_labels_kernel_ms(self, which: int) -> float:
        """HIP-event time of the last ``surf_score_labels``: 0 distances +
        resolve + records, 1 weights, 2 the score kernel, 3 column sort + star
        walk (``fs_plan_surf_labels_kernel_ms``; -1: unavailable)."""
        return float(_lib.fs_plan_surf_labels_kernel_ms(self._h, int(which)))

    def score_targets(self, targets, s_a_ptr: int, s_ca_ptr: int, s_c_ptr: int) -> None:
        """The RReliefF sums of the (B, n) float64 host targets on a one-class
        ReliefF plan (``fs_plan_score_targets``): S_A into s_a[n_kept], S_CA
        into s_ca[B * n_kept], S_C into s_c[B], all three in the memory space
        ``score`` writes to.  Pass 1 and the selection run once per call."""
        t = _targets_arg(targets, self.n)
        check(_lib.fs_plan_score_targets(self._h, _p(t, _f64p), t.shape[0], _vp(s_a_ptr or None),
                                         _vp(s_ca_ptr or None), _vp(s_c_ptr or None)))

    def targets_kernel_ms(self, which: int) -> float:
        """HIP-event time of the last ``score_targets``: 0 the selection, 1
        the update kernel summed over the chunks of targets
        (``fs_plan_targets_kernel_ms``; -1: unavailable)."""
        return float(_lib.fs_plan_targets_kernel_ms(self._h, int(which)))

    def ref_temp(self) -> None:
        """Reference order: the score up to the float32 temp rows, whose column
        sums ``ref_sums`` continues (``fs_plan_ref_temp``; ReliefF, SURF)."""
        check(_lib.fs_plan_ref_temp(self._h))


def mdr_combinations(p: int, k: int) -> int:
    """C(p, k), the number of combinations ``mdr_scan`` scores
    (``fs_mdr_combinations``); ValueError above 2^62."""
    c = _i64(0)
    check(_lib.fs_mdr_combinations(int(p), int(k), ctypes.byref(c)))
    return int(c.value)


def mdr_unrank(p: int, k: int, rank: int):
    """The combination at ``rank`` in ``itertools.combinations(range(p), k)``
    order as a tuple of ints (``fs_mdr_unrank``): the reference's
    ``all_combos[rank]`` (MDR.py:283) without the list."""
    f = np.empty(int(k) if 1 <= int(k) <= 6 else 6, dtype=np.int32)
    check(_lib.fs_mdr_unrank(int(p), int(k), int(rank), _p(f, _i32p)))
    return tuple(int(v) for v in f[:k])


def mdr_scan(backend, x, is_case, k, fold=None, n_folds=0, device=0, n_jobs=-1, want_ba=False):
    """Balanced accuracy of every k-combination of the genotype columns of
    ``x`` (uint8, values 0/1/2) for all folds in one pass (``fs_mdr_scan``;
    replaces ``mdr_kernel`` / ``_batch_balanced_accuracy_cpu``, MDR.py:20-129).

    ``fold[i]`` is the fold whose test set holds sample i; ``fold=None``
    trains one scan on all samples.  Returns (best_ba float32[F], best_rank
    int64[F]) with F = max(n_folds, 1), plus the F x C(p,k) float32 array of
    every BA when ``want_ba`` (small jobs only)."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    if x.ndim != 2:
        raise ValueError("x must be a 2-D array")
    n, p = x.shape
    case = np.ascontiguousarray(is_case, dtype=np.uint8)
    if case.shape != (n,):
        raise ValueError("is_case must have one entry per row of x")
    fv = None
    if fold is not None:
        fv = np.ascontiguousarray(fold, dtype=np.int32)
        if fv.shape != (n,):
            raise ValueError("fold must have one entry per row of x")
    else:
        n_folds = 0
    nf = max(int(n_folds), 1)
    best_ba = np.zeros(nf, dtype=np.float32)
    best_rank = np.zeros(nf, dtype=np.int64)
    ba = None
    if want_ba:
        ba = np.zeros((nf, mdr_combinations(p, k)), dtype=np.float32)
    check(_lib.fs_mdr_scan(_backend_code(backend), int(device), _p(x, _u8p), n, p, _p(case, _u8p),
                           int(k), None if fv is None else _p(fv, _i32p), int(n_folds),
                           int(n_jobs), _p(best_ba, _f32p), _p(best_rank, _i64p),
                           None if ba is None else _p(ba, _f32p)))
    return (best_ba, best_rank, ba) if want_ba else (best_ba, best_rank)


def mdr_scan_labels(backend, x, labels, k, fold=None, n_folds=0, device=0, n_jobs=-1,
                    want_ba=False):
    """``mdr_scan`` for B labellings of one genotype matrix in one pass
    (``fs_mdr_scan_labels``): ``labels`` is B x n, nonzero = case, and the
    folds are shared.  Returns (best_ba float32[B, F], best_rank int64[B, F])
    with F = max(n_folds, 1), plus the B x F x C(p,k) float32 array of every BA
    when ``want_ba`` (small jobs only).  Row b equals ``mdr_scan(backend, x,
    labels[b], ...)`` bit for bit."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    if x.ndim != 2:
        raise ValueError("x must be a 2-D array")
    n, p = x.shape
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    if lab.ndim != 2 or lab.shape[1] != n:
        raise ValueError("labels must be 2-D with one column per row of x")
    nb = lab.shape[0]
    fv = None
    if fold is not None:
        fv = np.ascontiguousarray(fold, dtype=np.int32)
        if fv.shape != (n,):
            raise ValueError("fold must have one entry per row of x")
    else:
        n_folds = 0
    nf = max(int(n_folds), 1)
    best_ba = np.zeros((nb, nf), dtype=np.float32)
    best_rank = np.zeros((nb, nf), dtype=np.int64)
    ba = None
    if want_ba:
        ba = np.zeros((nb, nf, mdr_combinations(p, k)), dtype=np.float32)
    check(_lib.fs_mdr_scan_labels(_backend_code(backend), int(device), _p(x, _u8p), n, p,
                                  _p(lab, _u8p), nb, int(k),
                                  None if fv is None else _p(fv, _i32p), int(n_folds), int(n_jobs),
                                  _p(best_ba, _f32p), _p(best_rank, _i64p),
                                  None if ba is None else _p(ba, _f32p)))
    return (best_ba, best_rank, ba) if want_ba else (best_ba, best_rank)


def mdr_labels_last_timing():
    """(upload, pack, scan, download) milliseconds of this thread's last GPU
    ``mdr_scan_labels`` (``fs_mdr_labels_last_timing``; -1 where unavailable)."""
    v = np.full(4, -1.0)
    check(_lib.fs_mdr_labels_last_timing(_p(v, _f64p)))
    return tuple(float(t) for t in v)


MDR_MAX_TOP = 4096  # kMdrMaxTop (fs_mdr.h)


def mdr_scan_top(backend, x, is_case, k, fold=None, n_folds=0, n_top=100, device=0, n_jobs=-1):
    """The ``n_top`` best k-combinations of every fold (``fs_mdr_scan_top``):
    (top_ba float32[F, n_top], top_rank int64[F, n_top]) with F =
    max(n_folds, 1), each row ordered by (BA descending, rank ascending) --
    ``np.argsort(-ba[f], kind="stable")[:n_top]`` of ``mdr_scan``'s ``want_ba``
    array without that array.  Entries past C(p,k) are rank -1, BA 0; entry 0
    is ``mdr_scan``'s result.  ``n_top`` is at most ``MDR_MAX_TOP``."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    if x.ndim != 2:
        raise ValueError("x must be a 2-D array")
    n, p = x.shape
    case = np.ascontiguousarray(is_case, dtype=np.uint8)
    if case.shape != (n,):
        raise ValueError("is_case must have one entry per row of x")
    fv = None
    if fold is not None:
        fv = np.ascontiguousarray(fold, dtype=np.int32)
        if fv.shape != (n,):
            raise ValueError("fold must have one entry per row of x")
    else:
        n_folds = 0
    nf = max(int(n_folds), 1)
    rows = min(max(int(n_top), 1), MDR_MAX_TOP)  # the call rejects n_top outside this range
    top_ba = np.zeros((nf, rows), dtype=np.float32)
    top_rank = np.full((nf, rows), -1, dtype=np.int64)
    check(_lib.fs_mdr_scan_top(_backend_code(backend), int(device), _p(x, _u8p), n, p,
                               _p(case, _u8p), int(k), None if fv is None else _p(fv, _i32p),
                               int(n_folds), int(n_top), int(n_jobs), _p(top_ba, _f32p),
                               _p(top_rank, _i64p)))
    return top_ba, top_rank


def mdr_top_last_timing():
    """(upload, pack, scan, download) milliseconds of this thread's last GPU
    ``mdr_scan_top`` (``fs_mdr_top_last_timing``; -1 where unavailable); the
    scan phase holds both scans and the selection."""
    v = np.full(4, -1.0)
    check(_lib.fs_mdr_top_last_timing(_p(v, _f64p)))
    return tuple(float(t) for t in v)


MI_UNITS = {"bit": 0, "nat": 1}


def mi_matrices(backend, codes, ycodes, n_states, unit="bit", n_jobs=-1, device=0,
                want_counts=False):
    """Relevance I(X_f; y) and the p x p matrix of pairwise mutual information
    of state codes (``fs_mi_matrices``; replaces ``_batch_mi_cpu`` and
    ``_mi_pair_gpu_kernel``, mutual_information.py:49-115).

    ``codes`` (n x p) and ``ycodes`` (n) hold values in ``0..n_states-1``
    (uint8).  Returns (relevance float64[p], redundancy float64[p, p]), plus
    the int32 [p, p, n_states, n_states] contingency tables of the pairs
    i < j when ``want_counts`` (small jobs only)."""
    x = np.ascontiguousarray(codes, dtype=np.uint8)
    if x.ndim != 2:
        raise ValueError("codes must be a 2-D array")
    n, p = x.shape
    yv = np.ascontiguousarray(ycodes, dtype=np.uint8)
    if yv.shape != (n,):
        raise ValueError("ycodes must have one entry per row of codes")
    if unit not in MI_UNITS:
        raise ValueError("unit must be 'bit' or 'nat'")
    rel = np.zeros(p, dtype=np.float64)
    red = np.zeros((p, p), dtype=np.float64)
    cnt = None
    if want_counts:
        cnt = np.zeros((p, p, int(n_states), int(n_states)), dtype=np.int32)
    check(_lib.fs_mi_matrices(_backend_code(backend), int(device), _p(x, _u8p), _p(yv, _u8p), n, p,
                              int(n_states), MI_UNITS[unit], int(n_jobs), _p(rel, _f64p),
                              _p(red, _f64p), None if cnt is None else _p(cnt, _i32p)))
    return (rel, red, cnt) if want_counts else (rel, red)


def mi_last_timing():
    """(upload, pack, scan, download) milliseconds of this thread's last GPU
    ``mi_matrices`` (``fs_mi_last_timing``; -1 where unavailable)."""
    v = np.full(4, -1.0)
    check(_lib.fs_mi_last_timing(_p(v, _f64p)))
    return tuple(float(t) for t in v)


class Cfs:
    """A CFS handle (``fs_cfs_*``): the packed state codes of one fit, its
    class correlations, and rows of symmetrical uncertainty computed when the
    search selects their feature (replaces ``_precompute_correlations_cpu`` /
    ``_gpu_kernel`` and ``_best_first_search``, CFS.py:80-162, 219-243).

    ``codes`` (n x p) and ``ycodes`` (n) hold values in ``0..n_states-1``
    (uint8)."""

    def __init__(self, backend, codes, ycodes, n_states, n_jobs=-1, device=0):
        self._h = _vp()
        x = np.ascontiguousarray(codes, dtype=np.uint8)
        if x.ndim != 2:
            raise ValueError("codes must be a 2-D array")
        self.n, self.p = x.shape
        yv = np.ascontiguousarray(ycodes, dtype=np.uint8)
        if yv.shape != (self.n,):
            raise ValueError("ycodes must have one entry per row of codes")
        check(_lib.fs_cfs_create(ctypes.byref(self._h), _backend_code(backend), int(device),
                                 _p(x, _u8p), _p(yv, _u8p), self.n, self.p, int(n_states),
                                 int(n_jobs)))

    def relevance(self):
        """float32 [p]: SU(X_f, y) (``fs_cfs_relevance``)."""
        r = np.zeros(self.p, dtype=np.float32)
        check(_lib.fs_cfs_relevance(self._h, _p(r, _f32p)))
        return r

    def search(self, min_r_cf=0.1):
        """(selected int64 [k] in selection order, merits float64 [k]) of the
        best-first search (``fs_cfs_search``)."""
        sel = np.zeros(self.p, dtype=np.int64)
        mer = np.zeros(self.p, dtype=np.float64)
        k = _i64(0)
        check(_lib.fs_cfs_search(self._h, float(min_r_cf), _p(sel, _i64p), ctypes.byref(k),
                                 _p(mer, _f64p)))
        return sel[:k.value].copy(), mer[:k.value].copy()

    def row(self, feature):
        """float32 [p]: SU(feature, .) with the diagonal 0 (``fs_cfs_row``)."""
        r = np.zeros(self.p, dtype=np.float32)
        check(_lib.fs_cfs_row(self._h, int(feature), _p(r, _f32p)))
        return r

    def close(self) -> None:
        if self._h:
            _lib.fs_cfs_destroy(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cfs_search_matrix(backend, r_cf, r_ff, min_r_cf=0.1, device=0):
    """The best-first search of CFS on a caller's float32 ``r_cf`` [p] and
    symmetric ``r_ff`` [p, p] (``fs_cfs_search_matrix``; ``_best_first_search``,
    CFS.py:115-162).  Returns (selected int64 [k], merits float64 [k])."""
    rc_ = np.ascontiguousarray(r_cf, dtype=np.float32)
    rf = np.ascontiguousarray(r_ff, dtype=np.float32)
    p = rc_.shape[0]
    if rc_.ndim != 1 or rf.shape != (p, p):
        raise ValueError("r_cf must be a vector of p entries and r_ff p x p")
    sel = np.zeros(max(p, 1), dtype=np.int64)
    mer = np.zeros(max(p, 1), dtype=np.float64)
    k = _i64(0)
    check(_lib.fs_cfs_search_matrix(_backend_code(backend), int(device), _p(rc_, _f32p),
                                    _p(rf, _f32p), p, float(min_r_cf), _p(sel, _i64p),
                                    ctypes.byref(k), _p(mer, _f64p)))
    return sel[:k.value].copy(), mer[:k.value].copy()


def cfs_last_timing():
    """(upload, pack, relevance, rows, steps) milliseconds of this thread's
    last GPU ``Cfs`` handle (``fs_cfs_last_timing``; -1 where unavailable)."""
    v = np.full(5, -1.0)
    check(_lib.fs_cfs_last_timing(_p(v, _f64p)))
    return tuple(float(t) for t in v)


MRMR_METHODS = {"MID": 0, "MIQ": 1}


def mrmr_select(backend, codes, ycodes, n_states, k, method="MID", unit="bit", n_jobs=-1,
                device=0, want_rows=True):
    """mRMR's selection without the redundancy matrix (``fs_mrmr_select``;
    mRMR.py:96-117): the relevance, then per step one pick and one row of
    mutual information, k p pairs in all.

    ``codes`` (n x p) and ``ycodes`` (n) hold values in ``0..n_states-1``
    (uint8).  Returns (selected int64 [k] in selection order, relevance
    float64 [p], rows float64 [k, p] with ``rows[s] = I(.; X_selected[s])``, or
    None without ``want_rows``)."""
    x = np.ascontiguousarray(codes, dtype=np.uint8)
    if x.ndim != 2:
        raise ValueError("codes must be a 2-D array")
    n, p = x.shape
    yv = np.ascontiguousarray(ycodes, dtype=np.uint8)
    if yv.shape != (n,):
        raise ValueError("ycodes must have one entry per row of codes")
    if unit not in MI_UNITS:
        raise ValueError("unit must be 'bit' or 'nat'")
    if method not in MRMR_METHODS:
        raise ValueError("method must be 'MID' or 'MIQ'")
    k = int(k)
    rel = np.zeros(p, dtype=np.float64)
    sel = np.zeros(max(k, 1), dtype=np.int64)
    rows = np.zeros((k, p), dtype=np.float64) if want_rows and 1 <= k <= p else None
    check(_lib.fs_mrmr_select(_backend_code(backend), int(device), _p(x, _u8p), _p(yv, _u8p), n, p,
                              int(n_states), MI_UNITS[unit], MRMR_METHODS[method], k, int(n_jobs),
                              _p(rel, _f64p), _p(sel, _i64p),
                              None if rows is None else _p(rows, _f64p)))
    return sel[:k], rel, rows


def mrmr_search_matrix(backend, relevance, redundancy, k, method="MID", device=0):
    """The greedy loop of mRMR on a caller's float64 ``relevance`` [p] and
    symmetric ``redundancy`` [p, p] (``fs_mrmr_search_matrix``; mRMR.py:96-117).
    Returns selected int64 [k] in selection order."""
    rel = np.ascontiguousarray(relevance, dtype=np.float64)
    red = np.ascontiguousarray(redundancy, dtype=np.float64)
    p = rel.shape[0]
    if rel.ndim != 1 or red.shape != (p, p):
        raise ValueError("relevance must be a vector of p entries and redundancy p x p")
    if method not in MRMR_METHODS:
        raise ValueError("method must be 'MID' or 'MIQ'")
    k = int(k)
    sel = np.zeros(max(k, 1), dtype=np.int64)
    check(_lib.fs_mrmr_search_matrix(_backend_code(backend), int(device), _p(rel, _f64p),
                                     _p(red, _f64p), p, MRMR_METHODS[method], k, _p(sel, _i64p)))
    return sel[:k]


def mrmr_last_timing():
    """(upload, pack, relevance, rows, steps) milliseconds of this thread's
    last GPU ``mrmr_select`` (``fs_mrmr_last_timing``; -1 where unavailable)."""
    v = np.full(5, -1.0)
    check(_lib.fs_mrmr_last_timing(_p(v, _f64p)))
    return tuple(float(t) for t in v)


JMI_METHODS = {"JMI": 0, "CMIM": 1}


def _jmi_codes(codes, ycodes, unit):
    x = np.ascontiguousarray(codes, dtype=np.uint8)
    if x.ndim != 2:
        raise ValueError("codes must be a 2-D array")
    yv = np.ascontiguousarray(ycodes, dtype=np.uint8)
    if yv.shape != (x.shape[0],):
        raise ValueError("ycodes must have one entry per row of codes")
    if unit not in MI_UNITS:
        raise ValueError("unit must be 'bit' or 'nat'")
    return x, yv


def jmi_select(backend, codes, ycodes, n_states, k, method="JMI", unit="bit", n_jobs=-1,
               device=0, want_rows=True):
    """JMI / CMIM selection on lazy rows of joint relevance (``fs_jmi_select``):
    the relevance, then per step one pick and one row
    ``J(., s) = I(X_., X_s; y)``, k p joint tables in all.

    ``codes`` (n x p) and ``ycodes`` (n) hold values in ``0..n_states-1``
    (uint8).  Returns (selected int64 [k] in selection order, relevance
    float64 [p], rows float64 [k, p] with ``rows[s] = J(., selected[s])``, or
    None without ``want_rows``)."""
    x, yv = _jmi_codes(codes, ycodes, unit)
    n, p = x.shape
    if method not in JMI_METHODS:
        raise ValueError("method must be 'JMI' or 'CMIM'")
    k = int(k)
    rel = np.zeros(p, dtype=np.float64)
    sel = np.zeros(max(k, 1), dtype=np.int64)
    rows = np.zeros((k, p), dtype=np.float64) if want_rows and 1 <= k <= p else None
    check(_lib.fs_jmi_select(_backend_code(backend), int(device), _p(x, _u8p), _p(yv, _u8p), n, p,
                             int(n_states), MI_UNITS[unit], JMI_METHODS[method], k, int(n_jobs),
                             _p(rel, _f64p), _p(sel, _i64p),
                             None if rows is None else _p(rows, _f64p)))
    return sel[:k], rel, rows


def jmi_rows(backend, codes, ycodes, n_states, anchors, unit="bit", n_jobs=-1, device=0):
    """The joint relevance of chosen anchor columns with every column
    (``fs_jmi_rows``): float64 [m, p] with ``rows[t, c] = I(X_c, X_anchors[t]; y)``
    and 0.0 at ``c == anchors[t]``."""
    x, yv = _jmi_codes(codes, ycodes, unit)
    n, p = x.shape
    anc = np.ascontiguousarray(anchors, dtype=np.int64)
    if anc.ndim != 1:
        raise ValueError("anchors must be a vector of column indices")
    m = anc.shape[0]
    rows = np.zeros((m, p), dtype=np.float64)
    check(_lib.fs_jmi_rows(_backend_code(backend), int(device), _p(x, _u8p), _p(yv, _u8p), n, p,
                           int(n_states), MI_UNITS[unit], _p(anc, _i64p), m, int(n_jobs),
                           _p(rows, _f64p)))
    return rows


def jmi_search_matrix(backend, relevance, joint, k, method="JMI", device=0):
    """The greedy loop of JMI / CMIM on a caller's float64 ``relevance`` [p] and
    symmetric ``joint`` [p, p] (``fs_jmi_search_matrix``).  Returns selected
    int64 [k] in selection order."""
    rel = np.ascontiguousarray(relevance, dtype=np.float64)
    jm = np.ascontiguousarray(joint, dtype=np.float64)
    p = rel.shape[0]
    if rel.ndim != 1 or jm.shape != (p, p):
        raise ValueError("relevance must be a vector of p entries and joint p x p")
    if method not in JMI_METHODS:
        raise ValueError("method must be 'JMI' or 'CMIM'")
    k = int(k)
    sel = np.zeros(max(k, 1), dtype=np.int64)
    check(_lib.fs_jmi_search_matrix(_backend_code(backend), int(device), _p(rel, _f64p),
                                    _p(jm, _f64p), p, JMI_METHODS[method], k, _p(sel, _i64p)))
    return sel[:k]


def jmi_last_timing():
    """(upload, pack, relevance, rows, steps) milliseconds of this thread's
    last GPU ``jmi_select`` (``fs_jmi_last_timing``; -1 where unavailable)."""
    v = np.full(5, -1.0)
    check(_lib.fs_jmi_last_timing(_p(v, _f64p)))
    return tuple(float(t) for t in v)


PAIR_SCORES = {"joint": 0, "gain": 1}
PAIR_MAX_TOP = 65536


def pair_screen(backend, codes, ycodes, n_states, n_top=100, score="gain", unit="bit", n_jobs=-1,
                device=0, want_feature_best=True):
    """The ``n_top`` best of all C(p,2) column pairs (``fs_pair_screen``) by
    joint relevance ``J(i, j) = I(X_i, X_j; y)`` (``score="joint"``) or by the
    interaction gain ``(J(i, j) - rel[i]) - rel[j]`` (``score="gain"``), ordered
    by (score descending, rank in ``itertools.combinations`` ascending).

    ``codes`` (n x p) and ``ycodes`` (n) hold values in ``0..n_states-1``
    (uint8).  Returns (relevance float64 [p], top_score float64 [m], top_pairs
    int64 [m, 2] with i < j, feature_best float64 [p]: the largest score of any
    pair that contains the feature, or None without ``want_feature_best``), with
    ``m = min(n_top, C(p,2))``."""
    x, yv = _jmi_codes(codes, ycodes, unit)
    n, p = x.shape
    if score not in PAIR_SCORES:
        raise ValueError("score must be 'joint' or 'gain'")
    n_top = int(n_top)
    size = min(max(n_top, 1), PAIR_MAX_TOP)
    rel = np.zeros(p, dtype=np.float64)
    top_s = np.zeros(size, dtype=np.float64)
    top_i = np.full(size, -1, dtype=np.int64)
    top_j = np.full(size, -1, dtype=np.int64)
    fb = np.zeros(p, dtype=np.float64) if want_feature_best else None
    check(_lib.fs_pair_screen(_backend_code(backend), int(device), _p(x, _u8p), _p(yv, _u8p), n, p,
                              int(n_states), MI_UNITS[unit], PAIR_SCORES[score], n_top,
                              int(n_jobs), _p(rel, _f64p), _p(top_s, _f64p), _p(top_i, _i64p),
                              _p(top_j, _i64p), None if fb is None else _p(fb, _f64p)))
    m = min(n_top, p * (p - 1) // 2)
    return rel, top_s[:m], np.stack([top_i[:m], top_j[:m]], axis=1), fb


def pair_screen_last_timing():
    """(upload, pack, relevance, scan with selection, download) milliseconds of
    this thread's last GPU ``pair_screen`` (``fs_pair_screen_last_timing``; -1
    where unavailable)."""
    v = np.full(5, -1.0)
    check(_lib.fs_pair_screen_last_timing(_p(v, _f64p)))
    return tuple(float(t) for t in v)


PAIR_MAX_LABELINGS = 65535


def pair_screen_labels(backend, codes, labels, n_states, score="gain", unit="bit", n_jobs=-1,
                       device=0, want_relevance=False):
    """The best pair of the pair screen under each of B labellings of y in one
    pass (``fs_pair_screen_labels``): row b is what
    ``pair_screen(backend, codes, labels[b], n_states, n_top=1)`` returns first,
    bit for bit on the same backend.

    ``codes`` (n x p) and ``labels`` (B x n) hold values in ``0..n_states-1``
    (uint8); the rows of ``labels`` are arbitrary.  Returns (best_score float64
    [B], best_pairs int64 [B, 2] with i < j, relevance float64 [B, p] or None
    without ``want_relevance``)."""
    x = np.ascontiguousarray(codes, dtype=np.uint8)
    if x.ndim != 2:
        raise ValueError("codes must be a 2-D array")
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    if lab.ndim != 2 or lab.shape[1] != x.shape[0]:
        raise ValueError("labels must be a 2-D array with one column per row of codes")
    if unit not in MI_UNITS:
        raise ValueError("unit must be 'bit' or 'nat'")
    if score not in PAIR_SCORES:
        raise ValueError("score must be 'joint' or 'gain'")
    n, p = x.shape
    B = lab.shape[0]
    if not (1 <= B <= PAIR_MAX_LABELINGS):
        raise ValueError(f"the number of labellings must be in 1..{PAIR_MAX_LABELINGS}")
    best_s = np.zeros(B, dtype=np.float64)
    best_i = np.full(B, -1, dtype=np.int64)
    best_j = np.full(B, -1, dtype=np.int64)
    rel = np.zeros((B, p), dtype=np.float64) if want_relevance else None
    check(_lib.fs_pair_screen_labels(_backend_code(backend), int(device), _p(x, _u8p),
                                     _p(lab, _u8p), B, n, p, int(n_states), MI_UNITS[unit],
                                     PAIR_SCORES[score], int(n_jobs), _p(best_s, _f64p),
                                     _p(best_i, _i64p), _p(best_j, _i64p),
                                     None if rel is None else _p(rel, _f64p)))
    return best_s, np.stack([best_i, best_j], axis=1), rel


def pair_labels_last_timing():
    """(upload, pack, relevance, scan with reduction, download) milliseconds of
    this thread's last GPU ``pair_screen_labels``
    (``fs_pair_labels_last_timing``; -1 where unavailable)."""
    v = np.full(5, -1.0)
    check(_lib.fs_pair_labels_last_timing(_p(v, _f64p)))
    return tuple(float(t) for t in v)
