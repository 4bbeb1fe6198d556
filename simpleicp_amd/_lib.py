"""ctypes binding of libsimpleicp_hip.so (C ABI: include/simpleicp_hip.h).

There is NO CPU fallback anywhere in this package: if the shared library is missing, or no
gfx950 device is visible, the operations raise ``BackendError`` -- they never silently run on
the host.  (The CPU oracle under oracle/ is test infrastructure and is not imported here.)
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from functools import partial
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
# SICP_LIBRARY: load another build of the same ABI (the sanitizer build of tests/test_asan.py)
LIB_PATH = Path(os.environ["SICP_LIBRARY"]) if os.environ.get("SICP_LIBRARY") else PKG / "libsimpleicp_hip.so"

FIX, MOV = 0, 1
OK, ERR_INVALID, ERR_HIP, ERR_NO_DEVICE, ERR_TOO_FEW, ERR_NUMERIC, ERR_EXCHANGE = 0, -1, -2, -3, -4, -5, -6
XCHG_ALLGATHER_F64, XCHG_SUM_F64, XCHG_MIN_U64, XCHG_MAX_U64 = 1, 2, 3, 4
PART_CLOUD, PART_QUERIES = 0, 1
K_KNN1, K_KNNK, K_NORMALEQ, K_SELECT, K_XCHG = 0, 1, 2, 3, 4
ABI_VERSION = 7          # include/simpleicp_hip.h SICP_ABI_VERSION this binding was written for
KERNEL_NAMES = {K_KNN1: "match", K_KNNK: "knnk_scan", K_NORMALEQ: "solve", K_SELECT: "reject_select", K_XCHG: "exchange"}
MATCH_KERNELS = {0: "k_knn1_scan", 1: "k_knn1_fscan", 2: "k_grid_nn", 3: "k_knn1_frec", 5: "k_grid_nn16", 6: "k_grid_nn16f"}

EXPORTS = [
    "sicp_abi_version", "sicp_last_error", "sicp_device_count", "sicp_ctx_create", "sicp_ctx_destroy",
    "sicp_ctx_device_name", "sicp_cloud_upload", "sicp_cloud_upload_columns", "sicp_cloud_upload_start", "sicp_cloud_upload_wait", "sicp_cloud_size", "sicp_cloud_transform",
    "sicp_cloud_download", "sicp_cloud_download_columns", "sicp_cloud_download_both", "sicp_cloud_set_planarity", "sicp_knn", "sicp_select_in_range", "sicp_estimate_normals", "sicp_icp_setup", "sicp_icp_iterate",
    "sicp_icp_run", "sicp_icp_get_state", "sicp_icp_uncertainties", "sicp_icp_normal_equations", "sicp_params_to_H",
    "sicp_corr_match", "sicp_corr_reject_planarity", "sicp_corr_reject_distances", "sicp_estimate_parameters",
    "sicp_set_exchange", "sicp_comm_unique_id", "sicp_comm_init", "sicp_comm_destroy", "sicp_comm_activate", "sicp_comm_info", "sicp_device_memory", "sicp_set_partition", "sicp_ctx_stream", "sicp_lexmin_gathered", "sicp_timing_enable", "sicp_timing_reset", "sicp_timing_get", "sicp_match_work", "sicp_match_deferred", "sicp_tail_cycles", "sicp_tail_selection", "sicp_exchange_info", "sicp_knn_work", "sicp_last_match_kernel",
    "sicp_xyz_count", "sicp_xyz_read", "sicp_xyz_write",
]

# include/simpleicp_hip_batch.h: a companion ABI with a version of its own (the list above and ABI_VERSION stay as they are)
BATCH_EXPORTS = ["sicp_batch_version", "sicp_icp_run_batch", "sicp_ctx_lean"]
BATCH_VERSION = 1
BATCH_PATH_BATCHED, BATCH_PATH_FALLBACK = 1, 2

# include/simpleicp_hip_device.h: clouds in device memory, a companion ABI with a version of its own as well
DEVICE_EXPORTS = ["sicp_device_version", "sicp_cloud_upload_strided", "sicp_select_n_device", "sicp_select_positions",
                  "sicp_cloud_write_strided"]
DEVICE_VERSION = 1
DT_F32, DT_F64 = 1, 2

# include/simpleicp_hip_normals.h: rejection by the angle between normals, a companion ABI with a version of its own too
NORMALS_EXPORTS = ["sicp_normals_version", "sicp_cloud_set_normals", "sicp_normal_angle_set", "sicp_corr_reject_normal_angle",
                   "sicp_normal_angle_info", "sicp_normal_cache_read"]
NORMALS_VERSION = 1

# include/simpleicp_hip_voxel.h: at most one point per voxel, a companion ABI with a version of its own as well
VOXEL_EXPORTS = ["sicp_voxel_version", "sicp_voxel_select", "sicp_voxel_select_masked"]
VOXEL_VERSION = 1

# include/simpleicp_hip_eval.h: fitness, inlier RMSE and the information sums of a registration, the same kind of companion
EVAL_EXPORTS = ["sicp_eval_version", "sicp_evaluate"]
EVAL_VERSION = 1

# include/simpleicp_hip_outlier.h: the statistical and the radius outlier filter, the same kind of companion
OUTLIER_EXPORTS = ["sicp_outlier_version", "sicp_outlier_statistical", "sicp_outlier_radius", "sicp_outlier_radius_cells"]
OUTLIER_VERSION = 1
# include/simpleicp_hip_chain.h: what the device-chained loop of the last run did
CHAIN_EXPORTS = ["sicp_chain_version", "sicp_chain_info"]
CHAIN_VERSION = 1
OUTLIER_MAX_K = 128
OUTLIER_MAX_BOX_CELLS = 4096

# include/simpleicp_hip_fpfh.h: FPFH descriptors, the same kind of companion
FPFH_EXPORTS = ["sicp_fpfh_version", "sicp_fpfh"]
FPFH_VERSION = 1
FPFH_MAX_K = 128
FPFH_BINS = 33

# include/simpleicp_hip_global.h: descriptor matching and RANSAC poses, the same kind of companion
GLOBAL_EXPORTS = ["sicp_global_version", "sicp_feature_match", "sicp_ransac_triplets"]
GLOBAL_VERSION = 1
MATCH_MAX_DIM = 64

# include/simpleicp_hip_posefit.h: least-squares poses of matched rows, the same kind of companion
POSEFIT_EXPORTS = ["sicp_posefit_version", "sicp_pose_refit"]
POSEFIT_VERSION = 1
POSEFIT_MAX_ROUNDS = 64
POSEFIT_SWEEPS = 6

# include/simpleicp_hip_robust.h: robust poses of matched rows (graduated Geman-McClure weights), the same kind of companion
ROBUST_EXPORTS = ["sicp_robust_version", "sicp_pose_robust"]
ROBUST_VERSION = 1
ROBUST_MAX_ROUNDS = 256

# include/simpleicp_hip_consistency.h: matches pruned by pairwise length consistency (compatibility graph, core numbers), the same
# kind of companion
CONSISTENCY_EXPORTS = ["sicp_consistency_version", "sicp_match_consistency"]
CONSISTENCY_VERSION = 1
CONSISTENCY_MAX_ROWS = 32768

# include/simpleicp_hip_keypoints.h: ISS keypoints, the same kind of companion
KEYPOINTS_EXPORTS = ["sicp_keypoints_version", "sicp_keypoints"]
KEYPOINTS_VERSION = 1
KEYPOINTS_MAX_K = 128

# include/simpleicp_hip_cluster.h: DBSCAN labels, the same kind of companion
CLUSTER_EXPORTS = ["sicp_cluster_version", "sicp_cluster"]
CLUSTER_VERSION = 1

# include/simpleicp_hip_plane.h: planes of a cloud scored by their inliers and refitted on them, the same kind of companion
PLANE_EXPORTS = ["sicp_plane_version", "sicp_plane_triplets", "sicp_plane_refit"]
PLANE_VERSION = 1
PLANE_MAX_ROUNDS = 16

# include/simpleicp_hip_farthest.h: farthest point sampling, the same kind of companion
FARTHEST_EXPORTS = ["sicp_farthest_version", "sicp_farthest"]
FARTHEST_VERSION = 1
FARTHEST_ONE_LIMIT = 12288

# include/simpleicp_hip_orient.h: normals oriented consistently along a spanning forest of the k-NN graph, the same kind of companion
ORIENT_EXPORTS = ["sicp_orient_version", "sicp_orient"]
ORIENT_VERSION = 1

# include/simpleicp_hip_regions.h: smooth regions of a cloud, region growing over the normals, the same kind of companion
REGIONS_EXPORTS = ["sicp_regions_version", "sicp_regions"]
REGIONS_VERSION = 1

# include/simpleicp_hip_denoise.h: moving-least-squares smoothing, every point projected onto its neighbourhood's plane, the same
# kind of companion
DENOISE_EXPORTS = ["sicp_denoise_version", "sicp_denoise"]
DENOISE_VERSION = 1


class BackendError(RuntimeError):
    """The HIP backend is unavailable or a HIP call failed."""

    def __init__(self, message, code=None):
        super().__init__(message)
        self.code = code


class EvalRecord(C.Structure):
    """struct sicp_eval (contract (E)): 96 bytes."""
    _fields_ = [("n_queries", C.c_int64), ("n_inliers", C.c_int64), ("sum_d2", C.c_double), ("sum_p", C.c_double * 3),
                ("sum_pp", C.c_double * 6)]


class _Stats(C.Structure):
    """A call's record, one field per counter or moment: as_dict() gives them in the structure's order, the int64 fields as int,
    the doubles as float."""

    def as_dict(self):
        return {name: (float if kind is C.c_double else int)(getattr(self, name)) for name, kind in self._fields_}


def _stats_dict(st):
    """A call's record as a dict, whether the context returned one of the structures above or (another backend) a mapping."""
    return st.as_dict() if hasattr(st, "as_dict") else dict(st)


class OutlierStats(_Stats):
    """struct sicp_outlier_stats (contract (O)): 40 bytes."""
    _fields_ = [("n_candidates", C.c_int64), ("n_kept", C.c_int64), ("mean", C.c_double), ("std", C.c_double),
                ("threshold", C.c_double)]


class FpfhStats(_Stats):
    """struct sicp_fpfh_stats (contract (F)): 32 bytes."""
    _fields_ = [("n_points", C.c_int64), ("n_pairs", C.c_int64), ("n_void_pairs", C.c_int64), ("n_empty", C.c_int64)]


class MatchStats(_Stats):
    """struct sicp_match_stats (contract (M)): 24 bytes."""
    _fields_ = [("n_query", C.c_int64), ("n_target", C.c_int64), ("n_unmatched", C.c_int64)]


class RansacStats(_Stats):
    """struct sicp_ransac_stats (contract (R)): 40 bytes."""
    _fields_ = [("n_hypotheses", C.c_int64), ("n_void", C.c_int64), ("n_pruned", C.c_int64), ("best", C.c_int64),
                ("best_inliers", C.c_int64)]


class PosefitStats(_Stats):
    """struct sicp_posefit_stats (contract (L)): 40 bytes."""
    _fields_ = [("n_poses", C.c_int64), ("n_void", C.c_int64), ("n_improved", C.c_int64), ("best", C.c_int64),
                ("best_inliers", C.c_int64)]


class RobustStats(_Stats):
    """struct sicp_robust_stats (contract (G)): 32 bytes."""
    _fields_ = [("n_poses", C.c_int64), ("n_void", C.c_int64), ("best", C.c_int64), ("best_inliers", C.c_int64)]


class ConsistencyStats(_Stats):
    """struct sicp_consistency_stats (contract (C)): 56 bytes."""
    _fields_ = [(name, C.c_int64) for name in ("n_rows", "n_valid", "n_edges", "max_degree", "max_core", "n_max_core", "n_subrounds")]


class KeypointStats(_Stats):
    """struct sicp_keypoint_stats (contract (I)): 48 bytes."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_salient", "n_keypoints", "n_small", "n_clipped_salient", "n_clipped_nms")]


class ClusterStats(_Stats):
    """struct sicp_cluster_stats (contract (U)): 56 bytes."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_core", "n_border", "n_noise", "n_clusters", "largest_label", "largest_size")]


class PlaneStats(_Stats):
    """struct sicp_plane_stats (contract (P)): 48 bytes."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_candidates", "n_hypotheses", "n_void", "best", "best_inliers")]


class PlaneRefitStats(_Stats):
    """struct sicp_plane_refit_stats (contract (Q)): 40 bytes."""
    _fields_ = [(name, C.c_int64) for name in ("n_planes", "n_void", "n_improved", "best", "best_inliers")]


class FarthestStats(_Stats):
    """struct sicp_farthest_stats (contract (S)): 32 bytes."""
    _fields_ = [("n_points", C.c_int64), ("n_candidates", C.c_int64), ("n_selected", C.c_int64), ("cover_d2", C.c_double)]


class OrientStats(_Stats):
    """struct sicp_orient_stats (contract (H)): 56 bytes."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_void", "n_components", "n_forest_edges", "n_flipped", "n_components_voted",
                                                "rounds")]


class RegionsStats(_Stats):
    """struct sicp_regions_stats (contract (J)): 72 bytes."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_void", "n_smooth", "n_border", "n_regions_all", "n_regions", "n_labelled",
                                                "largest_label", "largest_size")]


class DenoiseStats(_Stats):
    """struct sicp_denoise_stats (contract (W)): 40 bytes."""
    _fields_ = [("n_points", C.c_int64), ("n_small", C.c_int64), ("n_moved", C.c_int64), ("n_clipped", C.c_int64),
                ("max_displacement", C.c_double)]


class IterParams(C.Structure):
    _fields_ = [("x", C.c_double * 6), ("obs", C.c_double * 6), ("obs_weight", C.c_double * 6),
                ("min_planarity", C.c_double), ("distance_weight", C.c_double), ("max_lm_steps", C.c_int64)]


class IterResult(C.Structure):
    _fields_ = [("x", C.c_double * 6), ("H", C.c_double * 16), ("n_queries", C.c_int64),
                ("n_planar", C.c_int64), ("n_kept", C.c_int64), ("median", C.c_double), ("mad", C.c_double),
                ("dist_mean", C.c_double), ("dist_std", C.c_double), ("res_mean", C.c_double),
                ("res_std", C.c_double), ("weight_used", C.c_double), ("cost", C.c_double),
                ("lm_steps", C.c_int64), ("ne_evals", C.c_int64)]


class BatchMember(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("params", IterParams), ("max_iterations", C.c_int64), ("min_change", C.c_double),
                ("results", C.POINTER(IterResult)), ("iterations", C.c_int64), ("status", C.c_int), ("path", C.c_int),
                ("error", C.c_char * 256)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)

_vp, _i64, _dbl, _cint = C.c_void_p, C.c_int64, C.c_double, C.c_int


# one companion header: its exports (the version function first), the header's file name, the noun of its entry points in the
# messages, the version this binding needs (None: _feature_version reports whatever the library says), the argtypes of the exports
# that take arguments
_Feature = namedtuple("_Feature", "exports header noun version argtypes")

FEATURES = {
    "batch": _Feature(BATCH_EXPORTS, "simpleicp_hip_batch.h", "batch", None, {
        "sicp_icp_run_batch": [C.POINTER(BatchMember), _i64, C.POINTER(_i64)],
        "sicp_ctx_lean": [_vp]}),
    "device": _Feature(DEVICE_EXPORTS, "simpleicp_hip_device.h", "device-cloud", DEVICE_VERSION, {
        "sicp_cloud_upload_strided": [_vp, _cint, _vp, _cint, _i64, _i64, _i64, _i64],
        "sicp_select_n_device": [_vp, _vp, _i64, _i64, _vp, C.POINTER(_i64)],
        "sicp_select_positions": [_i64, _i64, _vp, C.POINTER(_i64)],
        "sicp_cloud_write_strided": [_vp, _cint, _vp, _vp, _cint, _i64, _i64]}),
    "normals": _Feature(NORMALS_EXPORTS, "simpleicp_hip_normals.h", "normal-angle", NORMALS_VERSION, {
        "sicp_cloud_set_normals": [_vp, _cint, _vp, _vp, _i64, _i64],
        "sicp_normal_angle_set": [_vp, _dbl, _cint],
        "sicp_corr_reject_normal_angle": [_vp, _dbl, _cint, _vp, _vp, C.POINTER(_i64)],
        "sicp_normal_angle_info": [_vp, _vp],
        "sicp_normal_cache_read": [_vp, _vp, _vp]}),
    "voxel": _Feature(VOXEL_EXPORTS, "simpleicp_hip_voxel.h", "voxel", VOXEL_VERSION, {
        "sicp_voxel_select": [_vp, _cint, _vp, _i64, _dbl, _vp, _vp, C.POINTER(_i64)],
        "sicp_voxel_select_masked": [_vp, _cint, _vp, _i64, _dbl, _vp, _vp, C.POINTER(_i64)]}),
    "evaluation": _Feature(EVAL_EXPORTS, "simpleicp_hip_eval.h", "evaluation", EVAL_VERSION, {
        "sicp_evaluate": [_vp, _cint, _cint, _vp, _i64, _vp, _dbl, C.POINTER(EvalRecord)]}),
    "outlier": _Feature(OUTLIER_EXPORTS, "simpleicp_hip_outlier.h", "outlier", OUTLIER_VERSION, {
        "sicp_outlier_statistical": [_vp, _cint, _vp, _i64, _vp, _cint, _dbl, _vp, _vp, C.POINTER(OutlierStats)],
        "sicp_outlier_radius": [_vp, _cint, _vp, _i64, _vp, _dbl, _i64, _vp, _vp, C.POINTER(_i64)],
        "sicp_outlier_radius_cells": [_vp, _cint, _dbl, _vp]}),
    "chain": _Feature(CHAIN_EXPORTS, "simpleicp_hip_chain.h", "chain", CHAIN_VERSION, {
        "sicp_chain_info": [_vp, _vp]}),
    "fpfh": _Feature(FPFH_EXPORTS, "simpleicp_hip_fpfh.h", "FPFH", FPFH_VERSION, {
        "sicp_fpfh": [_vp, _cint, _vp, _cint, _dbl, _vp, _vp, _vp, C.POINTER(FpfhStats)]}),
    "global": _Feature(GLOBAL_EXPORTS, "simpleicp_hip_global.h", "global-registration", GLOBAL_VERSION, {
        "sicp_feature_match": [_vp, _vp, _i64, _vp, _i64, _cint, _vp, _vp, C.POINTER(MatchStats)],
        "sicp_ransac_triplets": [_vp, _vp, _vp, _i64, _vp, _i64, _dbl, _dbl, _vp, _vp, C.POINTER(RansacStats)]}),
    "posefit": _Feature(POSEFIT_EXPORTS, "simpleicp_hip_posefit.h", "pose-refit", POSEFIT_VERSION, {
        "sicp_pose_refit": [_vp, _vp, _vp, _i64, _vp, _i64, _dbl, _cint, _vp, _vp, C.POINTER(PosefitStats)]}),
    "robust": _Feature(ROBUST_EXPORTS, "simpleicp_hip_robust.h", "robust-pose", ROBUST_VERSION, {
        "sicp_pose_robust": [_vp, _vp, _vp, _i64, _vp, _i64, _dbl, _cint, _dbl, _dbl, _vp, _vp, _vp, C.POINTER(RobustStats)]}),
    "consistency": _Feature(CONSISTENCY_EXPORTS, "simpleicp_hip_consistency.h", "match-consistency", CONSISTENCY_VERSION, {
        "sicp_match_consistency": [_vp, _vp, _vp, _i64, _dbl, _dbl, _vp, _vp, C.POINTER(ConsistencyStats)]}),
    "keypoints": _Feature(KEYPOINTS_EXPORTS, "simpleicp_hip_keypoints.h", "keypoint", KEYPOINTS_VERSION, {
        "sicp_keypoints": [_vp, _cint, _cint, _dbl, _cint, _dbl, _dbl, _dbl, _i64, _vp, _vp, _vp, C.POINTER(KeypointStats)]}),
    "cluster": _Feature(CLUSTER_EXPORTS, "simpleicp_hip_cluster.h", "cluster", CLUSTER_VERSION, {
        "sicp_cluster": [_vp, _cint, _dbl, _i64, _vp, _vp, C.POINTER(ClusterStats)]}),
    "plane": _Feature(PLANE_EXPORTS, "simpleicp_hip_plane.h", "plane", PLANE_VERSION, {
        "sicp_plane_triplets": [_vp, _vp, _i64, _vp, _vp, _i64, _dbl, _vp, _vp, C.POINTER(PlaneStats)],
        "sicp_plane_refit": [_vp, _vp, _i64, _vp, _vp, _i64, _dbl, _cint, _vp, _vp, _vp, C.POINTER(PlaneRefitStats)]}),
    "farthest": _Feature(FARTHEST_EXPORTS, "simpleicp_hip_farthest.h", "farthest-point", FARTHEST_VERSION, {
        "sicp_farthest": [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, C.POINTER(FarthestStats)]}),
    "orient": _Feature(ORIENT_EXPORTS, "simpleicp_hip_orient.h", "normal-orientation", ORIENT_VERSION, {
        "sicp_orient": [_vp, _cint, _vp, _cint, _vp, _cint, _vp, _vp, C.POINTER(OrientStats)]}),
    "regions": _Feature(REGIONS_EXPORTS, "simpleicp_hip_regions.h", "smooth-region", REGIONS_VERSION, {
        "sicp_regions": [_vp, _cint, _vp, _cint, _dbl, _dbl, _cint, _vp, _i64, _vp, C.POINTER(RegionsStats)]}),
    "denoise": _Feature(DENOISE_EXPORTS, "simpleicp_hip_denoise.h", "denoising", DENOISE_VERSION, {
        "sicp_denoise": [_vp, _cint, _cint, _dbl, _dbl, _dbl, _i64, _vp, _vp, _vp, C.POINTER(DenoiseStats)]}),
}

_lib = None


def load():
    """dlopen the library (building it first if hipcc is around and it is stale)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        try:
            from . import build as _build
            _build.build()
        except Exception as exc:  # noqa: BLE001
            raise BackendError(f"{LIB_PATH} is missing and could not be built ({exc}); "
                               "run `python -m simpleicp_amd.build`") from exc
    try:
        L = C.CDLL(str(LIB_PATH))
    except OSError as exc:
        raise BackendError(f"cannot load {LIB_PATH}: {exc}") from exc
    vp, i64, dbl, cint = _vp, _i64, _dbl, _cint
    L.sicp_abi_version.restype = cint
    if L.sicp_abi_version() != ABI_VERSION:
        # (SICP_LIBRARY makes it easy to point at a stale build: its entry points would be called with the wrong arguments)
        raise BackendError(f"{LIB_PATH} implements ABI version {L.sicp_abi_version()}, this binding needs {ABI_VERSION}; "
                           "rebuild with `python -m simpleicp_amd.build`")
    L.sicp_last_error.restype = C.c_char_p
    L.sicp_device_count.argtypes = [C.POINTER(cint)]
    L.sicp_ctx_create.argtypes = [cint, C.POINTER(vp)]
    L.sicp_ctx_destroy.argtypes = [vp]
    L.sicp_ctx_device_name.argtypes = [vp, C.c_char_p, cint]
    L.sicp_cloud_upload.argtypes = [vp, cint, vp, i64, i64]
    L.sicp_cloud_upload_columns.argtypes = [vp, cint, vp, vp, vp, i64, i64]
    L.sicp_cloud_upload_start.argtypes = [vp, cint, vp, vp, vp, vp, i64, i64]
    L.sicp_cloud_upload_wait.argtypes = [vp, cint]
    L.sicp_cloud_size.argtypes = [vp, cint, C.POINTER(i64)]
    L.sicp_cloud_transform.argtypes = [vp, cint, vp]
    L.sicp_cloud_download.argtypes = [vp, cint, vp]
    L.sicp_cloud_download_columns.argtypes = [vp, cint, vp, vp, vp]
    L.sicp_cloud_download_both.argtypes = [vp, cint, vp, vp, vp, vp]
    L.sicp_cloud_set_planarity.argtypes = [vp, cint, vp, vp, i64, i64]
    L.sicp_knn.argtypes = [vp, cint, vp, i64, cint, vp, dbl, vp, vp]
    L.sicp_select_in_range.argtypes = [vp, cint, cint, vp, i64, vp, dbl, vp]
    L.sicp_estimate_normals.argtypes = [vp, cint, vp, i64, cint, vp, vp, vp]
    L.sicp_icp_setup.argtypes = [vp, vp, i64, vp, vp]
    L.sicp_icp_iterate.argtypes = [vp, C.POINTER(IterParams), C.POINTER(IterResult)]
    L.sicp_icp_run.argtypes = [vp, C.POINTER(IterParams), i64, dbl, C.POINTER(IterResult), C.POINTER(i64)]
    L.sicp_icp_get_state.argtypes = [vp, vp, vp, vp, vp]
    L.sicp_icp_uncertainties.argtypes = [vp, vp]
    L.sicp_icp_normal_equations.argtypes = [vp, vp, vp]
    L.sicp_params_to_H.argtypes = [vp, vp]
    L.sicp_corr_match.argtypes = [vp, vp, vp, vp]
    L.sicp_corr_reject_planarity.argtypes = [vp, dbl, vp, vp, C.POINTER(i64)]
    L.sicp_corr_reject_distances.argtypes = [vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(i64)]
    L.sicp_estimate_parameters.argtypes = [vp, C.POINTER(IterParams), vp, C.POINTER(IterResult)]
    L.sicp_set_exchange.argtypes = [vp, EXCHANGE_FN, vp, cint, cint, cint]
    L.sicp_comm_unique_id.argtypes = [vp]
    L.sicp_comm_init.argtypes = [vp, vp, cint, cint, cint]
    L.sicp_comm_destroy.argtypes = [vp]
    L.sicp_comm_activate.argtypes = [vp, cint, cint]
    L.sicp_comm_info.argtypes = [vp, C.POINTER(cint * 6)]
    L.sicp_device_memory.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.sicp_set_partition.argtypes = [vp, cint]
    L.sicp_ctx_stream.argtypes = [vp, C.POINTER(vp)]
    L.sicp_lexmin_gathered.argtypes = [vp, vp, cint, i64, vp, vp, vp]
    L.sicp_timing_enable.argtypes = [vp, cint]
    L.sicp_timing_reset.argtypes = [vp]
    L.sicp_match_work.argtypes = [vp, vp]
    L.sicp_match_deferred.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.sicp_tail_cycles.argtypes = [vp, vp]
    L.sicp_tail_selection.argtypes = [vp, vp]
    L.sicp_exchange_info.argtypes = [vp, vp]
    L.sicp_knn_work.argtypes = [vp, vp]
    L.sicp_last_match_kernel.argtypes = [vp, C.POINTER(cint)]
    L.sicp_xyz_count.argtypes = [C.c_char_p, C.POINTER(i64)]
    L.sicp_xyz_read.argtypes = [C.c_char_p, vp, i64, C.POINTER(i64), cint]
    L.sicp_xyz_write.argtypes = [C.c_char_p, vp, i64, cint, cint, C.c_char_p, cint]
    L.sicp_timing_get.argtypes = [vp, cint, C.POINTER(dbl), C.POINTER(i64)]
    for name in EXPORTS:
        if name != "sicp_last_error":
            getattr(L, name).restype = cint
    for feature in FEATURES.values():
        # (a library that predates a companion header loads all the same: _feature_version reports it when the feature is asked for)
        if all(hasattr(L, name) for name in feature.exports):
            for name in feature.exports:
                getattr(L, name).restype = cint
                if name in feature.argtypes:
                    getattr(L, name).argtypes = feature.argtypes[name]
    _lib = L
    return L


def _ptr(a):
    """numpy array / torch tensor / address as an int / None -> void* (host-or-device pointer)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if hasattr(a, "data_ptr"):          # torch.Tensor (host or device)
        return C.c_void_p(a.data_ptr())
    if isinstance(a, (int, np.integer)):
        return C.c_void_p(int(a))
    raise TypeError(f"unsupported buffer type {type(a)}")


def _chk(L, rc):
    if rc != OK:
        raise BackendError(L.sicp_last_error().decode(), rc)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _matched_rows(src, dst):
    """The matched rows of a host-form call as float64 arrays, and whether both are (m, 3)."""
    s, d = _f64(src), _f64(dst)
    return s, d, s.ndim == 2 and s.shape[1] == 3 and d.shape == s.shape


def _pose_call_arrays(src, dst, poses):
    """Host form of pose_refit / pose_robust: the checked arrays (poses None: one pose), and the (b, 12) poses and (b,) inliers
    that leave."""
    s, d, ok = _matched_rows(src, dst)
    p = None if poses is None else _f64(poses)
    if not ok or (p is not None and (p.ndim != 2 or p.shape[1] != 12)):
        raise ValueError("src and dst must be (m, 3), poses (b, 12) or None")
    b = 1 if p is None else p.shape[0]
    return s, d, p, np.empty((b, 12), np.float64), np.empty(b, np.int32)


def _cloud_rows(X, mask):
    """Host form of plane_triplets / plane_refit: the (n, 3) float64 rows and the (n,) uint8 mask (None: every row), checked."""
    x = _f64(X)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError("X must be (n, 3)")
    m = None
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask) != 0).view(np.uint8)
        if m.shape != (x.shape[0],):
            raise ValueError(f"mask must have shape ({x.shape[0]},), not {m.shape}")
    return x, m


def device_count():
    n = C.c_int(0)
    load().sicp_device_count(C.byref(n))
    return n.value


def params_to_H(x):
    H = np.empty(16)
    load().sicp_params_to_H(_ptr(_f64(x)), _ptr(H))
    return H.reshape(4, 4)


def _feature_version(name):
    """The version the loaded library reports for the companion header FEATURES[name]; BackendError when it lacks one of the
    header's entry points, or implements another version than this binding needs."""
    L, f = load(), FEATURES[name]
    missing = [export for export in f.exports if not hasattr(L, export)]
    if missing:
        raise BackendError(f"{LIB_PATH} has no {f.noun} entry points ({', '.join(missing)}): it predates include/{f.header}; "
                           "rebuild with `python -m simpleicp_amd.build`")
    v = getattr(L, f.exports[0])()
    if f.version is not None and v != f.version:
        raise BackendError(f"{LIB_PATH} implements {name} version {v}, this binding needs {f.version}")
    return v


# SICP_<X>_VERSION of the loaded library; BackendError when it lacks the header's entry points or implements another version
batch_version = partial(_feature_version, "batch")             # (any version: icp_run_batch checks it)
device_version = partial(_feature_version, "device")
normals_version = partial(_feature_version, "normals")
voxel_version = partial(_feature_version, "voxel")
eval_version = partial(_feature_version, "evaluation")
outlier_version = partial(_feature_version, "outlier")
fpfh_version = partial(_feature_version, "fpfh")
global_version = partial(_feature_version, "global")
posefit_version = partial(_feature_version, "posefit")
robust_version = partial(_feature_version, "robust")
consistency_version = partial(_feature_version, "consistency")
keypoints_version = partial(_feature_version, "keypoints")
cluster_version = partial(_feature_version, "cluster")
plane_version = partial(_feature_version, "plane")
farthest_version = partial(_feature_version, "farthest")
orient_version = partial(_feature_version, "orient")
regions_version = partial(_feature_version, "regions")
denoise_version = partial(_feature_version, "denoise")


def select_positions(m, Q):
    """The positions among m kept rows that select_n_points(Q) picks (sicp_select_positions; host only): int64 vector."""
    device_version()
    L = load()
    out = np.empty(max(min(int(m), int(Q)), 1), np.int64)
    cnt = C.c_int64()
    _chk(L, L.sicp_select_positions(int(m), int(Q), _ptr(out), C.byref(cnt)))
    return out[:cnt.value]


class BatchRun:
    """One member's outcome of icp_run_batch: the per-iteration IterResults, the status, the message of a failure, the path."""

    def __init__(self, results, status, error, path):
        self.results, self.status, self.error, self.path = results, status, error, path

    def raise_for_status(self):
        """The BackendError (with `.results`) Context.icp_run would have raised, if any."""
        if self.status != OK:
            err = BackendError(self.error, self.status)
            err.results = self.results
            raise err


def icp_run_batch(members):
    """sicp_icp_run_batch over [(Context, icp_run keyword arguments), ...]: every member's loop behind one call.
    Returns ([BatchRun per member, in order], fallback_count); raises BackendError on a batch-wide error (nothing ran then)."""
    if batch_version() != BATCH_VERSION:
        raise BackendError(f"{LIB_PATH} implements batch version {load().sicp_batch_version()}, this binding needs {BATCH_VERSION}")
    arr = (BatchMember * max(len(members), 1))()
    keep = []
    for i, (ctx, kw) in enumerate(members):
        m = arr[i]
        m.ctx = ctx._h.value
        m.params = ctx._params(kw.get("x"), kw.get("obs"), kw.get("obs_weight"), kw.get("min_planarity", 0.3),
                               kw.get("distance_weight", 1.0), kw.get("max_lm_steps", 0))
        n = int(kw.get("max_iterations", 100))
        res = (IterResult * max(n, 1))()
        keep.append(res)
        m.results = C.cast(res, C.POINTER(IterResult))
        m.max_iterations = n
        m.min_change = float(kw.get("min_change", 1.0))
    fb = C.c_int64()
    L = load()
    _chk(L, L.sicp_icp_run_batch(arr, len(members), C.byref(fb)))
    out = []
    for i in range(len(members)):
        m = arr[i]
        out.append(BatchRun([keep[i][j] for j in range(m.iterations)], m.status, m.error.decode(), m.path))
    return out, fb.value


class Context:
    """One GPU context (= one `sicp_ctx`): device-resident clouds + ICP iteration state."""

    def __init__(self, device=0):
        self._L = load()
        self._h = C.c_void_p()
        self._cb = None
        rc = self._L.sicp_ctx_create(int(device), C.byref(self._h))
        if rc != OK:
            self._h = C.c_void_p()
            raise BackendError(self._L.sicp_last_error().decode(), rc)
        self.device = int(device)
        self._corr_owner = None      # the CorrPts object whose correspondences the context holds (simpleicp_amd/corrpts.py)
        self._bg_src = {}            # slot -> the host arrays an upload_start is still reading (kept alive until the slot's next upload)

    # -- plumbing --
    def _chk(self, rc):
        _chk(self._L, rc)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.sicp_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def device_name(self):
        buf = C.create_string_buffer(256)
        self._chk(self._L.sicp_ctx_device_name(self._h, buf, 256))
        return buf.value.decode()

    def make_lean(self):
        """A lean batch member (sicp_ctx_lean): its staged uploads and download_both share ONE pinned ring with the process's other
        lean contexts instead of a 48 MiB ring of its own."""
        batch_version()
        self._chk(self._L.sicp_ctx_lean(self._h))

    # -- clouds --
    def upload(self, slot, xyz, index_base=0):
        """xyz: (n,3) float64 numpy array or CUDA/host torch tensor."""
        if isinstance(xyz, np.ndarray):
            xyz = _f64(xyz)
        n = int(xyz.shape[0])
        if tuple(xyz.shape) != (n, 3):
            raise ValueError("cloud must have shape (n, 3)")
        self._chk(self._L.sicp_cloud_upload(self._h, slot, _ptr(xyz), n, int(index_base)))

    def upload_strided(self, slot, ptr, dtype, n, row_stride, col_stride, index_base=0):
        """(n, 3) points of a strided view in device memory (sicp_cloud_upload_strided): ptr a device address, dtype DT_F32 /
        DT_F64, strides in elements."""
        device_version()
        self._chk(self._L.sicp_cloud_upload_strided(self._h, slot, C.c_void_p(int(ptr)), int(dtype), int(n), int(row_stride),
                                                     int(col_stride), int(index_base)))

    def write_strided(self, slot, H, ptr, dtype, row_stride, col_stride):
        """The slot's points under H into a strided (n, 3) view in device memory (sicp_cloud_write_strided); the slot is unchanged."""
        device_version()
        self._chk(self._L.sicp_cloud_write_strided(self._h, slot, _ptr(_f64(H).reshape(16)), C.c_void_p(int(ptr)), int(dtype),
                                                   int(row_stride), int(col_stride)))

    def select_n_device(self, mask_ptr, n, Q, sel_ptr):
        """sicp_select_n_device: rows of a device mask (n bytes; None = all rows) picked as select_n_points(Q) picks them, into
        device memory at sel_ptr (Q int64).  Returns how many were picked."""
        device_version()
        q = C.c_int64()
        self._chk(self._L.sicp_select_n_device(self._h, None if mask_ptr is None else C.c_void_p(int(mask_ptr)), int(n), int(Q),
                                               C.c_void_p(int(sel_ptr)), C.byref(q)))
        return q.value

    def select_in_range_into(self, query_slot, search_slot, H, max_range, out_ptr):
        """select_in_range over ALL points of query_slot with the verdicts left in device memory (out_ptr: one byte per point)."""
        Hp = None if H is None else _f64(H).reshape(16)
        self._chk(self._L.sicp_select_in_range(self._h, query_slot, search_slot, None, self.size(query_slot), _ptr(Hp),
                                               float(max_range), C.c_void_p(int(out_ptr))))

    def estimate_normals_into(self, slot, sel_ptr, Q, k, normals_ptr, planarity_ptr):
        """estimate_normals with the selection and both outputs in device memory ((Q, 3) / (Q) float32)."""
        self._chk(self._L.sicp_estimate_normals(self._h, slot, C.c_void_p(int(sel_ptr)), int(Q), int(k),
                                                C.c_void_p(int(normals_ptr)), C.c_void_p(int(planarity_ptr)), None))

    def icp_setup_device(self, sel_ptr, Q, normals_ptr, planarity_ptr):
        """icp_setup from device memory (selection (Q) int64, normals (Q, 3) and planarity (Q) float32)."""
        self._chk(self._L.sicp_icp_setup(self._h, C.c_void_p(int(sel_ptr)), int(Q), C.c_void_p(int(normals_ptr)),
                                         C.c_void_p(int(planarity_ptr))))
        self._Q = int(Q)

    def upload_columns(self, slot, x, y, z, index_base=0):
        """x, y, z: contiguous float64 vectors of one length (no (n,3) gather on the host)."""
        cols = [_f64(np.asarray(v)) for v in (x, y, z)]
        n = len(cols[0])
        if any(v.ndim != 1 or len(v) != n for v in cols):
            raise ValueError("x, y, z must be vectors of the same length")
        self._chk(self._L.sicp_cloud_upload_columns(self._h, slot, _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), n,
                                                    int(index_base)))

    def upload_start(self, slot, xyz=None, columns=None, index_base=0):
        """The same upload running BEHIND the caller (sicp_cloud_upload_start): (n,3) rows OR three contiguous columns.  Returns once
        the device arrays are sized; any later call naming the slot waits for it first (and raises its error).  The source arrays are
        kept alive here; the caller must not write to them before `upload_wait` / the next call on the slot."""
        if (xyz is None) == (columns is None):
            raise ValueError("xyz OR columns")
        if xyz is not None:
            src = [_f64(xyz) if isinstance(xyz, np.ndarray) else xyz]
            n = int(src[0].shape[0])
            if tuple(src[0].shape) != (n, 3):
                raise ValueError("cloud must have shape (n, 3)")
            args = (_ptr(src[0]), None, None, None)
        else:
            src = [_f64(np.asarray(v)) for v in columns]
            n = len(src[0])
            if len(src) != 3 or any(v.ndim != 1 or len(v) != n for v in src):
                raise ValueError("x, y, z must be vectors of the same length")
            args = (None, _ptr(src[0]), _ptr(src[1]), _ptr(src[2]))
        # the slot's previous sources stay referenced until the C call has joined the helper that may still be reading them
        prev = self._bg_src.get(slot)
        try:
            self._chk(self._L.sicp_cloud_upload_start(self._h, slot, *args, n, int(index_base)))
        finally:
            self._bg_src[slot] = src
            del prev

    def upload_wait(self, slot):
        try:
            self._chk(self._L.sicp_cloud_upload_wait(self._h, slot))
        finally:
            self._bg_src.pop(slot, None)

    def size(self, slot):
        n = C.c_int64()
        self._chk(self._L.sicp_cloud_size(self._h, slot, C.byref(n)))
        return n.value

    def transform(self, slot, H):
        self._chk(self._L.sicp_cloud_transform(self._h, slot, _ptr(_f64(H).reshape(16))))

    def download(self, slot):
        out = np.empty((self.size(slot), 3))
        self._chk(self._L.sicp_cloud_download(self._h, slot, _ptr(out)))
        return out

    def download_columns(self, slot):
        """The cloud as three contiguous float64 vectors (x, y, z)."""
        n = self.size(slot)
        cols = [np.empty(n) for _ in range(3)]
        self._chk(self._L.sicp_cloud_download_columns(self._h, slot, _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2])))
        return cols

    def download_both(self, slot):
        """((n, 3) array, [x, y, z] vectors) in ONE pass over the link (pinned, pipelined, transposed by host threads)."""
        n = self.size(slot)
        out = np.empty((n, 3))
        cols = [np.empty(n) for _ in range(3)]
        self._chk(self._L.sicp_cloud_download_both(self._h, slot, _ptr(out), _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2])))
        return out, cols

    def set_planarity(self, slot, planarity=None, rows=None, n_global=None):
        """The cloud's `planarity` column (corrpts.py:158-163 tests the movable cloud's too): a dense float32 vector
        by global point index, or (rows, values) pairs with NaN elsewhere; None = no such column."""
        self._set_columns(self._L.sicp_cloud_set_planarity, "planarity", 1, slot, planarity, rows, n_global)

    def set_normals(self, slot, normals=None, rows=None, n_global=None):
        """The cloud's normal columns (sicp_cloud_set_normals), like set_planarity: a dense (n, 3) float32 block by global point
        index, or (rows, normals) pairs with NaN elsewhere; None = no such columns."""
        normals_version()
        self._set_columns(self._L.sicp_cloud_set_normals, "normals", 3, slot, normals, rows, n_global)

    def _set_columns(self, entry, what, width, slot, values, rows, n_global):
        """set_planarity and set_normals: `width` float32 columns per point through `entry`."""
        if values is None:
            self._chk(entry(self._h, slot, None, None, 0, 0))
            return
        v = np.ascontiguousarray(values, dtype=np.float32)
        if width > 1:
            v = v.reshape(-1, width)
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        if r is not None and len(r) != len(v):
            raise ValueError(f"rows and {what} must have the same length")
        n = int(n_global if n_global is not None else (len(v) if r is None else self.size(slot)))
        dummy = np.zeros(width, np.float32)
        self._chk(entry(self._h, slot, _ptr(r), _ptr(v if len(v) else dummy), len(v), n))

    def normal_angle_set(self, cos_max=None, k=10):
        """The ctx setting sicp_icp_run / sicp_icp_iterate honour (sicp_normal_angle_set): reject correspondences whose normals
        have |cos| < cos_max; None = off."""
        normals_version()
        self._chk(self._L.sicp_normal_angle_set(self._h, 0.0 if cos_max is None else float(cos_max), int(k)))

    def corr_reject_normal_angle(self, cos_max, k=10, H=None, pc2_normals=None):
        """The operator (sicp_corr_reject_normal_angle) over the alive correspondences; pc2_normals: (Q, 3) float32 per
        correspondence, None = the movable slot's columns or normals estimated on the device.  Returns how many are still alive."""
        normals_version()
        Hc = None if H is None else _f64(H).reshape(16)
        nv = None
        if pc2_normals is not None:
            nv = np.ascontiguousarray(pc2_normals, dtype=np.float32)
            if nv.shape != (self._Q, 3):
                raise ValueError("pc2_normals must have one row per correspondence")
        n = C.c_int64()
        self._chk(self._L.sicp_corr_reject_normal_angle(self._h, float(cos_max), int(k), _ptr(Hc), _ptr(nv), C.byref(n)))
        return n.value

    def normal_angle_info(self):
        """Since icp_setup (sicp_normal_angle_info): normals estimated on demand, correspondences the verdict dropped in the last
        iteration, bytes of the cache, iterations whose miss list was empty."""
        normals_version()
        out = np.zeros(4, np.int64)
        self._chk(self._L.sicp_normal_angle_info(self._h, _ptr(out)))
        return {"normals_estimated": int(out[0]), "normal_angle_dropped": int(out[1]), "normal_cache_bytes": int(out[2]),
                "normal_miss_free_iterations": int(out[3])}

    def normal_cache(self):
        """The movable slot's cache of estimated normals (sicp_normal_cache_read): ((n, 3) float32, (n,) bool "is there")."""
        normals_version()
        n = self.size(MOV)
        nv, have = np.empty((n, 3), np.float32), np.empty(n, np.uint8)
        self._chk(self._L.sicp_normal_cache_read(self._h, _ptr(nv), _ptr(have)))
        return nv, have.astype(bool)

    # -- at most one point per voxel (contract (V)) --
    def voxel_select(self, slot, voxel_size, origin=None, rows=None, keep_ptr=None):
        """sicp_voxel_select: among the rows `rows` of the slot (None = all its points) the lowest-index point of every voxel of
        the lattice (cell voxel_size, origin None = zeros) is kept.  Returns the bool verdicts, one per candidate; with keep_ptr (a
        device address of that many bytes) they are left there and the number kept is returned instead."""
        voxel_version()
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        m = self.size(slot) if r is None else len(r)
        o = None if origin is None else _f64(origin).reshape(3)
        kept = C.c_int64()
        out = np.empty(max(m, 1), dtype=np.uint8) if keep_ptr is None else keep_ptr
        self._chk(self._L.sicp_voxel_select(self._h, slot, _ptr(r), m, float(voxel_size), _ptr(o), _ptr(out), C.byref(kept)))
        return out[:m].view(np.bool_) if keep_ptr is None else kept.value

    def voxel_select_masked(self, slot, mask_ptr, n, voxel_size, origin=None, keep_ptr=None):
        """sicp_voxel_select_masked: the candidates are the points whose byte of the device mask (n bytes at mask_ptr) is non-zero;
        the verdicts go to keep_ptr (device memory, n bytes; None = over the mask).  Returns how many were kept."""
        voxel_version()
        o = None if origin is None else _f64(origin).reshape(3)
        kept = C.c_int64()
        self._chk(self._L.sicp_voxel_select_masked(self._h, slot, C.c_void_p(int(mask_ptr)), int(n), float(voxel_size), _ptr(o),
                                                   C.c_void_p(int(mask_ptr if keep_ptr is None else keep_ptr)), C.byref(kept)))
        return kept.value

    # -- outlier removal (contract (O)) --
    def _outlier_shape(self, slot, rows, mask_ptr):
        """(rows as int64 or None, entries of every output) of an outlier call."""
        if rows is not None and mask_ptr is not None:
            raise ValueError("rows and mask_ptr are mutually exclusive")
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        if r is not None and len(r) == 0:
            raise ValueError("rows must not be empty (None: every point of the slot)")
        return r, (self.size(slot) if r is None else len(r))

    def outlier_statistical(self, slot, k, std_ratio, rows=None, mask_ptr=None, keep_ptr=None, mean_ptr=None):
        """sicp_outlier_statistical: the candidates -- the rows `rows` of the slot, the points whose byte of the device mask at
        mask_ptr is non-zero, or (both None) every point -- whose mean distance to their k nearest points of the slot is at most
        mean + std_ratio * std over the candidates are kept.  Returns (bool verdicts, (N,) float64 mean distances, OutlierStats),
        N = len(rows) or the slot's size; with keep_ptr (device memory, N bytes; may be mask_ptr) the verdicts are left there, the
        distances at mean_ptr if given (N doubles), and the OutlierStats alone is returned."""
        outlier_version()
        r, N = self._outlier_shape(slot, rows, mask_ptr)
        st = OutlierStats()
        host = keep_ptr is None
        keep, d = (np.empty(max(N, 1), np.uint8), np.empty(max(N, 1), np.float64)) if host else (keep_ptr, mean_ptr)
        self._chk(self._L.sicp_outlier_statistical(self._h, slot, _ptr(r), N, _ptr(mask_ptr), int(k), float(std_ratio), _ptr(keep),
                                                   _ptr(d), C.byref(st)))
        return (keep[:N].view(np.bool_), d[:N], st) if host else st

    def outlier_radius(self, slot, radius, min_points, rows=None, mask_ptr=None, keep_ptr=None, count_ptr=None):
        """sicp_outlier_radius: the candidates (as outlier_statistical takes them) with more than min_points points of the slot,
        themselves included, closer than radius (strict) are kept.  Returns (bool verdicts, (N,) uint32 counts capped at
        min_points + 1, number kept); with keep_ptr (device memory, N bytes) the verdicts are left there, the counts at count_ptr
        if given, and the number kept alone is returned."""
        outlier_version()
        r, N = self._outlier_shape(slot, rows, mask_ptr)
        kept = C.c_int64()
        host = keep_ptr is None
        keep, cnt = (np.empty(max(N, 1), np.uint8), np.empty(max(N, 1), np.uint32)) if host else (keep_ptr, count_ptr)
        self._chk(self._L.sicp_outlier_radius(self._h, slot, _ptr(r), N, _ptr(mask_ptr), float(radius), int(min_points), _ptr(keep),
                                              _ptr(cnt), C.byref(kept)))
        return (keep[:N].view(np.bool_), cnt[:N], kept.value) if host else kept.value

    def outlier_radius_cells(self, slot, radius):
        """sicp_outlier_radius_cells: (cells along x, y, z, their product) of the box a ball of this radius spans on the slot's
        grid; outlier_radius is accepted iff the product is at most OUTLIER_MAX_BOX_CELLS."""
        outlier_version()
        out = np.zeros(4, np.int64)
        self._chk(self._L.sicp_outlier_radius_cells(self._h, slot, float(radius), _ptr(out)))
        return tuple(int(v) for v in out)

    # -- FPFH descriptors (contract (F)) --
    def fpfh(self, slot, normals, k, radius=np.inf, viewpoint=None, fpfh_ptr=None, counts_ptr=None, want_counts=False):
        """sicp_fpfh: the 33-bin FPFH descriptor of every point of the slot from its k nearest points (the point itself
        included in k) within radius (strict; inf = none).  normals: (n, 3) float32, a numpy array or a device tensor; viewpoint:
        three floats, the normals are turned towards it first (None: used as they are).  Returns ((n, 33) float32, (n, 34) uint16
        counts or None, FpfhStats); with fpfh_ptr (device memory, n * 33 floats) the descriptors are left there, the counts at
        counts_ptr if given (n * 34 uint16), and the FpfhStats alone is returned."""
        fpfh_version()
        n = self.size(slot)
        if isinstance(normals, np.ndarray) or not hasattr(normals, "data_ptr"):
            normals = np.ascontiguousarray(normals, dtype=np.float32)
        if tuple(normals.shape) != (n, 3):
            raise ValueError("normals must have shape (n, 3), one row per point of the slot")
        vp = None if viewpoint is None else _f64(viewpoint).reshape(3)
        st = FpfhStats()
        host = fpfh_ptr is None
        out, cnt = fpfh_ptr, counts_ptr
        if host:
            out = np.empty((n, FPFH_BINS), np.float32)
            cnt = np.empty((n, FPFH_BINS + 1), np.uint16) if want_counts else None
        self._chk(self._L.sicp_fpfh(self._h, slot, _ptr(normals), int(k), float(radius), _ptr(vp), _ptr(out), _ptr(cnt), C.byref(st)))
        return (out, cnt, st) if host else st

    # -- ISS keypoints (contract (I)) --
    def keypoints(self, slot, k_s, salient_radius=np.inf, k_n=None, nms_radius=np.inf, gamma21=0.975, gamma32=0.975, min_neighbors=5,
                  keep_ptr=None, saliency_ptr=None, eig_ptr=None, want_saliency=False):
        """sicp_keypoints: the ISS keypoints of the slot -- the points whose k_s nearest points within salient_radius (strict; inf
        = none; the point itself included) have eigenvalues e2 < gamma21 * e1, e3 < gamma32 * e2, e3 > 0 and which no point of
        their k_n nearest within nms_radius beats in e3 (k_n None: k_s).  Returns (bool verdicts (n,), (n,) float64 saliency
        or None, (n, 3) float64 eigenvalues e1 e2 e3 or None, KeypointStats) -- the two arrays with want_saliency; with keep_ptr
        (device memory, n bytes) the verdicts are left there, the saliency at saliency_ptr (n doubles) and the eigenvalues at
        eig_ptr (3 n doubles) if given, and the KeypointStats alone is returned."""
        keypoints_version()
        n = self.size(slot)
        kn = int(k_s) if k_n is None else int(k_n)
        st = KeypointStats()
        args = (int(k_s), float(salient_radius), kn, float(nms_radius), float(gamma21), float(gamma32), int(min_neighbors))
        host = keep_ptr is None
        keep, sal, eig = keep_ptr, saliency_ptr, eig_ptr
        if host:
            keep = np.empty(max(n, 1), np.uint8)
            sal = np.empty(n, np.float64) if want_saliency else None
            eig = np.empty((n, 3), np.float64) if want_saliency else None
        self._chk(self._L.sicp_keypoints(self._h, slot, *args, _ptr(keep), _ptr(sal), _ptr(eig), C.byref(st)))
        return (keep[:n].view(np.bool_), sal, eig, st) if host else st

    # -- DBSCAN labels (contract (U)) --
    def cluster(self, slot, radius, min_points, labels_ptr=None, core_ptr=None):
        """sicp_cluster: the DBSCAN labels of the slot -- a point with at least min_points points of the slot, itself included,
        strictly within radius is core; clusters are the connected components of the core points, labelled 0, 1, ... in the order
        of their lowest core index; a point that is not core takes the smallest label among its core neighbours; -1: noise.
        Returns ((n,) int32 labels, (n,) bool core flags, ClusterStats); with labels_ptr (device memory, n int32) the labels are
        left there, the core bytes at core_ptr if given (n bytes), and the ClusterStats alone is returned."""
        cluster_version()
        n = self.size(slot)
        st = ClusterStats()
        host = labels_ptr is None
        labels, core = (np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.uint8)) if host else (labels_ptr, core_ptr)
        self._chk(self._L.sicp_cluster(self._h, slot, float(radius), int(min_points), _ptr(labels), _ptr(core), C.byref(st)))
        return (labels[:n], core[:n].view(np.bool_), st) if host else st

    # -- consistent normal orientation (contract (H)) --
    def orient(self, slot, normals, k, reference=None, away=False, normals_ptr=None, flipped_ptr=None, want_flipped=True):
        """sicp_orient: the normals of the slot's points, every component of the k-NN graph given one sign -- neighbouring normals
        agree along the minimum spanning forest under (larger |dot| first, then the smaller indices), the lowest index of a component
        keeps its sign; reference (three floats): a component is turned as a whole towards it (away: away from it) by the majority
        of its points.  normals: (n, 3) float32, a numpy array or a device tensor.  Returns ((n, 3) float32 normals, (n,) bool
        flipped or None, OrientStats); with normals_ptr (host or device memory, n * 3 floats; it may be the normals' own address)
        the result is left there, the flipped bytes at flipped_ptr if given (n bytes), and the OrientStats alone is returned."""
        orient_version()
        n = self.size(slot)
        if isinstance(normals, np.ndarray) or not hasattr(normals, "data_ptr"):
            normals = np.ascontiguousarray(normals, dtype=np.float32)
        if tuple(normals.shape) != (n, 3):
            raise ValueError("normals must have shape (n, 3), one row per point of the slot")
        ref = None if reference is None else _f64(reference).reshape(3)
        st = OrientStats()
        host = normals_ptr is None
        out, flipped = normals_ptr, flipped_ptr
        if host:
            out = np.empty((n, 3), np.float32)
            flipped = np.empty(max(n, 1), np.uint8) if want_flipped else None
        self._chk(self._L.sicp_orient(self._h, slot, _ptr(normals), int(k), _ptr(ref), 1 if away else 0, _ptr(out), _ptr(flipped),
                                      C.byref(st)))
        return (out, None if flipped is None else flipped[:n].view(np.bool_), st) if host else st

    # -- smooth regions (contract (J)) --
    def regions(self, slot, normals, k, cos_min, radius=float("inf"), oriented=False, seeds=None, min_size=1, labels_ptr=None):
        """sicp_regions: the smooth regions of the slot's points -- the connected components of the smooth points (a normal that
        is not void, seeds[i] != 0) under the edges of the k-NN graph strictly within radius whose normals agree, |dot| >= cos_min
        (oriented: dot >= cos_min); a point that is not smooth joins the region with the lowest root it has such an edge with;
        regions of fewer than min_size members are dropped, the others numbered in the order of their lowest index; -1: no
        region.  normals: (n, 3) float32, seeds: (n,) bytes or None -- numpy arrays or device tensors.  Returns ((n,) int32
        labels, RegionsStats); with labels_ptr (host or device memory, n int32) the labels are left there and the RegionsStats
        alone is returned."""
        regions_version()
        n = self.size(slot)
        if isinstance(normals, np.ndarray) or not hasattr(normals, "data_ptr"):
            normals = np.ascontiguousarray(normals, dtype=np.float32)
        if tuple(normals.shape) != (n, 3):
            raise ValueError("normals must have shape (n, 3), one row per point of the slot")
        if seeds is not None:
            if isinstance(seeds, np.ndarray) or not hasattr(seeds, "data_ptr"):
                seeds = np.ascontiguousarray(np.asarray(seeds) != 0).view(np.uint8)
            if tuple(seeds.shape) != (n,):
                raise ValueError("seeds must have shape (n,), one byte per point of the slot")
        st = RegionsStats()
        host = labels_ptr is None
        labels = np.empty(max(n, 1), np.int32) if host else labels_ptr
        self._chk(self._L.sicp_regions(self._h, slot, _ptr(normals), int(k), float(radius), float(cos_min), 1 if oriented else 0,
                                       _ptr(seeds), int(min_size), _ptr(labels), C.byref(st)))
        return (labels[:n], st) if host else st

    # -- moving-least-squares smoothing (contract (W)) --
    def denoise(self, slot, k, radius=float("inf"), bandwidth=float("inf"), strength=1.0, min_neighbors=3, points_ptr=None,
                normals_ptr=None, displacement_ptr=None, want_normals=False, want_displacement=False):
        """sicp_denoise: the slot's points, each projected onto the plane fitted to its k nearest points (the point itself
        included) strictly within radius (inf = none) -- weights (1 - d2 / bandwidth^2)^2 where positive, else 0 (inf: all 1) --,
        moved by strength (0 .. 1) times its signed distance g along the plane's normal; a point with fewer than min_neighbors
        such neighbours stays where it is.  Returns ((n, 3) float64 points, (n, 3) float32 normals or None, (n,) float64
        displacements g or None, DenoiseStats); with points_ptr (host or device memory, 3 n doubles) the points are left there,
        the normals at normals_ptr (3 n floats) and the displacements at displacement_ptr (n doubles) if given, and the
        DenoiseStats alone is returned."""
        denoise_version()
        n = self.size(slot)
        st = DenoiseStats()
        host = points_ptr is None
        pts, nrm, disp = points_ptr, normals_ptr, displacement_ptr
        if host:
            pts = np.empty((max(n, 1), 3), np.float64)
            nrm = np.empty((n, 3), np.float32) if want_normals else None
            disp = np.empty(n, np.float64) if want_displacement else None
        self._chk(self._L.sicp_denoise(self._h, slot, int(k), float(radius), float(bandwidth), float(strength), int(min_neighbors),
                                       _ptr(pts), _ptr(nrm), _ptr(disp), C.byref(st)))
        return (pts[:n], nrm, disp, st) if host else st

    # -- planes of a cloud (contracts (P) and (Q)) --
    def plane_triplets(self, X, triples, max_distance, mask=None, n=None, h=None, planes_ptr=None, inliers_ptr=None, want_planes=True):
        """sicp_plane_triplets: one plane per triple of rows of X (unit normal and d: contract (P)), scored by the candidate rows
        -- mask != 0; None: all -- strictly within max_distance of it.  Host form: an (n, 3) float64 array, an (n,) mask or None
        and (h, 3) int32 triples; returns ((h, 4) float64 planes or None, (h,) int32 inliers: -1 void, PlaneStats).  Pointer form:
        X, mask (or None) and triples are addresses (ints) of host or device memory, n and h given; the inliers are left at
        inliers_ptr (h int32), the planes at planes_ptr if given (h * 4 doubles), and the PlaneStats alone is returned."""
        plane_version()
        st = PlaneStats()
        host = inliers_ptr is None
        x, m, tri, planes, inl = X, mask, triples, planes_ptr, inliers_ptr
        if host:
            x, m = _cloud_rows(X, mask)
            tri = np.ascontiguousarray(triples, dtype=np.int32)
            if tri.ndim != 2 or tri.shape[1] != 3:
                raise ValueError("triples must be (h, 3)")
            n, h = x.shape[0], tri.shape[0]
            planes = np.empty((h, 4), np.float64) if want_planes else None
            inl = np.empty(h, np.int32)
        self._chk(self._L.sicp_plane_triplets(self._h, _ptr(x), int(n), _ptr(m), _ptr(tri), int(h), float(max_distance), _ptr(planes),
                                              _ptr(inl), C.byref(st)))
        return (planes, inl, st) if host else st

    def plane_refit(self, X, planes, max_distance, rounds, mask=None, n=None, b=None, planes_ptr=None, inliers_ptr=None, keep_ptr=None,
                    want_keep=False):
        """sicp_plane_refit: every plane refitted on its own inliers among the candidate rows of X in `rounds` rounds (contract
        (Q)); what leaves is the plane with the most inliers among the one given and every round's.  Host form: an (n, 3) float64
        array, an (n,) mask or None and (b, 4) float64 planes; returns ((b, 4) float64 planes, (b,) int32 inliers: -1 void, the
        (n,) bool inlier mask of the output plane -- want_keep, b == 1 -- or None, PlaneRefitStats).  Pointer form: X, mask (or
        None) and planes are addresses (ints) of host or device memory, n and b given; the planes are left at planes_ptr (b * 4
        doubles), the inliers at inliers_ptr (b int32), the mask's bytes at keep_ptr if given (n bytes), and the PlaneRefitStats
        alone is returned."""
        plane_version()
        st = PlaneRefitStats()
        host = inliers_ptr is None
        x, m, p, out, inl, keep = X, mask, planes, planes_ptr, inliers_ptr, keep_ptr
        if host:
            x, m = _cloud_rows(X, mask)
            p = _f64(planes)
            if p.ndim != 2 or p.shape[1] != 4:
                raise ValueError("planes must be (b, 4)")
            n, b = x.shape[0], p.shape[0]
            out, inl = np.empty((b, 4), np.float64), np.empty(b, np.int32)
            keep = np.empty(max(n, 1), np.uint8) if want_keep else None
        self._chk(self._L.sicp_plane_refit(self._h, _ptr(x), int(n), _ptr(m), _ptr(p), int(b), float(max_distance), int(rounds), _ptr(out),
                                           _ptr(inl), _ptr(keep), C.byref(st)))
        return (out, inl, None if keep is None else keep[:n].view(np.bool_), st) if host else st

    # -- farthest point sampling (contract (S)) --
    def farthest(self, X, count, start=-1, mask=None, n=None, idx_ptr=None, d2_ptr=None, want_d2=True):
        """sicp_farthest: `count` rows of X, one after the other, each the candidate row -- mask != 0 (None: all), coordinates
        finite -- farthest from those already taken (contract (S)); start: the first pick, -1 the lowest candidate.  Host form: an
        (n, 3) float64 array and an (n,) mask or None; returns ((count,) int64 picks, -1 from n_selected on, (count,) float64 squared
        distances -- +0.0 from n_selected on; None without want_d2 --, FarthestStats).  Pointer form: X and mask (or None) are
        addresses (ints) of host or device memory, n given; the picks are left at idx_ptr (count int64), the distances at d2_ptr
        if given (count doubles), and the FarthestStats alone is returned."""
        farthest_version()
        st = FarthestStats()
        host = idx_ptr is None
        x, m, idx, d2 = X, mask, idx_ptr, d2_ptr
        if host:
            x, m = _cloud_rows(X, mask)
            n = x.shape[0]
            idx = np.empty(max(int(count), 1), np.int64)
            d2 = np.empty(max(int(count), 1), np.float64) if want_d2 else None
        self._chk(self._L.sicp_farthest(self._h, _ptr(x), _ptr(m), int(n), int(count), int(start), _ptr(idx), _ptr(d2), C.byref(st)))
        return (idx, d2, st) if host else st

    # -- descriptor matching and RANSAC poses (contracts (M) and (R)) --
    def feature_match(self, query, target, nq=None, nt=None, dim=None, idx_ptr=None, d2_ptr=None, want_d2=True):
        """sicp_feature_match: for every row of query (nq, dim) the row of target (nt, dim) with the smallest (d2, row), d2 the
        float32 sum of squared differences in column order; -1 / +inf where no row has a finite d2.  Host form: float32 arrays;
        returns ((nq,) int32, (nq,) float32 or None, MatchStats).  Device form: query and target are device addresses (ints) of
        contiguous float32 rows, nq, nt, dim given; the indices are left at idx_ptr (nq int32), the distances at d2_ptr if
        given (nq float32), and the MatchStats alone is returned."""
        global_version()
        st = MatchStats()
        host = idx_ptr is None
        q, t, idx, d2 = query, target, idx_ptr, d2_ptr
        if host:
            q, t = np.ascontiguousarray(query, dtype=np.float32), np.ascontiguousarray(target, dtype=np.float32)
            if q.ndim != 2 or t.ndim != 2 or q.shape[1] != t.shape[1]:
                raise ValueError("query and target must be (nq, dim) and (nt, dim)")
            nq, nt, dim = q.shape[0], t.shape[0], q.shape[1]
            idx = np.empty(nq, np.int32)
            d2 = np.empty(nq, np.float32) if want_d2 else None
        self._chk(self._L.sicp_feature_match(self._h, _ptr(q), int(nq), _ptr(t), int(nt), int(dim), _ptr(idx), _ptr(d2), C.byref(st)))
        return (idx, d2, st) if host else st

    def ransac_triplets(self, src, dst, triples, max_distance, edge_ratio, m=None, h=None, poses_ptr=None, inliers_ptr=None,
                        want_poses=True):
        """sicp_ransac_triplets: one pose per triple of the matched rows src[c] <-> dst[c] (the minimal solver of contract (R),
        pruned by the edge-length check first), scored by its inliers within max_distance.  Host form: (m, 3) float64 arrays and
        (h, 3) int32 triples; returns ((h, 12) float64 poses -- R row-major, then t -- or None, (h,) int32 inliers: -1 void, -2
        pruned, RansacStats).  Device form: src, dst and triples are device addresses (ints), m and h given; the inliers are left
        at inliers_ptr (h int32), the poses at poses_ptr if given (h * 12 doubles), and the RansacStats alone is returned."""
        global_version()
        st = RansacStats()
        host = inliers_ptr is None
        s, d, tri, poses, inl = src, dst, triples, poses_ptr, inliers_ptr
        if host:
            s, d, ok = _matched_rows(src, dst)
            tri = np.ascontiguousarray(triples, dtype=np.int32)
            if not ok or tri.ndim != 2 or tri.shape[1] != 3:
                raise ValueError("src and dst must be (m, 3), triples (h, 3)")
            m, h = s.shape[0], tri.shape[0]
            poses = np.empty((h, 12), np.float64) if want_poses else None
            inl = np.empty(h, np.int32)
        self._chk(self._L.sicp_ransac_triplets(self._h, _ptr(s), _ptr(d), int(m), _ptr(tri), int(h), float(max_distance),
                                               float(edge_ratio), _ptr(poses), _ptr(inl), C.byref(st)))
        return (poses, inl, st) if host else st

    # -- least-squares poses of matched rows (contract (L)) --
    def pose_refit(self, src, dst, poses, max_distance, rounds, m=None, b=None, poses_ptr=None, inliers_ptr=None):
        """sicp_pose_refit: every pose refitted on its own inliers among the matched rows src[c] <-> dst[c] in `rounds` rounds
        (contract (L)); what leaves is the pose with the most inliers among the one given and every round's.  poses None: the
        plain least-squares fit of all finite rows (b = 1).  Host form: (m, 3) float64 arrays and (b, 12) float64 poses -- R
        row-major, then t --; returns ((b, 12) float64 poses, (b,) int32 inliers: -1 void, PosefitStats).  Pointer form: src, dst
        and poses (or None) are addresses (ints) of host or device memory, m and b given; the poses are left at poses_ptr
        (b * 12 doubles), the inliers at inliers_ptr (b int32), and the PosefitStats alone is returned."""
        posefit_version()
        st = PosefitStats()
        host = inliers_ptr is None
        s, d, p, out, inl = _pose_call_arrays(src, dst, poses) if host else (src, dst, poses, poses_ptr, inliers_ptr)
        if host:
            m, b = s.shape[0], len(inl)
        self._chk(self._L.sicp_pose_refit(self._h, _ptr(s), _ptr(d), int(m), _ptr(p), int(b), float(max_distance), int(rounds), _ptr(out),
                                          _ptr(inl), C.byref(st)))
        return (out, inl, st) if host else st

    # -- robust poses of matched rows (contract (G)) --
    def pose_robust(self, src, dst, poses, max_distance, rounds, divisor, start_scale=0.0, m=None, b=None, poses_ptr=None,
                    inliers_ptr=None, scales_ptr=None):
        """sicp_pose_robust: every pose refitted over all matched rows src[c] <-> dst[c] under Geman-McClure weights whose scale
        starts at start_scale (0: twice the largest squared residual under the start) and is divided by `divisor` after each of
        the `rounds` rounds, never below max_distance^2 (contract (G)); what leaves is the latest pose.  poses None: the start is
        the identity (b = 1).  Host form: (m, 3) float64 arrays and (b, 12) float64 poses -- R row-major, then t --; returns
        ((b, 12) float64 poses, (b,) int32 inliers: -1 void, (b,) float64 final scales, RobustStats).  Pointer form: src, dst and
        poses (or None) are addresses (ints) of host or device memory, m and b given; the poses are left at poses_ptr (b * 12
        doubles), the inliers at inliers_ptr (b int32), the scales at scales_ptr (b doubles), and the RobustStats alone is
        returned."""
        robust_version()
        st = RobustStats()
        host = inliers_ptr is None
        s, d, p, out, inl = _pose_call_arrays(src, dst, poses) if host else (src, dst, poses, poses_ptr, inliers_ptr)
        scales = scales_ptr
        if host:
            m, b = s.shape[0], len(inl)
            scales = np.empty(b, np.float64)
        self._chk(self._L.sicp_pose_robust(self._h, _ptr(s), _ptr(d), int(m), _ptr(p), int(b), float(max_distance), int(rounds),
                                           float(divisor), float(start_scale), _ptr(out), _ptr(inl), _ptr(scales), C.byref(st)))
        return (out, inl, scales, st) if host else st

    # -- matches pruned by pairwise length consistency (contract (C)) --
    def match_consistency(self, src, dst, tolerance, min_length, m=None, degree_ptr=None, core_ptr=None):
        """sicp_match_consistency: rows i and j of the matched rows src[c] <-> dst[c] are compatible when their distance in src and
        their distance in dst differ by at most `tolerance` and neither is below `min_length` (contract (C)); every row's degree
        and core number in that graph.  Host form: (m, 3) float64 arrays; returns ((m,) int32 degrees, (m,) int32 core numbers,
        ConsistencyStats).  Pointer form: src and dst are addresses (ints) of host or device memory, m given; the degrees are left
        at degree_ptr and the core numbers at core_ptr (m int32 each), and the ConsistencyStats alone is returned."""
        consistency_version()
        st = ConsistencyStats()
        host = degree_ptr is None
        s, d, degree, core = src, dst, degree_ptr, core_ptr
        if host:
            s, d, ok = _matched_rows(src, dst)
            if not ok:
                raise ValueError("src and dst must be (m, 3)")
            m = s.shape[0]
            degree, core = np.empty(m, np.int32), np.empty(m, np.int32)
        self._chk(self._L.sicp_match_consistency(self._h, _ptr(s), _ptr(d), int(m), float(tolerance), float(min_length), _ptr(degree),
                                                 _ptr(core), C.byref(st)))
        return (degree, core, st) if host else st

    # -- how good a registration is (contract (E)) --
    def evaluate(self, query_slot, search_slot, H=None, max_distance=np.inf, rows=None):
        """sicp_evaluate: every point of query_slot (rows: these rows of it, in this order -- an int64 array, or a device tensor)
        searches its nearest point among H * search_slot (H None = identity) within max_distance (strict).  Returns the
        EvalRecord: the number of queries and of inliers, and the ten tree sums of contract (E) over the inliers."""
        eval_version()
        if rows is not None and not hasattr(rows, "data_ptr"):
            rows = np.ascontiguousarray(rows, dtype=np.int64)
        Q = 0 if rows is None else int(rows.shape[0])
        if rows is not None and Q == 0:
            raise ValueError("rows must not be empty (None: every point of the slot)")
        Hm = None if H is None else _f64(H).reshape(16)
        rec = EvalRecord()
        self._chk(self._L.sicp_evaluate(self._h, query_slot, search_slot, _ptr(rows), Q, _ptr(Hm), float(max_distance), C.byref(rec)))
        return rec

    # -- nearest neighbours --
    def knn(self, slot, q_xyz, k=1, H=None, max_dist=np.inf):
        q = _f64(q_xyz)
        Q = len(q)
        idx = np.empty((Q, k), np.int64)
        d2 = np.empty((Q, k), np.float64)
        Hc = None if H is None else _f64(H).reshape(16)
        self._chk(self._L.sicp_knn(self._h, slot, _ptr(q), Q, int(k), _ptr(Hc), float(max_dist), _ptr(idx), _ptr(d2)))
        return idx, d2

    def select_in_range(self, query_slot, search_slot, sel=None, H=None, max_range=np.inf):
        """bool mask over `sel` (all points of query_slot when None): nearest neighbour in search_slot (under H)
        closer than max_range -- both clouds already resident (sicp_select_in_range)."""
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.int64)
        Q = self.size(query_slot) if sel is None else len(sel)
        out = np.empty(Q, dtype=np.uint8)
        Hp = None if H is None else _f64(H).reshape(16)
        self._chk(self._L.sicp_select_in_range(self._h, query_slot, search_slot, _ptr(sel), Q, _ptr(Hp), float(max_range),
                                               _ptr(out)))
        return out.view(np.bool_)

    def estimate_normals(self, slot, sel_idx, k, want_nn=False):
        sel = np.ascontiguousarray(sel_idx, dtype=np.int64)
        Q = len(sel)
        nv = np.empty((Q, 3), np.float32)
        pl = np.empty(Q, np.float32)
        nn = np.empty((Q, k), np.int64) if want_nn else None
        self._chk(self._L.sicp_estimate_normals(self._h, slot, _ptr(sel), Q, int(k), _ptr(nv), _ptr(pl), _ptr(nn)))
        return (nv, pl, nn) if want_nn else (nv, pl)

    # -- ICP iteration --
    def icp_setup(self, sel_idx, normals, planarity):
        sel = np.ascontiguousarray(sel_idx, dtype=np.int64)
        nv = np.ascontiguousarray(normals, dtype=np.float32)
        pl = np.ascontiguousarray(planarity, dtype=np.float32)
        if nv.shape != (len(sel), 3) or pl.shape != (len(sel),):
            raise ValueError("normals must be (Q,3) and planarity (Q,)")
        self._chk(self._L.sicp_icp_setup(self._h, _ptr(sel), len(sel), _ptr(nv), _ptr(pl)))
        self._Q = len(sel)

    def icp_iterate(self, x, obs, obs_weight, min_planarity=0.3, distance_weight=1.0, max_lm_steps=0):
        """One iteration; distance_weight None = automatic (simpleicp.py:233-234).  Returns IterResult;
        raises BackendError(code=ERR_TOO_FEW) when fewer than 6 correspondences survive."""
        P = self._params(x, obs, obs_weight, min_planarity, distance_weight, max_lm_steps)
        R = IterResult()
        rc = self._L.sicp_icp_iterate(self._h, C.byref(P), C.byref(R))
        if rc != OK:
            err = BackendError(self._L.sicp_last_error().decode(), rc)
            err.result = R
            raise err
        return R

    @staticmethod
    def _params(x, obs, obs_weight, min_planarity=0.3, distance_weight=1.0, max_lm_steps=0):
        return IterParams((C.c_double * 6)(*x), (C.c_double * 6)(*obs), (C.c_double * 6)(*obs_weight),
                          min_planarity, -1.0 if distance_weight is None else distance_weight, int(max_lm_steps))

    def icp_run(self, x, obs, obs_weight, min_planarity=0.3, distance_weight=1.0, max_iterations=100, min_change=1.0,
                max_lm_steps=0):
        """The whole loop in one ABI call (sicp_icp_run).  Returns the list of per-iteration IterResult;
        raises BackendError (with `.results`) like icp_iterate when an iteration fails."""
        P = self._params(x, obs, obs_weight, min_planarity, distance_weight, max_lm_steps)
        n = int(max_iterations)
        res = (IterResult * max(n, 1))()
        done = C.c_int64()
        rc = self._L.sicp_icp_run(self._h, C.byref(P), n, float(min_change), res, C.byref(done))
        out = [res[i] for i in range(done.value)]
        if rc != OK:
            err = BackendError(self._L.sicp_last_error().decode(), rc)
            err.results = out
            raise err
        return out

    def icp_run_batch(self, members):
        """sicp_icp_run_batch with this context as the first member: see the module-level icp_run_batch."""
        if not members or members[0][0] is not self:
            raise ValueError("the batch's first member must be this context")
        return icp_run_batch(members)

    def icp_state(self, pc2_idx=True, dist=True, keep=True, residual=True):
        Q = self._Q
        a = np.empty(Q, np.int64) if pc2_idx else None
        b = np.empty(Q, np.float64) if dist else None
        c = np.empty(Q, np.uint8) if keep else None
        d = np.empty(Q, np.float64) if residual else None
        self._chk(self._L.sicp_icp_get_state(self._h, _ptr(a), _ptr(b), _ptr(c), _ptr(d)))
        return a, b, (None if c is None else c.astype(bool)), d

    def icp_uncertainties(self):
        s = np.empty(6)
        self._chk(self._L.sicp_icp_uncertainties(self._h, _ptr(s)))
        return s

    def icp_normal_equations(self, x):
        out = np.empty(30)
        self._chk(self._L.sicp_icp_normal_equations(self._h, _ptr(_f64(x)), _ptr(out)))
        return out

    # -- the iteration's operators one by one (CorrPts / SimpleICPOptimization, corrpts.py / optimization.py) --
    def corr_match(self, H=None):
        """CorrPts.match: (pc2_idx (Q) int64, point-to-plane distances (Q)) of the points declared by icp_setup in the
        movable slot under H (None = identity); every correspondence is alive afterwards."""
        Q = self._Q
        idx, dist = np.empty(Q, np.int64), np.empty(Q, np.float64)
        Hc = None if H is None else _f64(H).reshape(16)
        self._chk(self._L.sicp_corr_match(self._h, _ptr(Hc), _ptr(idx), _ptr(dist)))
        return idx, dist

    def corr_reject_planarity(self, min_planarity, pc1_planarity=None, pc2_planarity=None):
        """CorrPts.reject_wrt_planarity; the columns per correspondence ((Q) float32, None = the cloud has none).
        Returns the number of correspondences still alive."""
        def col(v):
            if v is None:
                return None
            v = np.ascontiguousarray(v, dtype=np.float32)
            if v.shape != (self._Q,):
                raise ValueError("planarity columns must have one value per correspondence")
            return v
        p1, p2 = col(pc1_planarity), col(pc2_planarity)
        n = C.c_int64()
        self._chk(self._L.sicp_corr_reject_planarity(self._h, float(min_planarity), _ptr(p1), _ptr(p2), C.byref(n)))
        return n.value

    def corr_reject_distances(self):
        """CorrPts.reject_wrt_point_to_plane_distances over the alive correspondences: (median, mad, n_alive)."""
        med, mad, n = C.c_double(), C.c_double(), C.c_int64()
        self._chk(self._L.sicp_corr_reject_distances(self._h, C.byref(med), C.byref(mad), C.byref(n)))
        return med.value, mad.value, n.value

    def estimate_parameters(self, x, obs, obs_weight, distance_weight=1.0, pc2_xyz=None, max_lm_steps=0):
        """SimpleICPOptimization.estimate_parameters over the alive correspondences, from x; pc2_xyz: (Q,3) current
        coordinates of the matched movable points (None = as matched).  Returns IterResult."""
        P = self._params(x, obs, obs_weight, 0.0, distance_weight, max_lm_steps)
        R = IterResult()
        p2 = None
        if pc2_xyz is not None:
            p2 = _f64(pc2_xyz)
            if p2.shape != (self._Q, 3):
                raise ValueError("pc2_xyz must be (Q, 3)")
        rc = self._L.sicp_estimate_parameters(self._h, C.byref(P), _ptr(p2), C.byref(R))
        if rc != OK:
            err = BackendError(self._L.sicp_last_error().decode(), rc)
            err.result = R
            raise err
        return R

    def stream_ptr(self):
        """Raw hipStream_t of the context (for torch.cuda.ExternalStream)."""
        p = C.c_void_p()
        self._chk(self._L.sicp_ctx_stream(self._h, C.byref(p)))
        return p.value or 0

    # -- multi-GPU exchange hook --
    def set_exchange(self, fn, rank, world, gn_shard=False):
        """fn(what, a_ptr, b_ptr, c_ptr, count) -> 0 on success; pointers are device addresses."""
        if fn is None:
            self._cb = EXCHANGE_FN(0)
        else:
            def tramp(_user, what, a, b, c, count):
                try:
                    return int(fn(what, a, b, c, count) or 0)
                except Exception:  # noqa: BLE001
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cb = EXCHANGE_FN(tramp)
        self._chk(self._L.sicp_set_exchange(self._h, self._cb, None, int(rank), int(world), int(bool(gn_shard))))

    # -- the library's own RCCL communicator (no host callback) --
    @staticmethod
    def comm_unique_id():
        """128-byte ncclUniqueId (rank 0 creates it, every rank passes the same bytes to comm_init)."""
        buf = C.create_string_buffer(128)
        L = load()
        _chk(L, L.sicp_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, rank, world, gn_shard=False):
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        self._cb = None
        self._chk(self._L.sicp_comm_init(self._h, C.c_char_p(bytes(unique_id)), int(rank), int(world), int(bool(gn_shard))))

    def comm_destroy(self):
        self._comm_key = self._comm_group = None          # (dist.attach's note of a parked communicator: there is none any more)
        self._chk(self._L.sicp_comm_destroy(self._h))

    def comm_activate(self, on=True, gn_shard=False):
        """Use (on) or park (off) the communicator the context already owns."""
        self._chk(self._L.sicp_comm_activate(self._h, int(bool(on)), int(bool(gn_shard))))

    def comm_info(self):
        """What exchange is in force: backend none / callback / rccl, ranks and rank (for rccl as RCCL counts them)."""
        out = (C.c_int * 6)()
        self._chk(self._L.sicp_comm_info(self._h, C.byref(out)))
        return {"backend": ("none", "callback", "rccl")[out[0]], "nranks": out[1], "rank": out[2],
                "partition": "queries" if out[3] == PART_QUERIES else "cloud", "gn_shard": bool(out[4]),
                "communicator": bool(out[5])}

    def device_memory(self):
        """(free, total) bytes of the context's device."""
        f, t = C.c_int64(), C.c_int64()
        self._chk(self._L.sicp_device_memory(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def set_partition(self, mode):
        """PART_CLOUD: ranks hold index ranges of the searched cloud; PART_QUERIES: ranks hold the whole cloud and
        match a slice of the queries each."""
        self._chk(self._L.sicp_set_partition(self._h, int(mode)))

    def lexmin_gathered(self, gathered):
        """gathered: (world, Q, 5) float64 records (d2, idx bits, x, y, z) -> (d2, idx, xyz)."""
        g = _f64(gathered)
        world, Q, five = g.shape
        assert five == 5
        d2, idx, xyz = np.empty(Q), np.empty(Q, np.int64), np.empty((Q, 3))
        self._chk(self._L.sicp_lexmin_gathered(self._h, _ptr(g), world, Q, _ptr(d2), _ptr(idx), _ptr(xyz)))
        return d2, idx, xyz

    # -- timing --
    def timing_enable(self, on=True, count_work=False):
        """Kernel timing with HIP events on the library's stream; count_work also makes the grid search tally the
        candidates and rows it touches (slower: a separate pass)."""
        self._chk(self._L.sicp_timing_enable(self._h, 2 if (on and count_work) else int(bool(on))))

    def timing_reset(self):
        self._chk(self._L.sicp_timing_reset(self._h))

    def last_match_kernel(self):
        k = C.c_int()
        self._chk(self._L.sicp_last_match_kernel(self._h, C.byref(k)))
        return MATCH_KERNELS[k.value]

    def match_work(self):
        """Work counters of the grid search since timing_reset (kept while timing is enabled)."""
        out = np.zeros(3, np.uint64)
        self._chk(self._L.sicp_match_work(self._h, _ptr(out)))
        d = C.c_uint64(0)
        self._chk(self._L.sicp_match_deferred(self._h, C.byref(d)))
        return {"candidates": int(out[0]), "rows": int(out[1]), "launches": int(out[2]), "deferred": int(d.value)}

    def chain_info(self):
        """Matches launched early (the tail -> match hand-over, include/simpleicp_hip_chain.h) in the last chained run / since the
        context was created; 0 = the single-stream chain."""
        out = np.zeros(2, dtype=np.int64)
        self._chk(self._L.sicp_chain_info(self._h, _ptr(out)))
        return {"last_run": int(out[0]), "total": int(out[1])}

    def tail_cycles(self):
        """k_icp_tail's own clock over its phases in the last iteration it ran (shader cycles)."""
        out = np.zeros(5)
        self._chk(self._L.sicp_tail_cycles(self._h, _ptr(out)))
        return dict(zip(("load", "select", "keep", "lm", "final"), (float(v) for v in out)))

    def tail_selection(self):
        """How the single-workgroup tail found median / MAD in its last iteration (histogram rounds; 0 = from the window around the
        previous iteration's value) and in how many iterations since icp_setup both came from their windows."""
        out = np.zeros(3, np.int64)
        self._chk(self._L.sicp_tail_selection(self._h, _ptr(out)))
        return {"median_rounds": int(out[0]), "mad_rounds": int(out[1]), "window_iterations": int(out[2])}

    def exchange_info(self):
        """What the chained iterations' exchanges did since icp_setup: form of the last one, how many ran."""
        out = np.zeros(4, np.int64)
        self._chk(self._L.sicp_exchange_info(self._h, _ptr(out)))
        return {"form": ("none", "records_allgather", "key_allreduces", "query_slices")[int(out[0])], "count": int(out[1]),
                "keys_min_q": int(out[2]), "callback_serves_u64": bool(out[3])}

    def knn_work(self):
        """Work counters of the one-sweep k-NN (normals) since timing_reset (kept while timing_enable(2) is in force)."""
        out = np.zeros(4, np.uint64)
        self._chk(self._L.sicp_knn_work(self._h, _ptr(out)))
        return {"candidates": int(out[0]), "sweeps": int(out[1]), "slow_queries": int(out[2]), "in_ball": int(out[3])}

    def timing(self):
        out = {}
        for k, name in KERNEL_NAMES.items():
            ms, n = C.c_double(), C.c_int64()
            self._chk(self._L.sicp_timing_get(self._h, k, C.byref(ms), C.byref(n)))
            out[name] = {"ms": ms.value, "launches": n.value}
        return out
