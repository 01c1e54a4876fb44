"""ctypes binding of the HIP library ``liblidarslam.so`` (C ABI: include/lidarslam.h).

The library is built in-tree (``python -m lidar_slam_amd.build`` or
``__graft_entry__.build()``).  There is NO CPU fallback: if the shared object
is missing or cannot be loaded, every entry point raises ``HIPLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LSLAM_LIB") or os.path.join(_HERE, "liblidarslam.so")  # override: experiments

# ---- constants mirrored from include/lidarslam.h ----
ABI_VERSION = 6  # include/lidarslam.h LSLAM_ABI_VERSION (struct layouts below)
LSLAM_OK = 0
LSLAM_ERR_ARG = -1
LSLAM_ERR_HIP = -2
LSLAM_ERR_NOMEM = -3
LSLAM_ERR_CAPACITY = -4
LSLAM_ERR_UNSUPPORTED = -5

VALID, N_TOO_SMALL, NO_INLIERS, EST_FAIL = 1, 2, 4, 8
EARLY_STOP, VERTICAL, NEW_LANDMARK, MATCHED = 16, 32, 64, 128
CAPACITY, CHUNK_BOUND = 256, 512

HYP_MT19937, HYP_PHILOX, HYP_EXPLICIT = 0, 1, 2
UKF_PREDICT, UKF_UPDATE, UKF_LMK_FROM_RANSAC, UKF_MAP, UKF_SIGMAS_IN = 1, 2, 4, 8, 16
K_POLAR, K_HYP, K_PIPELINE, K_LANDMARK, K_UKF, K_RNG, K_CONSENSUS = 0, 1, 2, 3, 4, 5, 6
K_EXPRESS, K_EXPRESS_SCATTER, K_MATCH, K_GRID, K_MAPMATCH, K_MAPFUSE, K_RELOC = 7, 8, 9, 10, 11, 12, 13
K_RAYCAST, K_RECENTRE = 14, 15
MATCH_EMPTY, MATCH_EDGE = 1, 2
GRID_BAD_POSE, GRID_CLIPPED = 1, 2
MAPMATCH_EMPTY, MAPMATCH_EDGE, MAPMATCH_BAD_POSE, MAPMATCH_WEAK = 1, 2, 4, 8
MAPFUSE_OUTLIER, MAPFUSE_BAD_COV = 16, 32
RELOC_LOST, RELOC_AMBIGUOUS = 1, 2
RAYCAST_BAD_POSE = 1
RAYCAST_INVALID, RAYCAST_MATCH, RAYCAST_NOVEL, RAYCAST_THROUGH, RAYCAST_UNMAPPED = 0, 1, 2, 3, 4  # cls & 15
RAYCAST_KIND_NONE, RAYCAST_KIND_UNKNOWN, RAYCAST_KIND_OCC = 0, 1, 2  # cls >> 4
RECENTRE_BAD_POSE, RECENTRE_MOVED, RECENTRE_CLEARED = 1, 2, 4
PAGE_LOST = 1
DIST_OCC, DIST_NOT_FREE = 0, 1  # lslam_dist_params.mode
DIST_EMPTY = 1
FIELD_BAD_POSE = 1
(FIELDALIGN_BAD_POSE, FIELDALIGN_CONVERGED, FIELDALIGN_SINGULAR, FIELDALIGN_FEW, FIELDALIGN_DIVERGED,
 FIELDALIGN_WEAK) = 1, 2, 4, 8, 16, 32
FIELDFUSE_OUTLIER, FIELDFUSE_BAD_COV = 64, 128
MERGE_ADD, MERGE_FILL = 0, 1  # lslam_gridmerge_params.mode
MERGE_MERGED, MERGE_WEAK, MERGE_CONFLICT, MERGE_SKIPPED, MERGE_BAD_XFORM = 1, 2, 4, 8, 16
GRIDPOINTS_BAD_ANCHOR, GRIDPOINTS_EMPTY, GRIDPOINTS_DECIMATED = 1, 2, 4
GRIDPOINTS_BANDS = 256  # LSLAM_GRIDPOINTS_BANDS: the second dimension of lslam_gridpoints_batch.band_counts
POSEGRAPH_EMPTY, POSEGRAPH_BAD_GRAPH, POSEGRAPH_CONVERGED, POSEGRAPH_SINGULAR, POSEGRAPH_DIVERGED = 1, 2, 4, 8, 16
POSEGATE_UNJUDGED, POSEGATE_ACCEPTED, POSEGATE_OUTLIER, POSEGATE_BAD_EDGE, POSEGATE_BAD_INFO = 0, 1, 2, 4, 8
POSEGATE_APPENDED, POSEGATE_NO_ROOM = 16, 32  # beside POSEGATE_ACCEPTED


class HIPLibraryError(RuntimeError):
    """The HIP library is missing, failed to load, or returned an error."""


class ChunkModel(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("ox", "oy", "ux", "uy", "a", "b", "tip_x", "tip_y",
                                          "proj_a", "proj_b")] + \
               [(n, C.c_int32) for n in ("n_inliers", "best_trial", "n_draws", "flags",
                                         "match_index", "landmark_id", "n_points", "reserved")]


class LandmarkRec(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("a", "b", "pos_x", "pos_y", "end_x", "end_y")] + \
               [("id", C.c_int32), ("life", C.c_int32)]


class RansacParams(C.Structure):
    _fields_ = [("residual_threshold", C.c_double), ("max_trials", C.c_int32), ("min_samples", C.c_int32),
                ("hyp_source", C.c_int32), ("life", C.c_int32), ("tol_a", C.c_double), ("tol_b", C.c_double),
                ("tol_dist", C.c_double), ("philox_seed", C.c_uint64)]


class UkfParams(C.Structure):
    _fields_ = [("n_landmarks", C.c_int32), ("flags", C.c_int32), ("dt", C.c_double),
                ("wheel_radius", C.c_double), ("wheel_base", C.c_double), ("alpha", C.c_double),
                ("beta", C.c_double), ("kappa", C.c_double), ("Q", C.c_double * 9)]


_VP = C.c_void_p


class ScanBatch(C.Structure):
    _fields_ = [("n_scans", C.c_int32), ("n_chunks", C.c_int32), ("n_points", C.c_int64),
                ("max_chunk_points", C.c_int32), ("max_scan_chunks", C.c_int32), ("lmk_capacity", C.c_int32),
                ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("xy", "scan_chunk_off", "chunk_pt_off", "seeds", "mt_state_in", "mt_state_out",
                                   "hyp", "id_base", "landmarks", "lmk_count", "lmk_walk", "inlier_mask", "models", "y_proj",
                                   "draws_out", "trial_cnt_out", "ukf_x", "ukf_P", "ukf_u", "ukf_z", "ukf_lmk",
                                   "ukf_R_diag", "theta_deg", "dist_mm", "ukf_sigmas")]


class ExpressMeasures(C.Structure):
    _fields_ = [(n, _VP) for n in ("angle_deg", "dist_mm", "new_scan", "valid", "xy", "pkt_valid")]


class ExpressRevs(C.Structure):
    _fields_ = [(n, _VP) for n in ("xy", "scan_chunk_off", "chunk_pt_off", "counts")] + \
               [("cap_points", C.c_int64), ("cap_scans", C.c_int32), ("cap_chunks", C.c_int32)]


class MatchParams(C.Structure):
    _fields_ = [("cell", C.c_double), ("theta_step", C.c_double), ("grid_w", C.c_int32), ("smear", C.c_int32),
                ("k_trans", C.c_int32), ("k_theta", C.c_int32)]


class MatchBatch(C.Structure):
    _fields_ = [("n_scans", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("ref_xy", "ref_off", "cur_xy", "cur_off", "rot", "delta", "best", "n_valid",
                                   "flags", "scores", "ukf_u")]


class GridParams(C.Structure):
    _fields_ = [("cell", C.c_double), ("max_range", C.c_double)] + \
               [(n, C.c_int32) for n in ("grid_w", "l_hit", "l_miss", "l_min", "l_max", "reserved")]


class GridBatch(C.Structure):
    _fields_ = [("n_robots", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("xy", "pt_off", "pose", "origin", "logodds", "rot", "n_used", "flags")]


class MapMatchParams(C.Structure):
    _fields_ = [("theta_step", C.c_double)] + \
               [(n, C.c_int32) for n in ("win_w", "smear", "k_trans", "k_theta", "occ_min", "min_permille")]


class MapMatchBatch(C.Structure):
    _fields_ = [("n_robots", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("xy", "pt_off", "pose", "origin", "logodds", "rot", "pose_out", "delta", "best",
                                   "n_valid", "rot0", "flags", "scores")]


class MapFuseParams(C.Structure):
    _fields_ = [("r_scale", C.c_double), ("nis_max", C.c_double), ("cut_permille", C.c_int32), ("reserved", C.c_int32)]


class MapFuseBatch(C.Structure):
    _fields_ = [("m", MapMatchBatch)] + [(n, _VP) for n in ("P", "P_out", "z", "Rm", "nis", "moments")]


class RelocParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("head_step", "dup_mm", "dup_rad", "reset_sigma_xy", "reset_sigma_theta")] + \
               [(n, C.c_int32) for n in ("n_head", "factor", "n_cand", "ambig_permille")]


class RelocBatch(C.Structure):
    _fields_ = [("n_robots", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("xy", "pt_off", "origin", "logodds", "rot", "head_rot", "n_occ", "n_used", "cand",
                                   "cand_pose", "fine_pose", "fine_delta", "fine_best", "fine_nvalid", "fine_rot0",
                                   "fine_flags", "result", "flags", "pose_out", "P_out", "coarse_scores")]


class RelocPriorParams(C.Structure):
    _fields_ = [("half_xy", C.c_double), ("half_theta", C.c_double), ("clear_min2", C.c_int32), ("reserved", C.c_int32)]


class RelocPriorBatch(C.Structure):
    _fields_ = [("r", RelocBatch)] + [(n, _VP) for n in ("clear_d2", "win_pose", "n_admit", "fine_clear2")]


class RaycastParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("occ_min", "free_max", "tol", "reserved")]


class RaycastBatch(C.Structure):
    _fields_ = [("n_robots", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("xy", "pt_off", "pose", "origin", "logodds", "cls", "stop", "counts", "rot", "flags")]


class RecentreParams(C.Structure):
    _fields_ = [("margin", C.c_int32), ("quantum", C.c_int32), ("reserved", C.c_int32 * 2)]


class RecentreBatch(C.Structure):
    _fields_ = [("n_robots", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("pose", "origin", "logodds", "shift", "flags")]


class PageParams(C.Structure):
    _fields_ = [("canvas_w", C.c_int32), ("reserved", C.c_int32 * 3)]


class PageBatch(C.Structure):
    _fields_ = [("n_robots", C.c_int32), ("reserved", C.c_int32)] + [(n, _VP) for n in ("canvas", "win", "moved", "flags")]


class DistParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("mode", "occ_min", "free_max", "d_max")]


class DistBatch(C.Structure):
    _fields_ = [("n_robots", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("logodds", "d2", "n_src", "flags")]


class FieldScoreParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("trunc2", "near2", "off2", "reserved")]


class FieldScoreBatch(C.Structure):
    _fields_ = [("n_robots", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("xy", "pt_off", "pose", "origin", "d2", "rot", "stats", "clear2", "flags")]


class FieldAlignParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("trunc", "damp_t", "damp_r", "eps_t", "eps_r", "max_shift", "max_turn")] + \
               [(n, C.c_int32) for n in ("n_iter", "min_points", "min_permille", "reserved")]


class FieldAlignBatch(C.Structure):
    _fields_ = [("n_robots", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("xy", "pt_off", "pose", "origin", "d2", "pose_out", "trace", "normal", "n_used",
                                   "iters", "flags")]


class FieldFuseParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("sigma_min", "r_scale", "floor_t", "floor_r", "nis_max")] + [("reserved", C.c_int64)]


class FieldFuseBatch(C.Structure):
    _fields_ = [("a", FieldAlignBatch)] + [(n, _VP) for n in ("P", "P_out", "z", "info", "info_f", "s2", "nis")]


class GridMergeParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("src_w", "n_src", "occ_min", "mode", "dry_run", "min_support",
                                         "max_contra_permille", "reserved")]


class GridMergeBatch(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("src", "src_origin", "src_index", "dst", "dst_origin", "xform", "stats", "flags")]


class GridPointsParams(C.Structure):
    _fields_ = [("radius", C.c_double), ("occ_min", C.c_int32), ("cap", C.c_int32)]


class GridPointsBatch(C.Structure):
    _fields_ = [("n_robots", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("logodds", "origin", "anchor", "xy", "pt_off", "counts", "flags", "band_counts")]


class PoseGraphParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("damp_t", "damp_r", "eps_t", "eps_r")] + \
               [(n, C.c_int32) for n in ("max_nodes", "max_edges", "n_iter", "reserved")]


class PoseGraphBatch(C.Structure):
    _fields_ = [("n_graphs", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("n_nodes", "n_edges", "pose", "edge_ij", "edge_z", "edge_info", "pose_out", "trace", "chi2",
                                   "edge_chi2", "iters", "flags")]


class PoseGateParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("damp_t", "damp_r", "nis_max")] + \
               [(n, C.c_int32) for n in ("max_nodes", "max_edges", "max_cand", "append")]


class PoseGateBatch(C.Structure):
    _fields_ = [("n_graphs", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, _VP) for n in ("n_nodes", "n_edges", "pose", "edge_ij", "edge_z", "edge_info", "n_cand", "cand_ij", "cand_z",
                                   "cand_info", "trace", "chi2", "cand_nis", "cand_err", "cand_cov", "cand_flags", "flags")]


assert C.sizeof(ChunkModel) == 112
assert C.sizeof(LandmarkRec) == 56

EXPORTS = [
    "lslam_version", "lslam_status_string", "lslam_last_error", "lslam_device_count", "lslam_ctx_create",
    "lslam_ctx_destroy", "lslam_sync", "lslam_malloc", "lslam_free", "lslam_host_alloc", "lslam_host_free",
    "lslam_h2d", "lslam_d2h", "lslam_d2d", "lslam_memset", "lslam_host_register", "lslam_host_unregister",
    "lslam_ctx_stream", "lslam_abi_sizes", "lslam_set_timing", "lslam_set_timing_mask", "lslam_timing",
    "lslam_timing_reset", "lslam_set_steps_budget",
    "lslam_ransac_params_default", "lslam_ukf_params_default", "lslam_inlier_cutoff", "lslam_ukf_weights",
    "lslam_mt_seed_state", "lslam_polar_to_xy", "lslam_hyp_mt19937", "lslam_ransac", "lslam_landmarks",
    "lslam_ukf_step", "lslam_ukf_trace", "lslam_scan_pipeline", "lslam_express_decode", "lslam_express_scans",
    "lslam_match_params_default", "lslam_scan_match",
    "lslam_grid_abi_sizes", "lslam_grid_params_default", "lslam_grid_update",
    "lslam_mapmatch_abi_sizes", "lslam_mapmatch_params_default", "lslam_map_match",
    "lslam_mapfuse_abi_sizes", "lslam_mapfuse_params_default", "lslam_map_fuse",
    "lslam_reloc_abi_sizes", "lslam_reloc_params_default", "lslam_map_relocalize", "lslam_set_reloc_budget",
    "lslam_raycast_abi_sizes", "lslam_raycast_params_default", "lslam_grid_raycast",
    "lslam_recentre_abi_sizes", "lslam_recentre_params_default", "lslam_grid_recentre",
    "lslam_dist_abi_sizes", "lslam_dist_params_default", "lslam_fieldscore_params_default",
    "lslam_grid_distance", "lslam_field_score",
    "lslam_fieldalign_abi_sizes", "lslam_fieldalign_params_default", "lslam_field_align",
    "lslam_fieldfuse_abi_sizes", "lslam_fieldfuse_params_default", "lslam_field_fuse",
    "lslam_relocprior_abi_sizes", "lslam_relocprior_params_default", "lslam_map_relocalize_prior",
    "lslam_page_abi_sizes", "lslam_page_params_default", "lslam_grid_recentre_paged", "lslam_grid_page_flush",
    "lslam_grid_page_load",
    "lslam_gridmerge_abi_sizes", "lslam_gridmerge_params_default", "lslam_grid_merge",
    "lslam_gridpoints_abi_sizes", "lslam_gridpoints_params_default", "lslam_grid_points",
    "lslam_posegraph_abi_sizes", "lslam_posegraph_params_default", "lslam_pose_graph",
    "lslam_posegate_abi_sizes", "lslam_posegate_params_default", "lslam_pose_graph_gate",
]

_lib = None
_err = None


def load():
    """Load and type the library (raises HIPLibraryError if unavailable)."""
    global _lib, _err
    if _lib is not None:
        return _lib
    if _err is not None:
        raise _err
    if not os.path.exists(LIB_PATH):
        _err = HIPLibraryError("HIP library %s is not built; run `python -m lidar_slam_amd.build` "
                               "(there is no CPU fallback)" % LIB_PATH)
        raise _err
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        _err = HIPLibraryError("cannot load %s: %s" % (LIB_PATH, e))
        raise _err
    P = C.POINTER
    i32, i64, u32, dbl, sz = C.c_int32, C.c_int64, C.c_uint32, C.c_double, C.c_size_t
    sig = {
        "lslam_version": ([], C.c_char_p),
        "lslam_status_string": ([C.c_int], C.c_char_p),
        "lslam_last_error": ([], C.c_char_p),
        "lslam_device_count": ([P(C.c_int)], C.c_int),
        "lslam_ctx_create": ([C.c_int, P(_VP)], C.c_int),
        "lslam_ctx_destroy": ([_VP], C.c_int),
        "lslam_sync": ([_VP], C.c_int),
        "lslam_malloc": ([_VP, sz, P(_VP)], C.c_int),
        "lslam_free": ([_VP, _VP], C.c_int),
        "lslam_host_alloc": ([sz, P(_VP)], C.c_int),
        "lslam_host_free": ([_VP], C.c_int),
        "lslam_h2d": ([_VP, _VP, _VP, sz], C.c_int),
        "lslam_d2h": ([_VP, _VP, _VP, sz], C.c_int),
        "lslam_d2d": ([_VP, _VP, _VP, sz], C.c_int),
        "lslam_memset": ([_VP, _VP, C.c_int, sz], C.c_int),
        "lslam_host_register": ([_VP, sz], C.c_int),
        "lslam_host_unregister": ([_VP], C.c_int),
        "lslam_ctx_stream": ([_VP, P(_VP)], C.c_int),
        "lslam_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_set_timing": ([_VP, C.c_int], C.c_int),
        "lslam_set_timing_mask": ([_VP, u32], C.c_int),
        "lslam_timing": ([_VP, C.c_int, P(dbl), P(i64)], C.c_int),
        "lslam_timing_reset": ([_VP], C.c_int),
        "lslam_set_steps_budget": ([_VP, i64], C.c_int),
        "lslam_ransac_params_default": ([P(RansacParams)], C.c_int),
        "lslam_ukf_params_default": ([P(UkfParams), i32], C.c_int),
        "lslam_inlier_cutoff": ([dbl], dbl),
        "lslam_ukf_weights": ([P(UkfParams), P(dbl), P(dbl), P(dbl)], C.c_int),
        "lslam_mt_seed_state": ([u32, P(u32)], C.c_int),
        "lslam_polar_to_xy": ([_VP, _VP, _VP, _VP, i64], C.c_int),
        "lslam_hyp_mt19937": ([_VP, P(ScanBatch), i32], C.c_int),
        "lslam_ransac": ([_VP, P(ScanBatch), P(RansacParams)], C.c_int),
        "lslam_landmarks": ([_VP, P(ScanBatch), P(RansacParams)], C.c_int),
        "lslam_ukf_step": ([_VP, P(ScanBatch), P(UkfParams)], C.c_int),
        "lslam_ukf_trace": ([_VP, P(ScanBatch), P(UkfParams), _VP], C.c_int),
        "lslam_scan_pipeline": ([_VP, P(ScanBatch), P(RansacParams), P(UkfParams)], C.c_int),
        "lslam_express_decode": ([_VP, _VP, i64, P(ExpressMeasures)], C.c_int),
        "lslam_express_scans": ([_VP, _VP, i64, i32, P(ExpressRevs)], C.c_int),
        "lslam_match_params_default": ([P(MatchParams)], C.c_int),
        "lslam_scan_match": ([_VP, P(MatchBatch), P(MatchParams), P(UkfParams)], C.c_int),
        "lslam_grid_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_grid_params_default": ([P(GridParams)], C.c_int),
        "lslam_grid_update": ([_VP, P(GridBatch), P(GridParams)], C.c_int),
        "lslam_mapmatch_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_mapmatch_params_default": ([P(MapMatchParams)], C.c_int),
        "lslam_map_match": ([_VP, P(MapMatchBatch), P(GridParams), P(MapMatchParams)], C.c_int),
        "lslam_mapfuse_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_mapfuse_params_default": ([P(MapFuseParams)], C.c_int),
        "lslam_map_fuse": ([_VP, P(MapFuseBatch), P(GridParams), P(MapMatchParams), P(MapFuseParams)], C.c_int),
        "lslam_reloc_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_reloc_params_default": ([P(RelocParams)], C.c_int),
        "lslam_map_relocalize": ([_VP, P(RelocBatch), P(GridParams), P(MapMatchParams), P(RelocParams)], C.c_int),
        "lslam_set_reloc_budget": ([_VP, i64], C.c_int),
        "lslam_raycast_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_raycast_params_default": ([P(RaycastParams)], C.c_int),
        "lslam_grid_raycast": ([_VP, P(RaycastBatch), P(GridParams), P(RaycastParams)], C.c_int),
        "lslam_recentre_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_recentre_params_default": ([P(RecentreParams)], C.c_int),
        "lslam_grid_recentre": ([_VP, P(RecentreBatch), P(GridParams), P(RecentreParams)], C.c_int),
        "lslam_dist_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_dist_params_default": ([P(DistParams)], C.c_int),
        "lslam_fieldscore_params_default": ([P(FieldScoreParams)], C.c_int),
        "lslam_grid_distance": ([_VP, P(DistBatch), P(GridParams), P(DistParams)], C.c_int),
        "lslam_field_score": ([_VP, P(FieldScoreBatch), P(GridParams), P(FieldScoreParams)], C.c_int),
        "lslam_fieldalign_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_fieldalign_params_default": ([P(FieldAlignParams)], C.c_int),
        "lslam_field_align": ([_VP, P(FieldAlignBatch), P(GridParams), P(FieldAlignParams)], C.c_int),
        "lslam_fieldfuse_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_fieldfuse_params_default": ([P(FieldFuseParams)], C.c_int),
        "lslam_field_fuse": ([_VP, P(FieldFuseBatch), P(GridParams), P(FieldAlignParams), P(FieldFuseParams)], C.c_int),
        "lslam_relocprior_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_relocprior_params_default": ([P(RelocPriorParams)], C.c_int),
        "lslam_map_relocalize_prior": ([_VP, P(RelocPriorBatch), P(GridParams), P(MapMatchParams), P(RelocParams),
                                        P(RelocPriorParams)], C.c_int),
        "lslam_page_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_page_params_default": ([P(PageParams)], C.c_int),
        "lslam_grid_recentre_paged": ([_VP, P(RecentreBatch), P(PageBatch), P(GridParams), P(RecentreParams), P(PageParams)],
                                      C.c_int),
        "lslam_grid_page_flush": ([_VP, P(PageBatch), _VP, P(GridParams), P(PageParams)], C.c_int),
        "lslam_grid_page_load": ([_VP, P(PageBatch), _VP, P(GridParams), P(PageParams)], C.c_int),
        "lslam_gridmerge_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_gridmerge_params_default": ([P(GridMergeParams)], C.c_int),
        "lslam_grid_merge": ([_VP, P(GridMergeBatch), P(GridParams), P(GridMergeParams)], C.c_int),
        "lslam_gridpoints_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_gridpoints_params_default": ([P(GridPointsParams)], C.c_int),
        "lslam_grid_points": ([_VP, P(GridPointsBatch), P(GridParams), P(GridPointsParams)], C.c_int),
        "lslam_posegraph_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_posegraph_params_default": ([P(PoseGraphParams)], C.c_int),
        "lslam_pose_graph": ([_VP, P(PoseGraphBatch), P(PoseGraphParams)], C.c_int),
        "lslam_posegate_abi_sizes": ([P(i64), C.c_int], C.c_int),
        "lslam_posegate_params_default": ([P(PoseGateParams)], C.c_int),
        "lslam_pose_graph_gate": ([_VP, P(PoseGateBatch), P(PoseGateParams)], C.c_int),
    }
    try:
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
    except AttributeError as e:
        _err = HIPLibraryError("%s lacks %s: a stale build? rebuild with `python -m lidar_slam_amd.build`"
                               % (LIB_PATH, e))
        raise _err
    _check_abi(L)
    _lib = L
    return L


def _check_abi(L):
    """The library must be the ABI these ctypes layouts describe: a stale .so (e.g. via LSLAM_LIB)
    would silently ignore appended struct fields."""
    global _err
    ver = L.lslam_version().decode(errors="replace")
    m = re.search(r"\(abi (\d+), src ([0-9a-f]{16}),", ver)
    if not m or int(m.group(1)) != ABI_VERSION:
        _err = HIPLibraryError("%s reports %r; this binding needs ABI %d (rebuild the library)"
                               % (LIB_PATH, ver, ABI_VERSION))
        raise _err
    _check_source(m.group(2))
    got, want = [], []
    for sizes, structs in _ABI_SIZES:
        buf = (C.c_int64 * len(structs))()
        getattr(L, sizes)(buf, len(structs))
        got += list(buf)
        want += [C.sizeof(t) for t in structs]
    if got != want:
        _err = HIPLibraryError("struct sizes differ between %s %s and the ctypes layouts %s" % (LIB_PATH, got, want))
        raise _err


# the exported sizes functions and the structs each reports, in its order
_ABI_SIZES = [
    ("lslam_abi_sizes", (ChunkModel, LandmarkRec, RansacParams, UkfParams, ScanBatch, ExpressMeasures, ExpressRevs,
                         MatchParams, MatchBatch)),
    ("lslam_grid_abi_sizes", (GridParams, GridBatch)),
    ("lslam_mapmatch_abi_sizes", (MapMatchParams, MapMatchBatch)),
    ("lslam_mapfuse_abi_sizes", (MapFuseParams, MapFuseBatch)),
    ("lslam_reloc_abi_sizes", (RelocParams, RelocBatch)),
    ("lslam_raycast_abi_sizes", (RaycastParams, RaycastBatch)),
    ("lslam_recentre_abi_sizes", (RecentreParams, RecentreBatch)),
    ("lslam_dist_abi_sizes", (DistParams, DistBatch, FieldScoreParams, FieldScoreBatch)),
    ("lslam_fieldalign_abi_sizes", (FieldAlignParams, FieldAlignBatch)),
    ("lslam_fieldfuse_abi_sizes", (FieldFuseParams, FieldFuseBatch)),
    ("lslam_relocprior_abi_sizes", (RelocPriorParams, RelocPriorBatch)),
    ("lslam_page_abi_sizes", (PageParams, PageBatch)),
    ("lslam_gridmerge_abi_sizes", (GridMergeParams, GridMergeBatch)),
    ("lslam_gridpoints_abi_sizes", (GridPointsParams, GridPointsBatch)),
    ("lslam_posegraph_abi_sizes", (PoseGraphParams, PoseGraphBatch)),
    ("lslam_posegate_abi_sizes", (PoseGateParams, PoseGateBatch)),
]


def _check_source(lib_hash, want=None):
    """The library must be built from the sources next to it: a stale .so (built from other
    sources, e.g. an A/B leftover) raises.  ``LSLAM_ALLOW_STALE=1`` skips the check (A/B runs of
    deliberately different builds via LSLAM_LIB)."""
    global _err
    if os.environ.get("LSLAM_ALLOW_STALE") == "1":
        return
    if want is None:
        from . import build
        want = build.source_hash()
    if lib_hash != want:
        _err = HIPLibraryError("%s was built from other sources (src %s, the tree's is %s): rebuild with "
                               "`python -m lidar_slam_amd.build`" % (LIB_PATH, lib_hash, want))
        raise _err


def check(status, what=""):
    if status != LSLAM_OK:
        L = load()
        msg = L.lslam_last_error().decode(errors="replace")
        st = L.lslam_status_string(status).decode()
        if status == LSLAM_ERR_ARG:
            raise ValueError("%s: %s (%s)" % (what, st, msg))
        raise HIPLibraryError("%s: %s (%s)" % (what, st, msg))
    return status


def call(name, ctx, batch, *params):
    """Entry point ``name`` on ``ctx`` with a batch and its parameter structs, each passed by reference
    (None: NULL), the status checked under the entry point's name.  The by-reference is ctypes' own:
    ``load`` declares those arguments as pointers, and a struct given for a pointer is passed so."""
    return check(getattr(load(), name)(ctx.handle, batch, *params), name)


def _params_factory(name, struct):
    """``name_params(**kw)``: the library's defaults for ``struct`` with the given fields set."""
    def make(**kw):
        p = struct()
        getattr(load(), "lslam_%s_params_default" % name)(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    make.__name__ = make.__qualname__ = name + "_params"
    return make


ransac_params = _params_factory("ransac", RansacParams)
match_params = _params_factory("match", MatchParams)
grid_params = _params_factory("grid", GridParams)
mapmatch_params = _params_factory("mapmatch", MapMatchParams)
mapfuse_params = _params_factory("mapfuse", MapFuseParams)
reloc_params = _params_factory("reloc", RelocParams)
raycast_params = _params_factory("raycast", RaycastParams)
recentre_params = _params_factory("recentre", RecentreParams)
dist_params = _params_factory("dist", DistParams)
fieldscore_params = _params_factory("fieldscore", FieldScoreParams)
fieldalign_params = _params_factory("fieldalign", FieldAlignParams)
fieldfuse_params = _params_factory("fieldfuse", FieldFuseParams)
relocprior_params = _params_factory("relocprior", RelocPriorParams)
page_params = _params_factory("page", PageParams)
gridmerge_params = _params_factory("gridmerge", GridMergeParams)
gridpoints_params = _params_factory("gridpoints", GridPointsParams)
posegraph_params = _params_factory("posegraph", PoseGraphParams)
posegate_params = _params_factory("posegate", PoseGateParams)


def ukf_params(n_landmarks, **kw):
    p = UkfParams()
    load().lslam_ukf_params_default(C.byref(p), int(n_landmarks))
    for k, v in kw.items():
        if k == "Q":
            for i, q in enumerate(list(v)):
                p.Q[i] = float(q)
        else:
            setattr(p, k, v)
    return p
