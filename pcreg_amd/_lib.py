"""Loader of libpcreg_hip.so (the C ABI declared in include/pcreg.h).

There is no CPU fallback: if the shared library has not been built, or no gfx950
device is usable, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCREG_LIB") or os.path.join(_HERE, "libpcreg_hip.so")     # PCREG_LIB: another build of the same library (A/B runs)

PCREG_OK, PCREG_E_ARG, PCREG_E_HIP, PCREG_E_NODEVICE, PCREG_E_WORKSPACE = 0, 1, 2, 3, 4
KNN_MAX_K = 32                   # PCREG_KNN_MAX_K
METRIC_SAD, METRIC_SSD = 0, 1
LAYOUT_FEATURE_MAJOR, LAYOUT_ROW_MAJOR = 0, 1


class PcregError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libpcreg_hip error {code}: {msg}")
        self.code = code


class RansacOpts(C.Structure):
    """pcreg_ransac_opts (include/pcreg.h) == ransacCoef of ransac.m:7-12."""
    _fields_ = [("minPtNum", C.c_int32), ("iterNum", C.c_int32), ("thDist", C.c_double),
                ("thInlrRatio", C.c_double), ("REFINE", C.c_int32), ("VERBOSE", C.c_int32),
                ("seed", C.c_uint64)]


class MatchOpts(C.Structure):
    """pcreg_match_opts (include/pcreg.h) == `par` of getMatches.m."""
    _fields_ = [("metric", C.c_int32), ("matchThreshold", C.c_double), ("maxRatio", C.c_double),
                ("unique", C.c_int32), ("prenormalized", C.c_int32), ("unnormalize", C.c_int32),
                ("norm_factor", C.c_double), ("change_metric", C.c_int32), ("metric_factor", C.c_double)]


class DescOpts(C.Structure):
    """pcreg_desc_opts (include/pcreg.h) == `options` of getSpacialHistogramDescriptors.m."""
    _fields_ = [("min_pts", C.c_int32), ("max_pts", C.c_int32), ("R", C.c_double), ("thVar", C.c_double * 2),
                ("k", C.c_double), ("ALIGN_POINTS", C.c_int32)]


class DevRansacResult(C.Structure):
    """pcreg_dev_ransac_result (include/pcreg.h)."""
    _fields_ = [("T", C.c_double * 16), ("n_inliers", C.c_int32), ("num_success", C.c_int32),
                ("max_inliers", C.c_int32), ("failed", C.c_int32), ("n", C.c_int32), ("winner", C.c_int32)]


class FgrOpts(C.Structure):
    """pcreg_fgr_opts (include/pcreg.h)."""
    _fields_ = [("delta2", C.c_double), ("iterations", C.c_int32), ("decrease_every", C.c_int32), ("division_factor", C.c_double),
                ("mu0", C.c_double), ("n_tuples", C.c_int32), ("reserved", C.c_int32), ("tuple_scale", C.c_double), ("seed", C.c_uint64)]


class FgrResult(C.Structure):
    """pcreg_fgr_result (include/pcreg.h)."""
    _fields_ = [("T", C.c_double * 16), ("mu0", C.c_double), ("mu_final", C.c_double), ("cost", C.c_double), ("sum_d2", C.c_double),
                ("failed", C.c_int32), ("n", C.c_int32), ("n_live", C.c_int32), ("n_kept", C.c_int32), ("n_inliers", C.c_int32),
                ("reserved", C.c_int32)]


# every symbol include/pcreg.h declares (tests/test_abi.py checks the two lists agree)
SYMBOLS = [
    "pcreg_last_error", "pcreg_version", "pcreg_device_count", "pcreg_set_device", "pcreg_device_name", "pcreg_debug_set", "pcreg_debug_match_stats",
    "pcreg_debug_knn_stats", "pcreg_debug_knn_unit_stats", "pcreg_debug_knn_direct_stats", "pcreg_debug_ransac_stats", "pcreg_debug_ransac_handover", "pcreg_debug_cluster_stats", "pcreg_debug_desc_stats", "pcreg_debug_dev_model_export", "pcreg_debug_search_export",
    "pcreg_estimate_transform", "pcreg_calc_dists", "pcreg_ransac", "pcreg_ransac_batched",
    "pcreg_fgr_resident_capacity", "pcreg_fgr_batched", "pcreg_dev_fgr_batched_workspace", "pcreg_dev_fgr_batched",
    "pcreg_knn2_points_f32", "pcreg_match_points_f32", "pcreg_match_features", "pcreg_get_matches", "pcreg_desc_set_create", "pcreg_desc_set_destroy", "pcreg_desc_set_size", "pcreg_get_matches_on_sets", "pcreg_get_matches_segmented_on_sets", "pcreg_sphere_counts", "pcreg_sphere_sweep", "pcreg_sphere_model_create", "pcreg_sphere_model_destroy", "pcreg_sphere_sweep_on_model", "pcreg_final_stage_limits", "pcreg_final_stage", "pcreg_get_matches_segmented", "pcreg_get_local_points",
    "pcreg_model_create", "pcreg_model_destroy", "pcreg_model_size", "pcreg_model_match_points_f32", "pcreg_model_knn_f32", "pcreg_knn_points_f32",
    "pcreg_model_range_f32", "pcreg_range_points_f32", "pcreg_model_cluster_f32", "pcreg_cluster_points_f32",
    "pcreg_model_dbscan_f32", "pcreg_dbscan_points_f32", "pcreg_dev_model_dbscan_workspace", "pcreg_dev_model_dbscan_f32",
    "pcreg_dev_model_create", "pcreg_dev_model_destroy", "pcreg_dev_model_search_workspace", "pcreg_dev_model_search_f32",
    "pcreg_dev_model_knn_workspace", "pcreg_dev_model_knn_f32", "pcreg_dev_merge_topk_f32",
    "pcreg_dev_model_range_workspace", "pcreg_dev_model_range_count_f32", "pcreg_dev_model_range_fill_f32",
    "pcreg_dev_model_cluster_workspace", "pcreg_dev_model_cluster_f32",
    "pcreg_model_score_f32", "pcreg_dev_model_score_workspace", "pcreg_dev_model_score_f32",
    "pcreg_model_refit_f32", "pcreg_dev_model_refit_workspace", "pcreg_dev_model_refit_f32",
    "pcreg_model_normals_f32", "pcreg_point_normals_f32", "pcreg_dev_model_normals_workspace", "pcreg_dev_model_normals_f32",
    "pcreg_model_refit_plane_f32", "pcreg_dev_model_refit_plane_workspace", "pcreg_dev_model_refit_plane_f32",
    "pcreg_model_refit_gicp_f32", "pcreg_dev_model_refit_gicp_workspace", "pcreg_dev_model_refit_gicp_f32",
    "pcreg_model_score_trimmed_f32", "pcreg_dev_model_score_trimmed_f32",
    "pcreg_model_refit_trimmed_f32", "pcreg_dev_model_refit_trimmed_f32",
    "pcreg_model_refit_plane_trimmed_f32", "pcreg_dev_model_refit_plane_trimmed_f32",
    "pcreg_model_refit_gicp_trimmed_f32", "pcreg_dev_model_refit_gicp_trimmed_f32",
    "pcreg_model_refit_cpd_f32", "pcreg_dev_model_refit_cpd_workspace", "pcreg_dev_model_refit_cpd_f32",
    "pcreg_model_denoise_f32", "pcreg_point_denoise_f32", "pcreg_dev_model_denoise_workspace", "pcreg_dev_model_denoise_f32",
    "pcreg_model_fps_f32", "pcreg_point_fps_f32", "pcreg_dev_model_fps_workspace", "pcreg_dev_model_fps_f32", "pcreg_debug_fps_stats",
    "pcreg_model_fpfh_f32", "pcreg_point_fpfh_f32", "pcreg_dev_model_fpfh_workspace", "pcreg_dev_model_fpfh_f32",
    "pcreg_model_fpfh_radius_f32", "pcreg_point_fpfh_radius_f32", "pcreg_dev_model_fpfh_radius_workspace", "pcreg_dev_model_fpfh_radius_count_f32",
    "pcreg_dev_model_fpfh_radius_f32",
    "pcreg_model_iss_f32", "pcreg_point_iss_f32", "pcreg_dev_model_iss_workspace", "pcreg_dev_model_iss_f32",
    "pcreg_model_fit_planes_f32", "pcreg_point_fit_planes_f32", "pcreg_dev_model_fit_planes_workspace", "pcreg_dev_model_fit_planes_f32",
    "pcreg_model_fit_spheres_f32", "pcreg_point_fit_spheres_f32", "pcreg_dev_model_fit_spheres_workspace", "pcreg_dev_model_fit_spheres_f32",
    "pcreg_model_fit_cylinders_f32", "pcreg_point_fit_cylinders_f32", "pcreg_dev_model_fit_cylinders_workspace", "pcreg_dev_model_fit_cylinders_f32",
    "pcreg_unique_rows3", "pcreg_aggregate_matches", "pcreg_dev_unique_rows3_workspace", "pcreg_dev_unique_rows3_f64",
    "pcreg_dev_aggregate_matches_workspace", "pcreg_dev_aggregate_matches", "pcreg_dev_estimate_transform_indexed",
    "pcreg_downsample_grid_f32", "pcreg_dev_downsample_grid_workspace", "pcreg_dev_downsample_grid_chunk", "pcreg_dev_downsample_grid_f32",
    "pcreg_ndt_create", "pcreg_ndt_destroy", "pcreg_ndt_size", "pcreg_ndt_get", "pcreg_ndt_refit_f32",
    "pcreg_dev_ndt_create", "pcreg_dev_ndt_destroy", "pcreg_dev_ndt_size", "pcreg_dev_ndt_get", "pcreg_dev_ndt_refit_workspace", "pcreg_dev_ndt_refit_f32",
    "pcreg_dev_model_match_f32", "pcreg_dev_model_match_table_f32", "pcreg_dev_match_from_table_f32",
    "pcreg_align_points_knn", "pcreg_align_points_knn_f32", "pcreg_align_points_knn_batched", "pcreg_spatial_histogram_descriptors",
    "pcreg_spatial_histogram_descriptors_f32", "pcreg_spatial_histogram_descriptors_mixed",
    "pcreg_dev_knn2_points_f32_workspace", "pcreg_dev_knn2_points_f32", "pcreg_dev_merge_top2_f32", "pcreg_dev_merge_top2_strided_f32",
    "pcreg_dev_ransac_workspace", "pcreg_dev_ransac",
    "pcreg_dev_ransac_partial", "pcreg_dev_ransac_finish", "pcreg_dev_ransac_finish_parts",
    "pcreg_dev_search_kernel_timing", "pcreg_dev_search_kernel_ms",
    "pcreg_dev_spatial_histogram_descriptors_workspace", "pcreg_dev_spatial_histogram_descriptors",
    "pcreg_dev_spatial_histogram_descriptors_rows_u16", "pcreg_dev_get_matches_rows_u16",
    "pcreg_dev_get_matches_workspace", "pcreg_dev_get_matches", "pcreg_dev_gather_matched_rows",
    "pcreg_dev_sphere_counts", "pcreg_dev_sphere_select_workspace", "pcreg_dev_sphere_select", "pcreg_dev_sphere_select_batched",
    "pcreg_dev_get_matches_segmented_workspace", "pcreg_dev_get_matches_segmented", "pcreg_dev_segmented_model_bytes", "pcreg_dev_segmented_model_prepare", "pcreg_dev_get_matches_segmented_prepared",
    "pcreg_dev_gather_rows_f64", "pcreg_dev_sweep_plan", "pcreg_dev_sweep_gather", "pcreg_dev_ransac_batched_workspace",
    "pcreg_dev_ransac_batched", "pcreg_dev_align_points_knn_batched", "pcreg_dev_quick_tf", "pcreg_dev_refine_by_distance",
    "pcreg_dev_quick_tf_batched", "pcreg_dev_final_close_refine_batched", "pcreg_dev_final_pick_apply",
    "pcreg_comm_get_unique_id", "pcreg_comm_init", "pcreg_comm_init_host_staged", "pcreg_comm_rank", "pcreg_comm_destroy",
    "pcreg_match_points_sharded_f32", "pcreg_ransac_sharded",
    "pcreg_pcd_info", "pcreg_pcd_read", "pcreg_pcd_write", "pcreg_mat_read_double",
]

_lib = None


def lib() -> C.CDLL:
    """The loaded library; raises if it was never built (run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C pcreg_amd/csrc` "
                "(or __graft_entry__.build()).  pcreg_amd has no CPU fallback.")
        # Load torch (the process's device-memory / RCCL plumbing) BEFORE the library: the
        # torch wheel bundles its own HIP runtime, and on this image the runtime that is
        # loaded second only sees the GPU when torch's was loaded first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.pcreg_last_error.restype = C.c_char_p
        L.pcreg_version.restype = C.c_char_p
        for name in ("pcreg_dev_model_search_workspace", "pcreg_dev_knn2_points_f32_workspace",
                     "pcreg_dev_ransac_workspace", "pcreg_dev_spatial_histogram_descriptors_workspace",
                     "pcreg_dev_get_matches_workspace", "pcreg_dev_sphere_select_workspace", "pcreg_dev_ransac_batched_workspace",
                     "pcreg_dev_get_matches_segmented_workspace", "pcreg_dev_segmented_model_bytes"):
            getattr(L, name).restype = C.c_size_t
        if hasattr(L, "pcreg_dev_model_knn_workspace"):     # (an older build given through PCREG_LIB lacks the k-nearest search)
            L.pcreg_dev_model_knn_workspace.restype = C.c_size_t
        if hasattr(L, "pcreg_dev_model_range_workspace"):   # (an older build given through PCREG_LIB lacks the radius search)
            L.pcreg_dev_model_range_workspace.restype = C.c_size_t
            vp, i, f, i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64          # (a float and 64-bit integers by value: declared)
            L.pcreg_dev_model_range_count_f32.argtypes = [vp, vp, i, i, f, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_dev_model_range_fill_f32.argtypes = [vp, vp, i, i, f, C.c_int32, vp, i64, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_range_f32.argtypes = [vp, vp, i, i, f, i64, vp, vp, vp]
            L.pcreg_range_points_f32.argtypes = [vp, i, i, vp, i, i, f, i64, vp, vp, vp]
        if hasattr(L, "pcreg_dev_model_cluster_workspace"):   # (an older build given through PCREG_LIB lacks the clustering)
            L.pcreg_dev_model_cluster_workspace.restype = C.c_size_t
            L.pcreg_dev_model_cluster_workspace.argtypes = [C.c_int]
            vp, i, f = C.c_void_p, C.c_int, C.c_float                            # (a float by value: declared)
            L.pcreg_dev_model_cluster_f32.argtypes = [vp, f, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_cluster_f32.argtypes = [vp, f, vp, vp, vp, vp]
            L.pcreg_cluster_points_f32.argtypes = [vp, i, i, f, vp, vp, vp, vp]
            L.pcreg_debug_cluster_stats.argtypes = [C.POINTER(C.c_longlong), C.c_int]
        if hasattr(L, "pcreg_dev_model_dbscan_workspace"):    # (an older build given through PCREG_LIB lacks DBSCAN)
            L.pcreg_dev_model_dbscan_workspace.restype = C.c_size_t
            L.pcreg_dev_model_dbscan_workspace.argtypes = [C.c_int]
            vp, i, f = C.c_void_p, C.c_int, C.c_float                            # (a float by value: declared)
            L.pcreg_dev_model_dbscan_f32.argtypes = [vp, f, i, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_dbscan_f32.argtypes = [vp, f, i, vp, vp, vp, vp, vp, vp]
            L.pcreg_dbscan_points_f32.argtypes = [vp, i, i, f, i, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "pcreg_dev_model_score_workspace"):     # (an older build given through PCREG_LIB lacks the transform scoring)
            L.pcreg_dev_model_score_workspace.restype = C.c_size_t
            L.pcreg_dev_model_score_workspace.argtypes = [C.c_int] * 3
            vp, i, f = C.c_void_p, C.c_int, C.c_float                            # (a float by value: declared)
            L.pcreg_dev_model_score_f32.argtypes = [vp, vp, i, i, vp, i, f, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_score_f32.argtypes = [vp, vp, i, i, vp, i, f, vp, vp, vp, vp]
        if hasattr(L, "pcreg_dev_model_refit_workspace"):     # (an older build given through PCREG_LIB lacks the refit)
            L.pcreg_dev_model_refit_workspace.restype = C.c_size_t
            L.pcreg_dev_model_refit_workspace.argtypes = [C.c_int] * 3
            vp, i, f = C.c_void_p, C.c_int, C.c_float
            L.pcreg_dev_model_refit_f32.argtypes = [vp, vp, i, i, vp, i, f, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_refit_f32.argtypes = [vp, vp, i, i, vp, i, f, i, vp, vp, vp, vp]
        if hasattr(L, "pcreg_dev_model_normals_workspace"):   # (an older build given through PCREG_LIB lacks the normals)
            L.pcreg_dev_model_normals_workspace.restype = C.c_size_t
            L.pcreg_dev_model_normals_workspace.argtypes = [C.c_int] * 2
            vp, i = C.c_void_p, C.c_int
            L.pcreg_dev_model_normals_f32.argtypes = [vp, i, vp, vp, i, vp, vp, C.c_size_t, vp]
            L.pcreg_model_normals_f32.argtypes = [vp, i, vp, vp, i, vp]
            L.pcreg_point_normals_f32.argtypes = [vp, i, i, i, vp, vp, i, vp]
        if hasattr(L, "pcreg_dev_model_denoise_workspace"):   # (an older build given through PCREG_LIB lacks the denoising)
            L.pcreg_dev_model_denoise_workspace.restype = C.c_size_t
            L.pcreg_dev_model_denoise_workspace.argtypes = [C.c_int] * 2
            vp, i, d = C.c_void_p, C.c_int, C.c_double                           # (a double by value: declared)
            L.pcreg_dev_model_denoise_f32.argtypes = [vp, i, d, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_denoise_f32.argtypes = [vp, i, d, vp, vp, vp, vp]
            L.pcreg_point_denoise_f32.argtypes = [vp, i, i, i, d, vp, vp, vp, vp]
        if hasattr(L, "pcreg_dev_model_fps_workspace"):       # (an older build given through PCREG_LIB lacks the farthest point sampling)
            L.pcreg_dev_model_fps_workspace.restype = C.c_size_t
            L.pcreg_dev_model_fps_workspace.argtypes = [C.c_int] * 2
            vp, i, f = C.c_void_p, C.c_int, C.c_float                            # (a float by value: declared)
            L.pcreg_dev_model_fps_f32.argtypes = [vp, i, i, f, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_fps_f32.argtypes = [vp, i, i, f, vp, vp, vp, vp, vp, vp]
            L.pcreg_point_fps_f32.argtypes = [vp, i, i, i, i, f, vp, vp, vp, vp, vp, vp]
            L.pcreg_debug_fps_stats.argtypes = [C.POINTER(C.c_longlong), C.c_int]
        if hasattr(L, "pcreg_dev_model_fpfh_workspace"):      # (an older build given through PCREG_LIB lacks the FPFH)
            L.pcreg_dev_model_fpfh_workspace.restype = C.c_size_t
            L.pcreg_dev_model_fpfh_workspace.argtypes = [C.c_int] * 2
            vp, i = C.c_void_p, C.c_int
            L.pcreg_dev_model_fpfh_f32.argtypes = [vp, i, vp, i, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_fpfh_f32.argtypes = [vp, i, vp, i, i, vp, vp, i, vp]
            L.pcreg_point_fpfh_f32.argtypes = [vp, i, i, i, vp, i, i, vp, vp, i, vp]
        if hasattr(L, "pcreg_dev_model_fpfh_radius_workspace"):   # (an older build given through PCREG_LIB lacks the radius FPFH)
            L.pcreg_dev_model_fpfh_radius_workspace.restype = C.c_size_t
            L.pcreg_dev_model_fpfh_radius_workspace.argtypes = [C.c_int, C.c_int64]
            vp, i, f, i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64            # (floats and 64-bit integers by value: declared)
            L.pcreg_dev_model_fpfh_radius_count_f32.argtypes = [vp, f, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_dev_model_fpfh_radius_f32.argtypes = [vp, f, i, vp, i, vp, i64, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_fpfh_radius_f32.argtypes = [vp, f, i, vp, i, i, vp, vp, i, vp, vp]
            L.pcreg_point_fpfh_radius_f32.argtypes = [vp, i, i, f, i, vp, i, i, vp, vp, i, vp, vp]
        if hasattr(L, "pcreg_dev_model_iss_workspace"):       # (an older build given through PCREG_LIB lacks the ISS keypoints)
            L.pcreg_dev_model_iss_workspace.restype = C.c_size_t
            L.pcreg_dev_model_iss_workspace.argtypes = [C.c_int]
            vp, i, f, d = C.c_void_p, C.c_int, C.c_float, C.c_double             # (floats and doubles by value: declared)
            L.pcreg_dev_model_iss_f32.argtypes = [vp, f, f, d, d, i, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_iss_f32.argtypes = [vp, f, f, d, d, i, vp, vp, vp, vp, vp]
            L.pcreg_point_iss_f32.argtypes = [vp, i, i, f, f, d, d, i, vp, vp, vp, vp, vp]
        if hasattr(L, "pcreg_dev_model_fit_planes_workspace"):    # (an older build given through PCREG_LIB lacks the plane extraction)
            L.pcreg_dev_model_fit_planes_workspace.restype = C.c_size_t
            L.pcreg_dev_model_fit_planes_workspace.argtypes = [C.c_int, C.c_int]
            vp, i, f, d, u64 = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_uint64
            L.pcreg_dev_model_fit_planes_f32.argtypes = [vp, f, vp, d, i, i, i, u64, vp, i] + [vp] * 9 + [vp, C.c_size_t, vp]
            L.pcreg_model_fit_planes_f32.argtypes = [vp, f, vp, d, i, i, i, u64, vp] + [vp] * 9
            L.pcreg_point_fit_planes_f32.argtypes = [vp, i, i, f, vp, d, i, i, i, u64, vp] + [vp] * 9
        if hasattr(L, "pcreg_dev_model_fit_spheres_workspace"):   # (an older build given through PCREG_LIB lacks the sphere extraction)
            L.pcreg_dev_model_fit_spheres_workspace.restype = C.c_size_t
            L.pcreg_dev_model_fit_spheres_workspace.argtypes = [C.c_int, C.c_int]
            vp, i, f, u64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64
            L.pcreg_dev_model_fit_spheres_f32.argtypes = [vp, f, f, f, i, i, i, u64, vp, i] + [vp] * 9 + [vp, C.c_size_t, vp]
            L.pcreg_model_fit_spheres_f32.argtypes = [vp, f, f, f, i, i, i, u64, vp] + [vp] * 9
            L.pcreg_point_fit_spheres_f32.argtypes = [vp, i, i, f, f, f, i, i, i, u64, vp] + [vp] * 9
        if hasattr(L, "pcreg_dev_model_fit_cylinders_workspace"):   # (an older build given through PCREG_LIB lacks the cylinder extraction)
            L.pcreg_dev_model_fit_cylinders_workspace.restype = C.c_size_t
            L.pcreg_dev_model_fit_cylinders_workspace.argtypes = [C.c_int, C.c_int]
            vp, i, f, d, u64 = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_uint64
            L.pcreg_dev_model_fit_cylinders_f32.argtypes = [vp, f, f, f, vp, d, vp, i, i, i, i, u64, vp, i] + [vp] * 10 + [vp, C.c_size_t, vp]
            L.pcreg_model_fit_cylinders_f32.argtypes = [vp, f, f, f, vp, d, vp, i, i, i, i, i, u64, vp] + [vp] * 10
            L.pcreg_point_fit_cylinders_f32.argtypes = [vp, i, i, f, f, f, vp, d, vp, i, i, i, i, i, u64, vp] + [vp] * 10
        if hasattr(L, "pcreg_dev_model_refit_plane_workspace"):   # (an older build given through PCREG_LIB lacks the plane refit)
            L.pcreg_dev_model_refit_plane_workspace.restype = C.c_size_t
            L.pcreg_dev_model_refit_plane_workspace.argtypes = [C.c_int] * 3
            vp, i, f = C.c_void_p, C.c_int, C.c_float
            L.pcreg_dev_model_refit_plane_f32.argtypes = [vp, vp, i, i, vp, i, f, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_refit_plane_f32.argtypes = [vp, vp, i, i, vp, i, f, i, vp, i, i, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "pcreg_dev_model_refit_gicp_workspace"):    # (an older build given through PCREG_LIB lacks the plane-to-plane refit)
            L.pcreg_dev_model_refit_gicp_workspace.restype = C.c_size_t
            L.pcreg_dev_model_refit_gicp_workspace.argtypes = [C.c_int] * 3
            vp, i, f, d = C.c_void_p, C.c_int, C.c_float, C.c_double            # (a double by value: declared)
            L.pcreg_dev_model_refit_gicp_f32.argtypes = [vp, vp, i, i, vp, i, f, vp, i, vp, i, d, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_refit_gicp_f32.argtypes = [vp, vp, i, i, vp, i, f, i, vp, i, vp, i, i, d, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "pcreg_dev_model_score_trimmed_f32"):           # (an older build given through PCREG_LIB lacks the trimmed entries)
            vp, i, f, d = C.c_void_p, C.c_int, C.c_float, C.c_double
            # the untrimmed twins' lists with keep_ratio after r2 and n_within, d2_cut at the end
            L.pcreg_dev_model_score_trimmed_f32.argtypes = [vp, vp, i, i, vp, i, f, d, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
            L.pcreg_model_score_trimmed_f32.argtypes = [vp, vp, i, i, vp, i, f, d, vp, vp, vp, vp, vp, vp]
            L.pcreg_dev_model_refit_trimmed_f32.argtypes = [vp, vp, i, i, vp, i, f, d, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
            L.pcreg_model_refit_trimmed_f32.argtypes = [vp, vp, i, i, vp, i, f, d, i, vp, vp, vp, vp, vp, vp]
            L.pcreg_dev_model_refit_plane_trimmed_f32.argtypes = [vp, vp, i, i, vp, i, f, d, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
            L.pcreg_model_refit_plane_trimmed_f32.argtypes = [vp, vp, i, i, vp, i, f, d, i, vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
            L.pcreg_dev_model_refit_gicp_trimmed_f32.argtypes = [vp, vp, i, i, vp, i, f, d, vp, i, vp, i, d, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
            L.pcreg_model_refit_gicp_trimmed_f32.argtypes = [vp, vp, i, i, vp, i, f, d, i, vp, i, vp, i, i, d, vp, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "pcreg_dev_model_refit_cpd_workspace"):     # (an older build given through PCREG_LIB lacks the coherent-point-drift refit)
            L.pcreg_dev_model_refit_cpd_workspace.restype = C.c_size_t
            L.pcreg_dev_model_refit_cpd_workspace.argtypes = [C.c_int] * 3
            vp, i, d = C.c_void_p, C.c_int, C.c_double                          # (a double by value: declared)
            L.pcreg_dev_model_refit_cpd_f32.argtypes = [vp, vp, i, i, vp, i, vp, d, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_model_refit_cpd_f32.argtypes = [vp, vp, i, i, vp, i, vp, d, i, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "pcreg_dev_fgr_batched_workspace"):     # (an older build given through PCREG_LIB lacks fast global registration)
            L.pcreg_dev_fgr_batched_workspace.restype = C.c_size_t
            L.pcreg_dev_fgr_batched_workspace.argtypes = [C.c_int] * 3
            vp, i = C.c_void_p, C.c_int
            L.pcreg_dev_fgr_batched.argtypes = [vp, vp, i, vp, i, i, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_fgr_batched.argtypes = [vp, vp, i, i, vp, i, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "pcreg_dev_unique_rows3_workspace"):    # (an older build given through PCREG_LIB lacks unique_rows)
            for name in ("pcreg_dev_unique_rows3_workspace", "pcreg_dev_aggregate_matches_workspace"):
                getattr(L, name).restype = C.c_size_t
                getattr(L, name).argtypes = [C.c_int]
        if hasattr(L, "pcreg_dev_downsample_grid_workspace"):  # (an older build given through PCREG_LIB lacks the downsampling)
            L.pcreg_dev_downsample_grid_workspace.restype = C.c_size_t
            L.pcreg_dev_downsample_grid_workspace.argtypes = [C.c_int]
            L.pcreg_dev_downsample_grid_chunk.argtypes = []
            vp, i, d = C.c_void_p, C.c_int, C.c_double                           # (a double by value: declared)
            L.pcreg_dev_downsample_grid_f32.argtypes = [vp, i, i, d, vp, i, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_downsample_grid_f32.argtypes = [vp, i, i, d, vp, i, vp, vp, vp]
        if hasattr(L, "pcreg_dev_ndt_refit_workspace"):     # (an older build given through PCREG_LIB lacks the NDT)
            L.pcreg_dev_ndt_refit_workspace.restype = C.c_size_t
            L.pcreg_dev_ndt_refit_workspace.argtypes = [C.c_int, C.c_int]
            vp, i, d = C.c_void_p, C.c_int, C.c_double
            L.pcreg_dev_ndt_create.argtypes = [vp, i, i, d, i, vp, vp]
            L.pcreg_ndt_create.argtypes = [vp, i, i, d, i, vp]
            for name in ("pcreg_dev_ndt_destroy", "pcreg_ndt_destroy"):
                getattr(L, name).argtypes = [vp]
            for name in ("pcreg_dev_ndt_size", "pcreg_ndt_size"):
                getattr(L, name).argtypes = [vp, vp, vp]
            for name in ("pcreg_dev_ndt_get", "pcreg_ndt_get"):
                getattr(L, name).argtypes = [vp] * 7
            L.pcreg_dev_ndt_refit_f32.argtypes = [vp, vp, i, i, vp, i, i, d, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
            L.pcreg_ndt_refit_f32.argtypes = [vp, vp, i, i, vp, i, i, d, i, vp, vp, vp, vp]
        for name, args in (("pcreg_debug_knn_stats", [C.POINTER(C.c_longlong), C.c_int]),
                           ("pcreg_debug_knn_unit_stats", [C.POINTER(C.c_longlong), C.c_int]),
                           ("pcreg_debug_knn_direct_stats", [C.POINTER(C.c_longlong), C.c_int]),
                           ("pcreg_debug_ransac_stats", [C.POINTER(C.c_longlong), C.c_int]),
                           ("pcreg_debug_ransac_handover", [C.POINTER(C.c_longlong), C.c_int]),
                           ("pcreg_debug_desc_stats", [C.POINTER(C.c_longlong), C.c_int]),
                           ("pcreg_debug_dev_model_export", [C.c_void_p] * 4 + [C.POINTER(C.c_float), C.c_void_p]),
                           ("pcreg_debug_search_export", [C.c_void_p, C.c_size_t, C.c_int, C.c_int] + [C.c_void_p] * 3)):
            if hasattr(L, name):             # (an older build given through PCREG_LIB lacks the test hooks)
                getattr(L, name).argtypes = args
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != PCREG_OK:
        raise PcregError(rc, lib().pcreg_last_error().decode(errors="replace"))
