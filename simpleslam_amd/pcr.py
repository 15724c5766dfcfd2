"""Host-side mirror of the reference's registration plugin over the C ABI.

Reference interface (compiled C++): PCR::PointCloudRegister with
``bool scan2Map(const PC_cPtr& src, const PC_cPtr& dst, pose_t& res)`` and
``scalar_t getFitnessScore()`` (reference PCR/include/PCR/PointCloudRegister.hpp:12-38),
implemented by LoamRegister / NdtRegister / VgicpRegister and selected by the config
key ``frontend.pcr`` (reference frontend/src/LidarOdometry.cpp:44-54).  The classes
below keep those names and meanings; every call goes through libpcr_hip.so
(include/pcr_hip.h) -- there is no CPU fallback: if the HIP library or a GPU is
missing, construction raises.

Clouds are float32 arrays of shape (n, 4) [x y z intensity] or (n, 8)
(pcl::PointXYZI layout), either numpy (host) or torch tensors resident in HBM.
Poses are 4x4 float64 numpy arrays (map <- lidar).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PCR_LIB (read HERE, by the Python loader -- the library itself reads no environment variable): another build of the library to load instead of the
# product, e.g. a variant ab/lib<tag>.so under A/B.  The A/B scripts set it; nothing overwrites lib/libpcr_hip.so.
LIB_PATH = os.environ.get("PCR_LIB") or os.path.join(_HERE, "lib", "libpcr_hip.so")


class PcrParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32),
        ("loam_iters", C.c_int32), ("loam_early_exit", C.c_int32),
        ("loam_knn_max_sq", C.c_double), ("loam_plane_thresh", C.c_double), ("loam_point_thresh", C.c_double),
        ("loam_pos_conv", C.c_double), ("loam_rot_conv", C.c_double),
        ("ndt_resolution", C.c_double), ("ndt_step_size", C.c_double), ("ndt_outlier_ratio", C.c_double),
        ("ndt_trans_eps", C.c_double), ("ndt_max_iters", C.c_int32), ("ndt_min_points", C.c_int32),
        ("ndt_search", C.c_int32),
        ("vgicp_resolution", C.c_double), ("vgicp_k_corr", C.c_int32), ("vgicp_max_iters", C.c_int32),
        ("vgicp_lm_inner", C.c_int32), ("vgicp_rot_eps", C.c_double), ("vgicp_trans_eps", C.c_double),
        ("vgicp_lm_init_scale", C.c_double), ("vgicp_search", C.c_int32),
        ("record_trace", C.c_int32),
        ("index_no_hints", C.c_int32), ("ndt_evaluate_repeats", C.c_int32), ("loam_disable_cache", C.c_int32), ("record_timeline", C.c_int32),
        ("loam_coresident", C.c_int32), ("loam_clamp_margin_mm", C.c_int32), ("full_target", C.c_int32), ("host_optimiser", C.c_int32),
        ("host_copy_xyz", C.c_int32), ("query_index", C.c_int32),
        ("liorf_iters", C.c_int32), ("liorf_file_row", C.c_int32), ("liorf_knn_max_sq", C.c_double), ("liorf_plane_thresh", C.c_double), ("liorf_point_thresh", C.c_double),
        ("liorf_min_rows", C.c_int32), ("liorf_min_scan", C.c_int32), ("liorf_rot_conv_deg", C.c_double), ("liorf_trans_conv_cm", C.c_double),
        ("liorf_degenerate_eig", C.c_double),
        ("gicp_max_corr_dist", C.c_double),
        ("vgicp_regularization", C.c_int32), ("vgicp_voxel_mode", C.c_int32),
    ]


# pcr_params.vgicp_regularization / vgicp_voxel_mode (include/pcr_hip.h: PCR_REG_*, PCR_VOXEL_*; fast_gicp's gicp_settings.hpp:6,10)
REG_NONE, REG_MIN_EIG, REG_NORMALIZED_MIN_EIG, REG_PLANE, REG_FROBENIUS = range(5)
VOXEL_ADDITIVE, VOXEL_ADDITIVE_WEIGHTED, VOXEL_MULTIPLICATIVE = range(3)
# pcr_params.vgicp_search (include/pcr_hip.h: PCR_VGICP_*; fast_gicp::NeighborSearchMethod, gicp_settings.hpp:8).  VGICP_DIRECT_RADIUS is refused.
VGICP_DIRECT27, VGICP_DIRECT7, VGICP_DIRECT1, VGICP_DIRECT_RADIUS = range(4)
# pcr_params.ndt_search (include/pcr_hip.h: PCR_NDT_*; pclomp::NeighborSearchMethod, ndt_omp.h:52-57).  NDT_KDTREE is refused.
NDT_KDTREE, NDT_DIRECT26, NDT_DIRECT7, NDT_DIRECT1 = range(4)
# pcr_params.query_index (include/pcr_hip.h: PCR_QUERY_INDEX_*), and the kinds queryIndexInfo() reports
QUERY_INDEX_AUTO, QUERY_INDEX_SPARSE = 0, 1
QUERY_INDEX_DENSE = 0


class PcrStats(C.Structure):
    _fields_ = [
        ("total_ms", C.c_double), ("index_ms", C.c_double), ("solve_ms", C.c_double), ("kernel_ms", C.c_double),
        ("kernel_launches", C.c_int32), ("iterations", C.c_int32), ("n_src", C.c_int64), ("n_dst", C.c_int64),
        ("attempts", C.c_int32), ("target_builds", C.c_int32), ("region_repeats", C.c_int32), ("region_index", C.c_int32),
        ("aux_kernel_ms", C.c_double), ("region_points", C.c_int64), ("region_voxels", C.c_int64), ("pairs_grad", C.c_int64), ("pairs_hess", C.c_int64),
        ("index_box_hint", C.c_int32), ("index_layout_hint", C.c_int32),
    ]


# every symbol include/pcr_hip.h declares
ABI_SYMBOLS = [
    "pcr_default_params", "pcr_create", "pcr_destroy", "pcr_last_error", "pcr_scan2map", "pcr_scan2map_device", "pcr_host_pin", "pcr_host_unpin",
    "pcr_set_target", "pcr_align", "pcr_invalidate_target", "pcr_fitness", "pcr_loam_linearize", "pcr_get_trace", "pcr_get_trace_counts",
    "pcr_vgicp_covariances", "pcr_vgicp_neighbours", "pcr_vgicp_linearize", "pcr_gicp_linearize", "pcr_voxel_filter", "pcr_voxel_filter_begin", "pcr_voxel_filter_end", "pcr_get_timeline", "pcr_ndt_derivatives", "pcr_ndt_voxels", "pcr_vgicp_voxels", "pcr_vgicp_correspondences", "pcr_ndt_pass_sums", "pcr_get_stats", "pcr_set_profile", "pcr_set_stream", "pcr_set_query_tile", "pcr_comm_unique_id", "pcr_comm_init", "pcr_comm_info", "pcr_comm_peer_export", "pcr_comm_init_peer",
    "pcr_comm_init_host", "pcr_set_shard", "pcr_set_params", "pcr_get_params", "pcr_fitness_gated",
    "pcr_map_create", "pcr_map_destroy", "pcr_map_last_error", "pcr_map_add_keyframe", "pcr_map_keyframes", "pcr_map_clear", "pcr_map_update", "pcr_map_update_begin", "pcr_map_wait", "pcr_map_update_window", "pcr_map_submap",
    "pcr_map_submap_indices", "pcr_map_generation", "pcr_scan2map_submap",
    "pcr_map_set_poses", "pcr_map_keyframe", "pcr_map_read_keyframe", "pcr_map_downsample_keyframes", "pcr_map_update_all", "pcr_map_view",
    "pcr_ndt_opt_create", "pcr_ndt_opt_destroy", "pcr_ndt_opt_request", "pcr_ndt_opt_feed", "pcr_ndt_opt_result", "pcr_ndt_opt_counts",
    "pcr_ndt_opt_create_device", "pcr_ndt_opt_set_replay", "pcr_ndt_opt_state", "pcr_ndt_opt_tables", "pcr_ndt_opt_hessian",
    "pcr_vgicp_opt_create", "pcr_vgicp_opt_destroy", "pcr_vgicp_opt_request", "pcr_vgicp_opt_feed", "pcr_vgicp_opt_result",
    "pcr_sc_default_params", "pcr_sc_create", "pcr_sc_destroy", "pcr_sc_last_error", "pcr_sc_size", "pcr_sc_add", "pcr_sc_descriptor", "pcr_sc_distance",
    "pcr_sc_query", "pcr_knn", "pcr_radius_search", "pcr_query_index_info", "pcr_fitness_batch", "pcr_reloc_default_params", "pcr_reloc_hypotheses", "pcr_relocalize",
    "pcr_sc_distances", "pcr_global_reloc_default_params", "pcr_global_reloc_hypotheses", "pcr_relocalize_global",
    "pcr_sc_rank_stored", "pcr_sc_shift_yaw", "pcr_sc_add_keyframes",
    "pcr_liorf_pose_to_6dof", "pcr_liorf_6dof_to_pose", "pcr_liorf_linearize", "pcr_liorf_result",
    "pcr_pose_to_mobile", "pcr_frontend_default_params", "pcr_frontend_create", "pcr_frontend_destroy", "pcr_frontend_last_error", "pcr_frontend_step",
    "pcr_frontend_prefetch", "pcr_frontend_finish", "pcr_frontend_reset",
    "pcr_graph_create", "pcr_graph_destroy", "pcr_graph_last_error", "pcr_graph_noise", "pcr_graph_add_poses", "pcr_graph_add_prior", "pcr_graph_add_between",
    "pcr_graph_add_between_poses", "pcr_graph_size", "pcr_graph_clear", "pcr_graph_default_params", "pcr_graph_optimize", "pcr_graph_poses",
    "pcr_graph_device_poses", "pcr_graph_linearize", "pcr_graph_apply", "pcr_map_set_poses_from_graph", "pcr_graph_load_g2o", "pcr_graph_save_g2o",
    "pcr_graph_tree", "pcr_graph_precondition", "pcr_graph_set_robust_kernel", "pcr_graph_get_robust_kernel", "pcr_graph_set_between_robust",
    "pcr_graph_set_between_enabled", "pcr_graph_add_loop", "pcr_graph_between_weights", "pcr_graph_robust_rho_w",
    "pcr_graph_set_fixed", "pcr_graph_fixed",
    "pcr_voxel_sparse_default_params", "pcr_voxel_filter_sparse", "pcr_voxel_sparse_order", "pcr_map_update_all_sparse",
    "pcr_kf_rank_near_host", "pcr_map_rank_near", "pcr_frontend_closest",
    "pcr_backend_default_params", "pcr_backend_create", "pcr_backend_destroy", "pcr_backend_last_error", "pcr_backend_graph", "pcr_backend_sc",
    "pcr_backend_register", "pcr_backend_add_keyframes", "pcr_backend_close_loops", "pcr_backend_loops", "pcr_backend_step", "pcr_backend_reset",
    "pcr_session_last_error", "pcr_tum_format", "pcr_tum_parse", "pcr_pcd_write", "pcr_pcd_read", "pcr_map_save", "pcr_map_load",
    "pcr_backend_set_save_dir", "pcr_backend_save", "pcr_backend_load", "pcr_backend_load_seconds",
    "pcr_deskew", "pcr_deskew_host", "pcr_frontend_step_timed",
]

# pcr_allreduce_fn (include/pcr_hip.h): int fn(double* inout, size_t count, int op, void* user)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_size_t, C.c_int, C.c_void_p)


# pcr_voxel_sparse_params.kind (include/pcr_hip.h: PCR_VOXEL_SPARSE_*)
VOXEL_SPARSE_V3, VOXEL_SPARSE_V2 = 3, 2


class VoxelSparseParams(C.Structure):
    """pcr_voxel_sparse_params (include/pcr_hip.h)"""
    _fields_ = [("kind", C.c_int32), ("max_voxel_pts", C.c_int32), ("min_voxel_pts", C.c_int32)]


class ScParams(C.Structure):
    """struct pcr_sc_params (include/pcr_hip.h)."""
    _fields_ = [("lidar_height", C.c_double), ("num_exclude_recent", C.c_int32), ("build_tree_gap", C.c_int32), ("num_candidates", C.c_int32),
                ("pad", C.c_int32), ("search_ratio", C.c_double), ("dist_thres", C.c_double)]


class RelocParams(C.Structure):
    """struct pcr_reloc_params (include/pcr_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("xy_range", C.c_double), ("xy_step", C.c_double), ("yaw_range", C.c_double),
                ("yaw_step", C.c_double), ("max_sq", C.c_double), ("refine_top", C.c_int32), ("pad_", C.c_int32), ("score_points", C.c_uint64)]


class RelocCandidate(C.Structure):
    """struct pcr_reloc_candidate (include/pcr_hip.h)."""
    _fields_ = [("hypothesis", C.c_int64), ("coarse_n_in", C.c_int64), ("coarse_score", C.c_double), ("pose", C.c_double * 16),
                ("converged", C.c_int32), ("pad_", C.c_int32), ("n_in", C.c_int64), ("score", C.c_double)]


class GlobalRelocParams(C.Structure):
    """struct pcr_global_reloc_params (include/pcr_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("places", C.c_int32), ("max_dist", C.c_double), ("local", RelocParams)]


# pcr_deskew's time_kind (include/pcr_hip.h: PCR_TIME_*) and the numpy type of its element
TIME_F32_SECONDS, TIME_U32_NANOSECONDS, TIME_F64_SECONDS = 0, 1, 2
_TIME_DTYPES = {TIME_F32_SECONDS: np.float32, TIME_U32_NANOSECONDS: np.uint32, TIME_F64_SECONDS: np.float64}


class DeskewMotion(C.Structure):
    """struct pcr_deskew_motion (include/pcr_hip.h)."""
    _fields_ = [("poses", C.POINTER(C.c_double)), ("stamps", C.POINTER(C.c_double)), ("K", C.c_size_t), ("t0", C.c_double), ("t_ref", C.c_double)]


class DeskewInfo(C.Structure):
    """struct pcr_deskew_info (include/pcr_hip.h)."""
    _fields_ = [("before", C.c_int64), ("after", C.c_int64), ("nonfinite", C.c_int64), ("ref_clamped", C.c_int32)]


class FrontendParams(C.Structure):
    """struct pcr_frontend_params (include/pcr_hip.h)."""
    _fields_ = [("grid_size", C.c_double), ("radius", C.c_double), ("kf_gap", C.c_double), ("mobile", C.c_int32)]


class FrontendInfo(C.Structure):
    """struct pcr_frontend_info (include/pcr_hip.h)."""
    _fields_ = [("registered", C.c_int32), ("converged", C.c_int32), ("iterations", C.c_int32), ("keyframe_added", C.c_int32), ("update_queued", C.c_int32),
                ("n_filtered", C.c_int64), ("n_submap", C.c_int64), ("keyframes", C.c_int64), ("updates", C.c_int64), ("seconds", C.c_double * 5)]


class GraphParams(C.Structure):
    """struct pcr_graph_params (include/pcr_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("max_iterations", C.c_int32), ("rel_tol", C.c_double), ("abs_tol", C.c_double), ("lambda_init", C.c_double),
                ("lambda_factor", C.c_double), ("lambda_max", C.c_double), ("pcg_max_iterations", C.c_int64), ("pcg_rel_tol", C.c_double), ("pcg_preconditioner", C.c_int32)]


class GraphResult(C.Structure):
    """struct pcr_graph_result (include/pcr_hip.h)."""
    _fields_ = [("iterations", C.c_int32), ("accepted", C.c_int32), ("pcg_iterations", C.c_int64), ("pcg_capped", C.c_int32), ("converged", C.c_int32),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_", C.c_double), ("delta", C.c_double * 16)]


class BackendParams(C.Structure):
    """struct pcr_backend_params (include/pcr_hip.h)."""
    _fields_ = [("grid_size", C.c_double), ("context_grid_size", C.c_double), ("history_range", C.c_int32), ("fitness_threshold", C.c_double),
                ("detectors", C.c_int32), ("dist_radius", C.c_double), ("dist_exclude_recent", C.c_int32), ("lc_method", C.c_int32),
                ("lc_between_refined", C.c_int32), ("sc", ScParams), ("graph", GraphParams)]


class BackendLoop(C.Structure):
    """struct pcr_backend_loop (include/pcr_hip.h)."""
    _fields_ = [("cur", C.c_int64), ("old", C.c_int64), ("detector", C.c_int32), ("converged", C.c_int32), ("iterations", C.c_int32),
                ("accepted", C.c_int32), ("fitness", C.c_double), ("pose", C.c_double * 16)]


class BackendInfo(C.Structure):
    """struct pcr_backend_info (include/pcr_hip.h)."""
    _fields_ = [("keyframes", C.c_int64), ("contexts", C.c_int64), ("keyframes_added", C.c_int32), ("candidates", C.c_int32), ("accepted", C.c_int32),
                ("factors_added", C.c_int32), ("optimized", C.c_int32), ("pad_", C.c_int32), ("graph", GraphResult), ("delta", C.c_double * 16),
                ("seconds", C.c_double * 9)]


class GlobalRelocCandidate(C.Structure):
    """struct pcr_global_reloc_candidate (include/pcr_hip.h)."""
    _fields_ = [("place", C.c_int64), ("sc_dist", C.c_double), ("sc_shift", C.c_int32), ("pad_", C.c_int32), ("c", RelocCandidate)]


_lib = None


def load_library():
    """dlopen libpcr_hip.so and declare the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C simpleslam_amd/csrc`). "
            "There is no CPU fallback.")
    try:
        # torch ships its own libamdhip64 under the same soname: whichever HIP runtime is mapped first serves the whole
        # process, and torch.cuda reports "No HIP GPUs" when that is not its own.  Map torch's first when it is installed.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.pcr_default_params.argtypes = [C.POINTER(PcrParams)]
    L.pcr_default_params.restype = None
    L.pcr_create.argtypes = [C.c_char_p, C.POINTER(PcrParams)]
    L.pcr_create.restype = vp
    L.pcr_destroy.argtypes = [vp]
    L.pcr_destroy.restype = None
    L.pcr_last_error.argtypes = [vp]
    L.pcr_last_error.restype = C.c_char_p
    L.pcr_scan2map.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, dp, ip]
    L.pcr_scan2map_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, dp, ip]
    L.pcr_host_pin.argtypes = [vp, C.c_size_t]
    L.pcr_host_unpin.argtypes = [vp]
    L.pcr_set_target.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int]
    L.pcr_align.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp, ip]
    L.pcr_invalidate_target.argtypes = [vp]
    L.pcr_fitness.argtypes = [vp]
    L.pcr_fitness.restype = C.c_double
    L.pcr_loam_linearize.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp, dp, dp, C.POINTER(C.c_int64), vp, vp, vp]
    L.pcr_get_trace.argtypes = [vp, C.POINTER(C.c_int32), vp, vp, vp, vp]
    L.pcr_get_trace_counts.argtypes = [vp, vp, vp]
    L.pcr_vgicp_covariances.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp]
    L.pcr_vgicp_neighbours.argtypes = [vp, C.c_size_t, vp, vp]
    L.pcr_vgicp_linearize.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp, dp, dp, dp, C.POINTER(C.c_int64)]
    L.pcr_gicp_linearize.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_int64), vp, vp, vp]
    L.pcr_ndt_derivatives.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp, dp, dp, dp, dp]
    L.pcr_get_timeline.argtypes = [vp, vp, C.c_size_t, ip, ip]
    L.pcr_ndt_voxels.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    fp = C.POINTER(C.c_float)
    L.pcr_liorf_pose_to_6dof.argtypes = [dp, fp]
    L.pcr_liorf_6dof_to_pose.argtypes = [fp, dp]
    L.pcr_liorf_linearize.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, fp, fp, vp, vp, dp, dp, C.POINTER(C.c_int64)]
    L.pcr_liorf_result.argtypes = [vp, fp, ip, C.POINTER(C.c_int64)]
    L.pcr_vgicp_voxels.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.pcr_vgicp_correspondences.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.pcr_ndt_pass_sums.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp, C.c_int, dp, dp, dp]
    L.pcr_voxel_filter.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_double, vp, C.c_size_t, C.c_int, C.POINTER(C.c_size_t)]
    L.pcr_voxel_filter_begin.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_double, vp, C.c_size_t]
    L.pcr_voxel_filter_end.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.pcr_voxel_sparse_default_params.argtypes = [C.POINTER(VoxelSparseParams)]
    L.pcr_voxel_sparse_default_params.restype = None
    L.pcr_voxel_filter_sparse.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.POINTER(VoxelSparseParams), vp, C.c_size_t, C.c_int,
                                          C.POINTER(C.c_size_t)]
    L.pcr_voxel_sparse_order.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.pcr_map_update_all_sparse.argtypes = [vp, C.c_double, C.POINTER(C.c_size_t)]
    L.pcr_get_stats.argtypes = [vp, C.POINTER(PcrStats)]
    L.pcr_scan2map_submap.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, dp, ip]
    L.pcr_ndt_opt_create.restype = vp
    L.pcr_ndt_opt_create.argtypes = [dp, C.c_double, C.c_double, C.c_int]
    L.pcr_ndt_opt_destroy.restype = None
    L.pcr_ndt_opt_destroy.argtypes = [vp]
    L.pcr_ndt_opt_request.argtypes = [vp, ip, dp, dp]
    L.pcr_ndt_opt_feed.argtypes = [vp, dp]
    L.pcr_ndt_opt_result.argtypes = [vp, dp, ip, ip, ip]
    L.pcr_ndt_opt_counts.argtypes = [vp, ip, ip, ip]
    L.pcr_ndt_opt_create_device.restype = vp
    L.pcr_ndt_opt_create_device.argtypes = [dp, C.c_double, C.c_double, C.c_int]
    L.pcr_ndt_opt_set_replay.argtypes = [vp, C.c_int]
    L.pcr_ndt_opt_state.argtypes = [vp, ip, ip, dp, ip]
    L.pcr_ndt_opt_tables.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), dp, dp]
    L.pcr_ndt_opt_hessian.argtypes = [vp, dp]
    L.pcr_vgicp_opt_create.restype = vp
    L.pcr_vgicp_opt_create.argtypes = [dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    L.pcr_vgicp_opt_destroy.restype = None
    L.pcr_vgicp_opt_destroy.argtypes = [vp]
    L.pcr_vgicp_opt_request.argtypes = [vp, ip, dp, dp]
    L.pcr_vgicp_opt_feed.argtypes = [vp, dp]
    L.pcr_vgicp_opt_result.argtypes = [vp, dp, ip, ip, ip]
    L.pcr_map_generation.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.pcr_set_profile.argtypes = [vp, C.c_int]
    L.pcr_set_stream.argtypes = [vp, vp]
    L.pcr_set_query_tile.argtypes = [vp, dp, dp]
    L.pcr_comm_unique_id.argtypes = [vp]
    L.pcr_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
    L.pcr_comm_peer_export.argtypes = [vp, vp]
    L.pcr_comm_init_peer.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    L.pcr_comm_init_host.argtypes = [vp, ALLREDUCE_FN, vp, C.c_int, C.c_int]
    L.pcr_comm_info.argtypes = [vp, ip, ip, ip]
    L.pcr_set_shard.argtypes = [vp, dp, dp, C.c_double]
    L.pcr_set_params.argtypes = [vp, C.POINTER(PcrParams)]
    L.pcr_get_params.argtypes = [vp, C.POINTER(PcrParams)]
    L.pcr_fitness_gated.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp, C.c_double, dp, C.POINTER(C.c_int64)]
    L.pcr_map_create.argtypes = [C.c_int]
    L.pcr_map_create.restype = vp
    L.pcr_map_destroy.argtypes = [vp]
    L.pcr_map_destroy.restype = None
    L.pcr_map_last_error.argtypes = [vp]
    L.pcr_map_last_error.restype = C.c_char_p
    L.pcr_map_add_keyframe.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp]
    L.pcr_map_keyframes.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.pcr_map_clear.argtypes = [vp]
    L.pcr_map_update.argtypes = [vp, dp, C.c_double, C.c_double, C.POINTER(C.c_size_t)]
    L.pcr_map_update_begin.argtypes = [vp, dp, C.c_double, C.c_double]
    L.pcr_map_wait.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.pcr_map_update_window.argtypes = [vp, C.c_longlong, C.c_int, C.c_double, C.POINTER(C.c_size_t)]
    L.pcr_map_submap.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.pcr_map_submap.restype = vp
    L.pcr_map_submap_indices.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.pcr_map_set_poses.argtypes = [vp, C.c_size_t, C.c_size_t, dp]
    L.pcr_map_keyframe.argtypes = [vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), dp]
    L.pcr_map_keyframe.restype = vp
    L.pcr_map_read_keyframe.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), dp]
    L.pcr_map_downsample_keyframes.argtypes = [vp, C.c_size_t, C.c_double, C.POINTER(C.c_size_t)]
    L.pcr_map_update_all.argtypes = [vp, C.c_double, C.POINTER(C.c_size_t)]
    L.pcr_map_view.argtypes = [vp]
    L.pcr_map_view.restype = vp
    L.pcr_sc_default_params.argtypes = [C.POINTER(ScParams)]
    L.pcr_sc_default_params.restype = None
    L.pcr_sc_create.argtypes = [C.c_int, C.POINTER(ScParams)]
    L.pcr_sc_create.restype = vp
    L.pcr_sc_destroy.argtypes = [vp]
    L.pcr_sc_destroy.restype = None
    L.pcr_sc_last_error.argtypes = [vp]
    L.pcr_sc_last_error.restype = C.c_char_p
    L.pcr_sc_size.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.pcr_sc_add.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int]
    L.pcr_sc_add_keyframes.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(C.c_size_t)]
    L.pcr_sc_descriptor.argtypes = [vp, C.c_size_t, vp, vp, vp]
    L.pcr_sc_distance.argtypes = [vp, C.c_size_t, C.c_size_t, dp, ip]
    L.pcr_sc_query.argtypes = [vp, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_float), dp]
    L.pcr_knn.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int64), dp]
    L.pcr_radius_search.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), dp,
                                    C.POINTER(C.c_size_t)]
    L.pcr_query_index_info.argtypes = [vp, ip, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.pcr_fitness_batch.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp, C.c_size_t, C.c_double, C.c_size_t, dp, C.POINTER(C.c_int64)]
    L.pcr_reloc_default_params.argtypes = [C.POINTER(RelocParams)]
    L.pcr_reloc_default_params.restype = None
    L.pcr_reloc_hypotheses.argtypes = [dp, C.POINTER(RelocParams), dp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.pcr_relocalize.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(RelocParams), dp, ip, C.POINTER(RelocCandidate), C.c_size_t,
                                 C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.pcr_sc_distances.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp, C.POINTER(C.c_int32)]
    L.pcr_sc_rank_stored.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_int64), dp, C.POINTER(C.c_int32)]
    L.pcr_sc_shift_yaw.argtypes = [C.c_int32]
    L.pcr_sc_shift_yaw.restype = C.c_float
    L.pcr_global_reloc_default_params.argtypes = [C.POINTER(GlobalRelocParams)]
    L.pcr_global_reloc_default_params.restype = None
    L.pcr_global_reloc_hypotheses.argtypes = [dp, C.c_int32, C.POINTER(RelocParams), dp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.pcr_relocalize_global.argtypes = [vp, vp, dp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(GlobalRelocParams), dp, ip,
                                        C.POINTER(GlobalRelocCandidate), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.pcr_pose_to_mobile.argtypes = [dp, dp]
    L.pcr_frontend_default_params.argtypes = [C.POINTER(FrontendParams)]
    L.pcr_frontend_default_params.restype = None
    L.pcr_frontend_create.argtypes = [vp, vp, C.POINTER(FrontendParams)]
    L.pcr_frontend_create.restype = vp
    L.pcr_frontend_destroy.argtypes = [vp]
    L.pcr_frontend_destroy.restype = None
    L.pcr_frontend_last_error.argtypes = [vp]
    L.pcr_frontend_last_error.restype = C.c_char_p
    L.pcr_frontend_step.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, dp, dp, C.POINTER(FrontendInfo)]
    L.pcr_frontend_prefetch.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int]
    L.pcr_frontend_finish.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.pcr_frontend_reset.argtypes = [vp]
    L.pcr_graph_create.argtypes = [C.c_int]
    L.pcr_graph_create.restype = vp
    L.pcr_graph_destroy.argtypes = [vp]
    L.pcr_graph_destroy.restype = None
    L.pcr_graph_last_error.argtypes = [vp]
    L.pcr_graph_last_error.restype = C.c_char_p
    L.pcr_graph_noise.argtypes = [C.c_int, dp]
    L.pcr_graph_add_poses.argtypes = [vp, dp, C.c_size_t]
    L.pcr_graph_add_prior.argtypes = [vp, C.c_size_t, dp, dp]
    L.pcr_graph_add_between.argtypes = [vp, C.c_size_t, C.c_size_t, dp, dp]
    L.pcr_graph_add_between_poses.argtypes = [vp, C.c_size_t, C.c_size_t, dp]
    L.pcr_graph_size.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.pcr_graph_clear.argtypes = [vp]
    L.pcr_graph_default_params.argtypes = [C.POINTER(GraphParams)]
    L.pcr_graph_default_params.restype = None
    L.pcr_graph_optimize.argtypes = [vp, C.POINTER(GraphParams), C.POINTER(GraphResult)]
    L.pcr_graph_poses.argtypes = [vp, C.c_size_t, C.c_size_t, dp]
    L.pcr_graph_device_poses.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.pcr_graph_device_poses.restype = vp
    L.pcr_graph_linearize.argtypes = [vp, dp, dp, dp, dp]
    L.pcr_graph_apply.argtypes = [vp, C.c_double, dp, dp]
    L.pcr_graph_tree.argtypes = [vp, C.POINTER(C.c_int64), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.pcr_graph_precondition.argtypes = [vp, C.c_double, C.c_int, dp, dp]
    L.pcr_map_set_poses_from_graph.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.pcr_graph_set_robust_kernel.argtypes = [vp, C.c_int, C.c_double]
    L.pcr_graph_get_robust_kernel.argtypes = [vp, C.POINTER(C.c_int), dp]
    L.pcr_graph_set_between_robust.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
    L.pcr_graph_set_between_enabled.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
    L.pcr_graph_add_loop.argtypes = [vp, C.c_size_t, C.c_size_t, dp, dp]
    L.pcr_graph_between_weights.argtypes = [vp, C.c_size_t, C.c_size_t, dp, dp, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]
    L.pcr_graph_robust_rho_w.argtypes = [C.c_int, C.c_double, C.c_double, dp, dp]
    L.pcr_graph_set_fixed.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
    L.pcr_graph_fixed.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8)]
    L.pcr_graph_load_g2o.argtypes = [vp, C.c_char_p]
    L.pcr_graph_save_g2o.argtypes = [vp, C.c_char_p]
    i64p = C.POINTER(C.c_int64)
    L.pcr_kf_rank_near_host.argtypes = [dp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_int, i64p, dp]
    L.pcr_map_rank_near.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_int, i64p, dp]
    L.pcr_frontend_closest.argtypes = [vp, i64p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.pcr_backend_default_params.argtypes = [C.POINTER(BackendParams)]
    L.pcr_backend_default_params.restype = None
    L.pcr_backend_create.argtypes = [vp, C.POINTER(BackendParams)]
    L.pcr_backend_create.restype = vp
    L.pcr_backend_destroy.argtypes = [vp]
    L.pcr_backend_destroy.restype = None
    L.pcr_backend_last_error.argtypes = [vp]
    L.pcr_backend_last_error.restype = C.c_char_p
    for name in ("pcr_backend_graph", "pcr_backend_sc", "pcr_backend_register"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = vp
    L.pcr_backend_add_keyframes.argtypes = [vp, i64p, C.c_size_t, C.POINTER(BackendInfo)]
    L.pcr_backend_close_loops.argtypes = [vp, C.POINTER(BackendInfo)]
    L.pcr_backend_loops.argtypes = [vp, C.POINTER(BackendLoop), C.c_size_t, C.POINTER(C.c_size_t)]
    L.pcr_backend_step.argtypes = [vp, i64p, C.c_size_t, C.POINTER(BackendInfo), C.POINTER(BackendInfo)]
    L.pcr_backend_reset.argtypes = [vp]
    L.pcr_session_last_error.argtypes = []
    L.pcr_session_last_error.restype = C.c_char_p
    L.pcr_tum_format.argtypes = [C.c_double, dp, C.c_int, C.c_char_p, C.c_size_t]
    L.pcr_tum_parse.argtypes = [C.c_char_p, dp, dp]
    L.pcr_pcd_write.argtypes = [C.c_char_p, vp, C.c_size_t, C.c_size_t]
    L.pcr_pcd_read.argtypes = [C.c_char_p, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]
    L.pcr_map_save.argtypes = [vp, C.c_char_p, C.c_size_t, dp, C.c_int]
    L.pcr_map_load.argtypes = [vp, C.c_char_p, C.c_double, dp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.pcr_backend_set_save_dir.argtypes = [vp, C.c_char_p]
    L.pcr_backend_save.argtypes = [vp, dp, C.c_int]
    L.pcr_backend_load.argtypes = [vp, C.c_char_p, dp, C.c_size_t, C.POINTER(BackendInfo)]
    L.pcr_backend_load_seconds.argtypes = [vp, dp]
    L.pcr_deskew.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_int, C.c_longlong, C.POINTER(DeskewMotion), vp, C.c_int, C.POINTER(DeskewInfo)]
    L.pcr_deskew_host.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_int, C.c_longlong, C.POINTER(DeskewMotion), vp, C.POINTER(DeskewInfo)]
    L.pcr_frontend_step_timed.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_int, C.c_longlong, C.POINTER(DeskewMotion), dp, dp,
                                          C.POINTER(FrontendInfo), C.POINTER(DeskewInfo)]
    _lib = L
    return L


def default_params(**overrides):
    p = PcrParams()
    load_library().pcr_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"pcr_params has no field {k!r}")
        setattr(p, k, v)
    return p


class PcrError(RuntimeError):
    pass


def reloc_params(**overrides):
    """pcr_reloc_default_params with fields overridden (xy_range, xy_step, yaw_range, yaw_step in radians, max_sq, refine_top, score_points)."""
    p = RelocParams()
    load_library().pcr_reloc_default_params(C.byref(p))
    for k, v in overrides.items():
        if k not in ("xy_range", "xy_step", "yaw_range", "yaw_step", "max_sq", "refine_top", "score_points"):
            raise AttributeError(f"pcr_reloc_params has no field {k!r}")
        setattr(p, k, v)
    return p


def reloc_hypotheses(coarse, **params):
    """pcr_reloc_hypotheses: the (K, 4, 4) lattice of poses around `coarse` (yaw outermost, then y, then x; include/pcr_hip.h)."""
    L = load_library()
    p = reloc_params(**params)
    c = _pose_in(coarse)
    dp = C.POINTER(C.c_double)
    K = C.c_size_t(0)
    rc = L.pcr_reloc_hypotheses(c.ctypes.data_as(dp), C.byref(p), None, 0, C.byref(K))
    if rc != 0 and K.value == 0:
        raise PcrError(L.pcr_last_error(None).decode())
    out = np.zeros((K.value, 16))
    if L.pcr_reloc_hypotheses(c.ctypes.data_as(dp), C.byref(p), out.ctypes.data_as(dp), K.value, C.byref(K)) != 0:
        raise PcrError(L.pcr_last_error(None).decode())
    return out.reshape(-1, 4, 4).transpose(0, 2, 1).copy()


_LOCAL_FIELDS = ("xy_range", "xy_step", "yaw_range", "yaw_step", "max_sq", "refine_top", "score_points")


def global_reloc_params(**overrides):
    """pcr_global_reloc_default_params with fields overridden: places, max_dist, and the fields of the per-place lattice (pcr_reloc_params:
    xy_range, xy_step, yaw_range, yaw_step in radians, max_sq, refine_top, score_points)."""
    p = GlobalRelocParams()
    load_library().pcr_global_reloc_default_params(C.byref(p))
    for k, v in overrides.items():
        if k in ("places", "max_dist"):
            setattr(p, k, v)
        elif k in _LOCAL_FIELDS:
            setattr(p.local, k, v)
        else:
            raise AttributeError(f"pcr_global_reloc_params has no field {k!r}")
    return p


def global_reloc_hypotheses(kf_pose, shift, **local):
    """pcr_global_reloc_hypotheses: the (K, 4, 4) lattice around the coarse pose of a place, kf_pose * Rz(-yaw) with yaw the float
    deg2rad(6 * shift) of pcr_sc_query.  local: fields of the per-place lattice (default: global_reloc_params().local)."""
    L = load_library()
    p = global_reloc_params(**local).local
    c = _pose_in(kf_pose)
    if isinstance(shift, (bool, float)) or not isinstance(shift, (int, np.integer)):
        raise TypeError(f"shift must be an integer, not {type(shift).__name__}")
    dp = C.POINTER(C.c_double)
    K = C.c_size_t(0)
    rc = L.pcr_global_reloc_hypotheses(c.ctypes.data_as(dp), int(shift), C.byref(p), None, 0, C.byref(K))
    if rc != 0 and K.value == 0:
        raise PcrError(L.pcr_last_error(None).decode())
    out = np.zeros((K.value, 16))
    if L.pcr_global_reloc_hypotheses(c.ctypes.data_as(dp), int(shift), C.byref(p), out.ctypes.data_as(dp), K.value, C.byref(K)) != 0:
        raise PcrError(L.pcr_last_error(None).decode())
    return out.reshape(-1, 4, 4).transpose(0, 2, 1).copy()


def _cand_dict(c):
    return dict(hypothesis=c.hypothesis, coarse_n_in=c.coarse_n_in, coarse_score=c.coarse_score, pose=_pose_out(np.array(c.pose[:])),
                converged=bool(c.converged), n_in=c.n_in, score=c.score)


def _cloud(x):
    """-> (pointer, n, stride_bytes, on_device, keepalive)"""
    if isinstance(x, tuple) and len(x) == 3:  # (device pointer, n, stride_bytes): SubMap.pointer() / SubMap.keyFramePointer(i)
        p, n, s = x
        return C.c_void_p(p), int(n), int(s), 1, None
    if hasattr(x, "data_ptr"):  # torch tensor
        import torch
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] < 3 or not x.is_contiguous():
            raise ValueError("cloud tensors must be contiguous float32 of shape (n, >=3)")
        return C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1] * 4, 1 if x.is_cuda else 0, x
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("clouds must have shape (n, >=3)")
    return a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1] * 4, 0, a


def _pose_in(T):
    T = np.asarray(T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("pose must be 4x4")
    return np.ascontiguousarray(T.T).reshape(16).copy()  # column-major


def _pose_out(buf):
    return buf.reshape(4, 4).T.copy()


class PointCloudRegister:
    """PCR::PointCloudRegister (reference PointCloudRegister.hpp:12-38)."""

    method = None

    def __init__(self, params=None, **overrides):
        self._lib = load_library()
        if params is None:
            params = default_params(**overrides)
        elif overrides:
            for k, v in overrides.items():
                setattr(params, k, v)
        self.params = params
        self._h = self._lib.pcr_create(self.method.encode(), C.byref(params))
        if not self._h:
            raise PcrError(self._lib.pcr_last_error(None).decode())
        self.isConverge = False
        # per-call marshalling kept off the hot path (a C++ caller has none): one persistent pose buffer and flag, and the
        # (pointer, size, stride) triple of the most recent device tensors remembered by identity
        self._pose_buf = (C.c_double * 16)()
        self._pose_cm = np.frombuffer(self._pose_buf, dtype=np.float64).reshape(4, 4)     # column-major 4x4 = transposed view
        self._conv = C.c_int(0)
        self._conv_ref = C.byref(self._conv)
        self._seen = {}

    def _cloud_cached(self, x):
        """(pointer, n, stride, on_device, keepalive) of a device tensor, remembered by identity through a WEAK reference (no tensor
        is kept alive by this object) and revalidated on every hit: same storage pointer, shape, strides and dtype."""
        if hasattr(x, "data_ptr"):
            import weakref
            hit = self._seen.get(id(x))
            if hit is not None and hit[0]() is x and hit[2] == (x.data_ptr(), tuple(x.shape), x.stride(), x.dtype):
                return hit[1]
            c = _cloud(x)
            if len(self._seen) > 64:
                self._seen = {k: v for k, v in self._seen.items() if v[0]() is not None}
                if len(self._seen) > 64:
                    self._seen.clear()
            self._seen[id(x)] = (weakref.ref(x), c[:4] + (None,), (x.data_ptr(), tuple(x.shape), x.stride(), x.dtype))
            return c
        return _cloud(x)

    # -- reference interface ------------------------------------------------
    def scan2Map(self, src, dst, res):
        """Refine `res` (4x4, map<-lidar) in place; returns isConverge.
        The target index is rebuilt on every call, like the reference (LoamRegister.cpp:110)."""
        sp, sn, ss, sdev, _k1 = self._cloud_cached(src)
        dp_, dn, ds, ddev, _k2 = self._cloud_cached(dst)
        if ss != ds:
            raise ValueError("src and dst must share a point stride")
        if sdev != ddev:
            raise ValueError("src and dst must both be host arrays or both be device tensors")
        res_np = np.asarray(res)
        if res_np.shape != (4, 4):
            raise ValueError("pose must be 4x4")
        self._pose_cm[...] = res_np.T
        fn = self._lib.pcr_scan2map_device if sdev else self._lib.pcr_scan2map
        self._check(fn(self._h, sp, sn, dp_, dn, ss, self._pose_buf, self._conv_ref))
        res_np[...] = self._pose_cm.T
        self.isConverge = bool(self._conv.value)
        return self.isConverge

    def getFitnessScore(self):
        return float(self._lib.pcr_fitness(self._h))

    # -- static-map localisation (reference test/loc.cpp) ----------------------
    def setTarget(self, dst):
        p, n, s, dev, _k = _cloud(dst)
        self._check(self._lib.pcr_set_target(self._h, p, n, s, dev))

    def align(self, src, res):
        p, n, s, dev, _k = self._cloud_cached(src)
        res_np = np.asarray(res)
        if res_np.shape != (4, 4):
            raise ValueError("pose must be 4x4")
        self._pose_cm[...] = res_np.T
        self._check(self._lib.pcr_align(self._h, p, n, s, dev, self._pose_buf, self._conv_ref))
        res_np[...] = self._pose_cm.T
        self.isConverge = bool(self._conv.value)
        return self.isConverge

    def invalidateTarget(self):
        self._check(self._lib.pcr_invalidate_target(self._h))

    def scan2MapSubmap(self, src, submap, pose, rebuild=False):
        """scan2Map with the device-resident sub-map of a SubMap as `dst` (no host copy of the map).  The handle keeps the target
        structures it builds for as long as the SubMap stays at the same generation (pcr_scan2map_submap); rebuild=True is the
        reference's behaviour of rebuilding on every call (pcr_scan2map_device on the same memory) -- same result either way."""
        p, n, s, dev, _k = _cloud(src)
        dp, dn, ds = submap.pointer()
        if dn and ds != s:
            raise ValueError("scan and sub-map must share one point layout")
        if not dev:
            import torch
            t = torch.from_numpy(np.ascontiguousarray(src, np.float32)).cuda()
            p, _k = C.c_void_p(t.data_ptr()), t
        pc = _pose_in(pose)
        conv = C.c_int(0)
        if rebuild:
            self._check(self._lib.pcr_scan2map_device(self._h, p, n, C.c_void_p(dp), dn, s, pc.ctypes.data_as(C.POINTER(C.c_double)), C.byref(conv)))
        else:
            self._check(self._lib.pcr_scan2map_submap(self._h, p, n, 1, submap._m, pc.ctypes.data_as(C.POINTER(C.c_double)), C.byref(conv)))
        np.asarray(pose)[...] = _pose_out(pc)
        self.isConverge = bool(conv.value)
        return self.isConverge

    # -- the step before the path ------------------------------------------------
    def voxelDownSample(self, cloud, grid_size):
        """pcp::voxelDownSample / pcl::VoxelGrid (reference common/pcp/pcp.hpp:14-28): centroid per occupied voxel, ascending
        voxel index.  Host array in -> numpy array out; CUDA tensor in -> CUDA tensor out (nothing leaves HBM)."""
        p, n, s, dev, keep = _cloud(cloud)
        cnt = C.c_size_t(0)
        if dev:
            import torch
            out = torch.empty((max(n, 1), s // 4), dtype=torch.float32, device=keep.device)
            self._check(self._lib.pcr_voxel_filter(self._h, p, n, s, 1, float(grid_size), C.c_void_p(out.data_ptr()), n, 1, C.byref(cnt)))
            return out[:cnt.value]
        out = np.zeros((max(n, 1), s // 4), np.float32)
        self._check(self._lib.pcr_voxel_filter(self._h, p, n, s, 0, float(grid_size), out.ctypes.data_as(C.c_void_p), n, 0, C.byref(cnt)))
        return out[:cnt.value].copy()

    def _voxel_sparse(self, cloud, grid_size, prm):
        p, n, s, dev, keep = _cloud(cloud)
        cnt = C.c_size_t(0)
        if dev:
            import torch
            out = torch.empty((max(n, 1), s // 4), dtype=torch.float32, device=keep.device)
            self._check(self._lib.pcr_voxel_filter_sparse(self._h, p, n, s, 1, float(grid_size), C.byref(prm), C.c_void_p(out.data_ptr()), n, 1, C.byref(cnt)))
            return out[:cnt.value]
        out = np.zeros((max(n, 1), s // 4), np.float32)
        self._check(self._lib.pcr_voxel_filter_sparse(self._h, p, n, s, 0, float(grid_size), C.byref(prm), out.ctypes.data_as(C.c_void_p), n, 0, C.byref(cnt)))
        return out[:cnt.value].copy()

    def voxelDownSampleV3(self, cloud, grid_size):
        """pcp::VoxelDownSampleV3 (reference common/pcp/pcp.hpp:157-263; pcr_voxel_filter_sparse): pcl::VoxelGrid's lattice without its limit on
        the voxel box -- the centroid per occupied voxel, ascending (z, y, x).  Host array in -> numpy array out; CUDA tensor in -> CUDA tensor out."""
        return self._voxel_sparse(cloud, grid_size, VoxelSparseParams(VOXEL_SPARSE_V3, 20, 0))

    def voxelDownSampleV2(self, cloud, grid_size, max_voxel_pts=20, min_voxel_pts=0):
        """pcp::VoxelDownSampleV2 (pcp.hpp:78-154, KISS-ICP's voxel hash; pcr_voxel_filter_sparse): voxel = (int)(p / grid_size); per voxel the
        max_voxel_pts rows of lowest index, emitted when more than min_voxel_pts: the first row's record with x, y, z replaced by their float mean.
        Ascending (z, y, x).  Host array in -> numpy array out; CUDA tensor in -> CUDA tensor out."""
        return self._voxel_sparse(cloud, grid_size, VoxelSparseParams(VOXEL_SPARSE_V2, int(max_voxel_pts), int(min_voxel_pts)))

    def sparseOrder(self):
        """pcr_voxel_sparse_order: what the last voxelDownSampleV3 / V2 on this registrar sorted -> (keys (m,) uint64, rows (m,) uint32): per kept
        input row, in sorted order, its packed voxel key and its original row index."""
        cnt = C.c_size_t(0)
        self._check(self._lib.pcr_voxel_sparse_order(self._h, None, None, 0, C.byref(cnt)))
        keys, rows = np.zeros(cnt.value, np.uint64), np.zeros(cnt.value, np.uint32)
        if cnt.value:
            self._check(self._lib.pcr_voxel_sparse_order(self._h, keys.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), cnt.value, C.byref(cnt)))
        return keys, rows

    def voxelDownSampleBegin(self, cloud, grid_size):
        """pcr_voxel_filter_begin for a CUDA tensor: queue the filter, return a token for voxelDownSampleEnd (the input must stay alive until then)."""
        import torch
        p, n, s, dev, keep = _cloud(cloud)
        if not dev:
            raise PcrError("voxelDownSampleBegin takes a CUDA tensor")
        out = torch.empty((max(n, 1), s // 4), dtype=torch.float32, device=keep.device)
        self._check(self._lib.pcr_voxel_filter_begin(self._h, p, n, s, float(grid_size), C.c_void_p(out.data_ptr()), n))
        return (out, keep)

    def voxelDownSampleEnd(self, token):
        cnt = C.c_size_t(0)
        self._check(self._lib.pcr_voxel_filter_end(self._h, C.byref(cnt)))
        return token[0][:cnt.value]

    # -- introspection ---------------------------------------------------------
    def stats(self):
        st = PcrStats()
        self._check(self._lib.pcr_get_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in PcrStats._fields_}

    def set_profile(self, level):
        self._check(self._lib.pcr_set_profile(self._h, int(level)))

    def set_stream(self, stream_ptr):
        self._check(self._lib.pcr_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_query_tile(self, lo, hi):
        lo = np.ascontiguousarray(lo, np.float64)
        hi = np.ascontiguousarray(hi, np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.pcr_set_query_tile(self._h, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp)))

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._check(self._lib.pcr_comm_init(self._h, C.cast(buf, C.c_void_p), rank, nranks))

    def comm_info(self):
        """pcr_comm_info -> dict(rank, nranks, transport): who takes part in this handle's exchange, as the communicator reports it."""
        r, n, t = C.c_int(0), C.c_int(1), C.c_int(0)
        self._check(self._lib.pcr_comm_info(self._h, C.byref(r), C.byref(n), C.byref(t)))
        return dict(rank=r.value, nranks=n.value, transport={0: "none", 1: "rccl", 2: "host", 3: "peer"}[t.value])

    def comm_peer_export(self):
        """64 bytes naming this rank's receive buffer of the peer exchange (pcr_comm_peer_export): share them in rank order, then comm_init_peer"""
        buf = C.create_string_buffer(64)
        self._check(self._lib.pcr_comm_peer_export(self._h, buf))
        return bytes(buf.raw)

    def comm_init_peer(self, handles, rank, nranks):
        """pcr_comm_init_peer: `handles` = every rank's comm_peer_export(), in rank order"""
        blob = b"".join(handles)
        assert len(blob) == 64 * nranks
        self._check(self._lib.pcr_comm_init_peer(self._h, blob, rank, nranks))

    def comm_init_host(self, fn, rank, nranks):
        """The exchange of a sharded call through the caller's collective (pcr_comm_init_host): fn(ptr, count, op, user) -> 0,
        combining `count` doubles in place over all ranks (op 0 = sum, 1 = max).  shard.ThreadCollective / shard.gloo_collective
        provide one.  fn = None clears it."""
        self._ar = ALLREDUCE_FN(fn) if fn is not None else ALLREDUCE_FN()      # kept alive with the handle
        self._check(self._lib.pcr_comm_init_host(self._h, self._ar, None, rank, nranks))

    def set_shard(self, lo, hi, halo):
        """pcr_set_shard: this rank's tile [lo, hi) and the halo its target cloud carries (shard.tile_for_method)."""
        lo = np.ascontiguousarray(lo, np.float64)
        hi = np.ascontiguousarray(hi, np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.pcr_set_shard(self._h, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), float(halo)))

    def set_params(self, **overrides):
        """pcr_set_params on the live handle: change optimiser settings between calls (e.g. VgicpRegister.initForLC)."""
        p = PcrParams()
        self._check(self._lib.pcr_get_params(self._h, C.byref(p)))
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise AttributeError(f"pcr_params has no field {k!r}")
            setattr(p, k, v)
        self._check(self._lib.pcr_set_params(self._h, C.byref(p)))
        self.params = p

    def fitnessGated(self, src, pose, max_sq=1.0):
        """getFitnessScore of the reference's test/align.cpp:29-61 against the handle's current target: mean of the squared
        1-NN distances <= max_sq of the source transformed by `pose` (-1 when none) and the number of points counted."""
        p, n, s, dev, _k = _cloud(src)
        pc = _pose_in(pose)
        score, cnt = C.c_double(0), C.c_int64(0)
        self._check(self._lib.pcr_fitness_gated(self._h, p, n, s, dev, pc.ctypes.data_as(C.POINTER(C.c_double)), float(max_sq), C.byref(score), C.byref(cnt)))
        return score.value, int(cnt.value)

    def fitnessBatch(self, src, poses, max_sq=1.0, score_points=0):
        """pcr_fitness_batch: fitnessGated of every pose of `poses` (K, 4, 4) in one pass -> (scores (K,) float64, n_in (K,) int64).  A pose a
        cut dense index cannot score is scored on the sparse index of the kept target (exactly); (-1, -1) only where that cannot be had
        (a caller's device target).  score_points: 0 = every point, else the subset floor(j n / score_points)."""
        p, n, s, dev, _k = _cloud(src)
        P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        cm = np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(-1)      # column-major per pose
        K = P.shape[0]
        scores = np.zeros(K, np.float64)
        n_in = np.zeros(K, np.int64)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.pcr_fitness_batch(self._h, p, n, s, dev, cm.ctypes.data_as(dp), K, float(max_sq), int(score_points),
                                                scores.ctypes.data_as(dp), n_in.ctypes.data_as(C.POINTER(C.c_int64))))
        return scores, n_in

    def knn(self, queries, k):
        """pcr_knn: the k nearest points of the kept target (setTarget) of every query -> (idx (n, k) int64, d2 (n, k) float64), each row
        ascending by (d2, idx); nanoflann's f64 distances on float coordinates, bit for bit.  Missing neighbours: idx -1, d2 +inf."""
        p, n, s, dev, _k = _cloud(queries)
        k = int(k)
        idx = np.zeros((n, max(k, 0)), np.int64)
        d2 = np.zeros((n, max(k, 0)), np.float64)
        self._check(self._lib.pcr_knn(self._h, p, n, s, dev, k, idx.ctypes.data_as(C.POINTER(C.c_int64)), d2.ctypes.data_as(C.POINTER(C.c_double))))
        return idx, d2

    def radiusSearch(self, queries, radius, sorted=True):
        """pcr_radius_search: the points of the kept target with d2 < radius^2 of every query -> (offsets (n + 1,) uint64, idx int64, d2 float64);
        query q's results are [offsets[q], offsets[q + 1]), ascending by (d2, idx) when sorted.  Sized by a first call that only counts."""
        p, n, s, dev, _k = _cloud(queries)
        offsets = np.zeros(n + 1, np.uint64)
        total = C.c_size_t(0)
        op, ip, dp = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_double)
        rc = self._lib.pcr_radius_search(self._h, p, n, s, dev, float(radius), int(bool(sorted)), 0, offsets.ctypes.data_as(op), None, None, C.byref(total))
        if rc != 0 and total.value == 0:
            self._check(rc)
        idx = np.zeros(total.value, np.int64)
        d2 = np.zeros(total.value, np.float64)
        if total.value:
            self._check(self._lib.pcr_radius_search(self._h, p, n, s, dev, float(radius), int(bool(sorted)), total.value, offsets.ctypes.data_as(op),
                                                    idx.ctypes.data_as(ip), d2.ctypes.data_as(dp), C.byref(total)))
        return offsets, idx, d2

    def queryIndexInfo(self):
        """pcr_query_index_info -> dict(kind, n_points, bytes): the index that answered the last knn / radiusSearch or fitness score ("dense",
        "sparse", or None when none has been answered since the target was set), the points it holds and the device memory it occupies."""
        kind, n, b = C.c_int(-1), C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pcr_query_index_info(self._h, C.byref(kind), C.byref(n), C.byref(b)))
        return dict(kind={QUERY_INDEX_DENSE: "dense", QUERY_INDEX_SPARSE: "sparse"}.get(kind.value), n_points=int(n.value), bytes=int(b.value))

    def relocalize(self, src, pose, **params):
        """pcr_relocalize from the coarse pose `pose` (4x4, updated in place as align() does) against the kept target (setTarget):
        -> (converged, candidates, chosen).  candidates: one dict per refined hypothesis (hypothesis, coarse_n_in, coarse_score, pose,
        converged, n_in, score); chosen: the index of the one taken.  params: fields of pcr_reloc_params (reloc_params)."""
        p, n, s, dev, _k = _cloud(src)
        rp = reloc_params(**params)
        pose_np = np.asarray(pose)
        if pose_np.shape != (4, 4):
            raise ValueError("pose must be 4x4")
        pc = _pose_in(pose_np)
        cap = rp.refine_top + 1
        cands = (RelocCandidate * cap)()
        conv, nc, ch = C.c_int(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pcr_relocalize(self._h, p, n, s, dev, C.byref(rp), pc.ctypes.data_as(C.POINTER(C.c_double)), C.byref(conv),
                                             cands, cap, C.byref(nc), C.byref(ch)))
        pose_np[...] = _pose_out(pc)
        out = [_cand_dict(c) for c in cands[:nc.value]]
        self.isConverge = bool(conv.value)
        return self.isConverge, out, int(ch.value)

    def relocalizeGlobal(self, src, sc, kf_poses, pose, **params):
        """pcr_relocalize_global: relocalise with no prior against the kept target (setTarget: the whole map).  sc: the ScanContext
        database with one context per key frame, kf_poses: their (M, 4, 4) poses; `pose` (4x4) receives the chosen pose in place.
        -> (converged, candidates, chosen).  candidates: one dict per refined hypothesis (place, sc_dist, sc_shift and relocalize's
        fields; hypothesis numbers the pose within its place's lattice).  params: fields of pcr_global_reloc_params (global_reloc_params)."""
        if not isinstance(sc, ScanContext):
            raise TypeError("sc must be a ScanContext")
        p, n, s, dev, _k = _cloud(src)
        gp = global_reloc_params(**params)
        pose_np = np.asarray(pose)
        if pose_np.shape != (4, 4) or pose_np.dtype != np.float64:
            raise ValueError("pose must be a float64 4x4 array (written in place)")
        kf = np.asarray(kf_poses, np.float64)
        if kf.ndim != 3 or kf.shape[1:] != (4, 4):
            raise ValueError("kf_poses must have shape (M, 4, 4)")
        kf_cm = np.ascontiguousarray(kf.transpose(0, 2, 1)).reshape(-1)      # column-major per pose
        cap = max(gp.places, 0) * max(gp.local.refine_top, 0)
        cands = (GlobalRelocCandidate * max(cap, 1))()
        out_pose = np.zeros(16)
        conv, nc, ch = C.c_int(0), C.c_size_t(0), C.c_size_t(0)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.pcr_relocalize_global(self._h, sc._s, kf_cm.ctypes.data_as(dp), kf.shape[0], p, n, s, dev, C.byref(gp),
                                                    out_pose.ctypes.data_as(dp), C.byref(conv), cands, cap, C.byref(nc), C.byref(ch)))
        pose_np[...] = _pose_out(out_pose)
        out = []
        for g in cands[:nc.value]:
            d = dict(place=int(g.place), sc_dist=g.sc_dist, sc_shift=int(g.sc_shift))
            d.update(_cand_dict(g.c))
            out.append(d)
        self.isConverge = bool(conv.value)
        return self.isConverge, out, int(ch.value)

    def _check(self, rc):
        if rc != 0:
            raise PcrError(self._lib.pcr_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pcr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LoamRegister(PointCloudRegister):
    """PCR::LoamRegister (reference PCR/src/LoamRegister.cpp)."""
    method = "loam"

    def linearize(self, src, pose, per_point=False):
        """One linearisation against the current target (setTarget): dict(JtJ, JtE, n[, status, rows, nn])."""
        p, n, s, dev, _k = _cloud(src)
        pc = _pose_in(pose)
        JtJ = np.zeros(36)
        JtE = np.zeros(6)
        cnt = C.c_int64(0)
        status = np.zeros(n, np.int8) if per_point else None
        rows = np.zeros((n, 7)) if per_point else None
        nn = np.zeros((n, 5), np.int32) if per_point else None
        dp = C.POINTER(C.c_double)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._check(self._lib.pcr_loam_linearize(self._h, p, n, s, dev, pc.ctypes.data_as(dp), JtJ.ctypes.data_as(dp),
                                                 JtE.ctypes.data_as(dp), C.byref(cnt), vp(status), vp(rows), vp(nn)))
        out = dict(JtJ=JtJ.reshape(6, 6), JtE=JtE, n=int(cnt.value))
        if per_point:
            out.update(status=status, rows=rows, nn=nn)
        return out

    def trace(self):
        """Per-iteration normal equations of the last call (needs record_trace=1)."""
        it = max(1, self.params.loam_iters)
        JtJ, JtE, n, x = np.zeros((it, 36)), np.zeros((it, 6)), np.zeros(it, np.int64), np.zeros((it, 6))
        k = C.c_int32(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.pcr_get_trace(self._h, C.byref(k), vp(JtJ), vp(JtE), vp(n), vp(x)))
        k = k.value
        hits, srch = np.zeros(it, np.int64), np.zeros(it, np.int64)
        self._check(self._lib.pcr_get_trace_counts(self._h, vp(hits), vp(srch)))
        return dict(iters_run=k, JtJ=JtJ[:k].reshape(-1, 6, 6), JtE=JtE[:k], n=n[:k], x=x[:k], cache_hits=hits[:k], searches=srch[:k])

    def timeline(self):
        """[launch][block][24] stamps in microseconds relative to each launch's earliest block entry
        (needs pcr_params.record_timeline = 1).  Columns 0-7: entry, prologue, posted, searched, plane, accumulated (entry stores issued), stored, partial
        sums folded (inside the prologue); 8-10 (dense search only): row ranges in LDS, first candidate chunk arrived, candidate stream done; 11: normal
        equations solved (inside the prologue); 12-15 (lanes that searched): gather returned, distances and proof, plane solved, plane gate; 16: pose in
        registers, 17: hit test done (both before 'posted'); 18: rows in LDS, 19: chunk sums done (both before 'accumulated'); 21: the wave's LDS-DMA of its cache
        entries has landed, 22: entry in registers, 23: the prologue's closing barrier passed (21-23 before 'prologue'; 21 and 22 not in launch 0),
        20: pose in registers (before 16)."""
        nl, nb = C.c_int(0), C.c_int(0)
        self._check(self._lib.pcr_get_timeline(self._h, None, 0, C.byref(nl), C.byref(nb)))
        raw = np.zeros((nl.value, nb.value, 24), np.uint64)
        self._check(self._lib.pcr_get_timeline(self._h, raw.ctypes.data_as(C.c_void_p), raw.size, C.byref(nl), C.byref(nb)))
        t = raw.astype(np.int64)
        return (t - t[:, :, :1].min(axis=1, keepdims=True)) / 100.0


class NdtRegister(PointCloudRegister):
    """PCR::NdtRegister (reference PCR/src/NdtRegister.cpp).  ndt_search=NDT_DIRECT26 | NDT_DIRECT7 | NDT_DIRECT1
    (NormalDistributionsTransform::setNeighborhoodSearchMethod, default NDT_DIRECT7) is a keyword argument like every other field of
    pcr_params, here and in make_register("ndt", ...); set_params changes it on a live handle and keeps the prepared target."""
    method = "ndt"

    def derivatives(self, src, p6, double_hessian=False, device_loop=False, kind=0):
        """One computeDerivatives pass at p = [t; roll pitch yaw] against the current target, by the kernels of the host-driven loop.
        device_loop=True: by the launches of the device-resident loop instead (pcr_ndt_pass_sums: the pass kernel scan2Map runs by default,
        its rows folded in the prologue of the next launch); kind 0 = score, gradient, float Hessian, 1 = score and gradient only (a
        line-search pass), 2 = the double Hessian alone (returned as hess_d)."""
        p, n, s, dev, _k = _cloud(src)
        p6 = np.ascontiguousarray(p6, np.float64).reshape(6)
        if device_loop:
            if double_hessian:
                raise ValueError("device_loop: the double Hessian is a pass of its own, kind=2")
            g, H = np.zeros(6), np.zeros(36)
            sc = C.c_double(0)
            dp = C.POINTER(C.c_double)
            self._check(self._lib.pcr_ndt_pass_sums(self._h, p, n, s, dev, p6.ctypes.data_as(dp), int(kind), C.byref(sc), g.ctypes.data_as(dp),
                                                    H.ctypes.data_as(dp)))
            if kind == 2:
                return dict(hess_d=H.reshape(6, 6))
            return dict(score=sc.value, grad=g) if kind == 1 else dict(score=sc.value, grad=g, hess=H.reshape(6, 6))
        g, H = np.zeros(6), np.zeros(36)
        Hd = np.zeros(36) if double_hessian else None
        sc = C.c_double(0)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.pcr_ndt_derivatives(self._h, p, n, s, dev, p6.ctypes.data_as(dp), C.byref(sc), g.ctypes.data_as(dp),
                                                  H.ctypes.data_as(dp), Hd.ctypes.data_as(dp) if Hd is not None else None))
        out = dict(score=sc.value, grad=g, hess=H.reshape(6, 6))
        if double_hessian:
            out["hess_d"] = Hd.reshape(6, 6)
        return out

    def voxels(self):
        """The voxel Gaussians of the current target (setTarget; pcr_ndt_voxels), sorted by (ix, iy, iz): dict(ijk (m, 3) int32 = the
        lattice coordinates floorf(p * inv_leaf), n (m,), mean (m, 3), icov (m, 3, 3), rejected = cells with enough points whose
        covariance failed the eigenvalue or the inverse test).  Raises on a handle whose target scan2Map prepared for one scan's region."""
        cnt, rej = C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pcr_ndt_voxels(self._h, None, 0, C.byref(cnt), C.byref(rej)))
        rec = np.dtype([("ijk", np.int32, 3), ("n", np.int32), ("mean", np.float64, 3), ("icov", np.float64, (3, 3))])
        assert rec.itemsize == 112
        raw = np.zeros(cnt.value, rec)
        if cnt.value:
            self._check(self._lib.pcr_ndt_voxels(self._h, raw.ctypes.data_as(C.c_void_p), raw.size, C.byref(cnt), C.byref(rej)))
        raw = raw[np.lexsort((raw["ijk"][:, 2], raw["ijk"][:, 1], raw["ijk"][:, 0]))]
        return dict(ijk=raw["ijk"].copy(), n=raw["n"].copy(), mean=raw["mean"].copy(), icov=raw["icov"].copy(), rejected=int(rej.value))


class VgicpRegister(PointCloudRegister):
    """PCR::VgicpRegister (reference PCR/src/VgicpRegister.cpp).  fast_gicp's two settings are keyword arguments like every other field of
    pcr_params: vgicp_regularization=REG_* (FastGICP::setRegularizationMethod, default REG_PLANE) and vgicp_voxel_mode=VOXEL_*
    (FastVGICP::setVoxelAccumulationMode, default VOXEL_ADDITIVE); set_params changes them on a live handle and drops the prepared target.
    vgicp_search=VGICP_DIRECT27 | VGICP_DIRECT7 | VGICP_DIRECT1 (FastVGICP::setNeighborSearchMethod, default VGICP_DIRECT1) is one too, here and
    in make_register("vgicp", ...); set_params changes it and KEEPS the prepared target."""
    method = "vgicp"

    def correspondences(self):
        """The (source row, voxel) pairs of the last linearize() (pcr_vgicp_correspondences): dict(row (m,) int32, ijk (m, 3) int32 = the
        voxel's lattice coordinates as voxels() reports them), ordered by row, a row's pairs in the order of the vgicp_search table."""
        cnt = C.c_size_t(0)
        self._check(self._lib.pcr_vgicp_correspondences(self._h, None, 0, C.byref(cnt)))
        rec = np.dtype([("row", np.int32), ("ijk", np.int32, 3)])
        assert rec.itemsize == 16
        raw = np.zeros(cnt.value, rec)
        if cnt.value:
            self._check(self._lib.pcr_vgicp_correspondences(self._h, raw.ctypes.data_as(C.c_void_p), raw.size, C.byref(cnt)))
        return dict(row=raw["row"].copy(), ijk=raw["ijk"].copy())

    def voxels(self):
        """The Gaussian voxels of the kept target (setTarget; pcr_vgicp_voxels), sorted by (ix, iy, iz): dict(ijk (m, 3) int32 = the lattice
        coordinates floor(p / res - 0.5), n (m,), mean (m, 3), cov (m, 3, 3)).  Raises on a handle whose target scan2Map prepared for one
        scan's region."""
        cnt = C.c_size_t(0)
        self._check(self._lib.pcr_vgicp_voxels(self._h, None, 0, C.byref(cnt)))
        rec = np.dtype([("ijk", np.int32, 3), ("n", np.int32), ("mean", np.float64, 3), ("cov6", np.float64, 6)])
        assert rec.itemsize == 88
        raw = np.zeros(cnt.value, rec)
        if cnt.value:
            self._check(self._lib.pcr_vgicp_voxels(self._h, raw.ctypes.data_as(C.c_void_p), raw.size, C.byref(cnt)))
        raw = raw[np.lexsort((raw["ijk"][:, 2], raw["ijk"][:, 1], raw["ijk"][:, 0]))]
        cov = raw["cov6"][:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
        return dict(ijk=raw["ijk"].copy(), n=raw["n"].copy(), mean=raw["mean"].copy(), cov=cov.copy())

    def initForLC(self):
        """VgicpRegister::initForLC (VgicpRegister.cpp:21-28) on the live object, as LoopClosureManager's constructor calls it
        (backend/src/LoopClosureManager.cpp:21-22): 100 iterations, transformation epsilon 1e-6.  (Its
        setMaxCorrespondenceDistance(150) only acts in the non-voxel GICP, fast_gicp_impl.hpp:18.)"""
        self.set_params(vgicp_max_iters=100, vgicp_trans_eps=1e-6)

    def covariances(self, pts):
        """(n,3,3) per-point covariances (fast_gicp_impl.hpp:241-297)."""
        p, n, s, dev, _k = _cloud(pts)
        c6 = np.zeros((n, 6))
        self._check(self._lib.pcr_vgicp_covariances(self._h, p, n, s, dev, c6.ctypes.data_as(C.c_void_p)))
        out = np.zeros((n, 3, 3))
        out[:, 0, 0], out[:, 0, 1], out[:, 0, 2], out[:, 1, 1], out[:, 1, 2], out[:, 2, 2] = c6.T
        out[:, 1, 0], out[:, 2, 0], out[:, 2, 1] = out[:, 0, 1], out[:, 0, 2], out[:, 1, 2]
        return out

    def neighbours(self, n):
        """(n,20) original indices of every point's 20 nearest neighbours as the last covariances() call on a scan-sized cloud found them
        (0xffffffff: none), and the number of queries that went to the wave-per-query search."""
        out = np.zeros((n, 20), np.uint32)
        q = C.c_uint32(0)
        self._check(self._lib.pcr_vgicp_neighbours(self._h, n, out.ctypes.data_as(C.c_void_p), C.byref(q)))
        return out, int(q.value)

    def linearize(self, src, pose):
        p, n, s, dev, _k = _cloud(src)
        pc = _pose_in(pose)
        H, b = np.zeros(36), np.zeros(6)
        err, nc = C.c_double(0), C.c_int64(0)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.pcr_vgicp_linearize(self._h, p, n, s, dev, pc.ctypes.data_as(dp), H.ctypes.data_as(dp),
                                                  b.ctypes.data_as(dp), C.byref(err), C.byref(nc)))
        return dict(H=H.reshape(6, 6), b=b, err=err.value, n=int(nc.value))


class GicpRegister(PointCloudRegister):
    """PCR::VgicpRegister with fast_gicp::FastGICP as its registrar (fast_gicp_impl.hpp:103-237): correspondences by exact nearest
    neighbour, the two covariances fused per pair."""
    method = "gicp"      # (vgicp_regularization=REG_* is read here too; vgicp_voxel_mode is ignored: there are no voxels)
    covariances = VgicpRegister.covariances      # (pcr_vgicp_covariances / pcr_vgicp_neighbours serve gicp handles: the same covariances)
    neighbours = VgicpRegister.neighbours

    def initForLC(self):
        """VgicpRegister::initForLC (VgicpRegister.cpp:21-28): 100 iterations, transformation epsilon 1e-6, and
        setMaxCorrespondenceDistance(150), which acts here (fast_gicp_impl.hpp:136)."""
        self.set_params(vgicp_max_iters=100, vgicp_trans_eps=1e-6, gicp_max_corr_dist=150.0)

    def linearize(self, src, pose, pose_eval=None, per_point=False):
        """One update_correspondences + linearize at `pose` against the kept target (setTarget): dict(H, b, err, n[, err_eval][, corr, d2, M]).
        err_eval = compute_error(pose_eval) on the correspondences of that linearisation; per_point: corr (n,) int32 with -1 for none,
        d2 (n,) float32 with +inf for none, M (n,3,3)."""
        p, n, s, dev, _k = _cloud(src)
        pc = _pose_in(pose)
        pe = _pose_in(pose_eval) if pose_eval is not None else None
        H, b = np.zeros(36), np.zeros(6)
        err, err_eval, nc = C.c_double(0), C.c_double(0), C.c_int64(0)
        corr = np.zeros(n, np.int32) if per_point else None
        d2 = np.zeros(n, np.float32) if per_point else None
        m6 = np.zeros((n, 6)) if per_point else None
        dp = C.POINTER(C.c_double)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._check(self._lib.pcr_gicp_linearize(self._h, p, n, s, dev, pc.ctypes.data_as(dp), pe.ctypes.data_as(dp) if pe is not None else None,
                                                 H.ctypes.data_as(dp), b.ctypes.data_as(dp), C.byref(err), C.byref(err_eval), C.byref(nc),
                                                 vp(corr), vp(d2), vp(m6)))
        out = dict(H=H.reshape(6, 6), b=b, err=err.value, n=int(nc.value))
        if pe is not None:
            out["err_eval"] = err_eval.value
        if per_point:
            M = np.zeros((n, 3, 3))
            M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2] = m6.T
            M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]
            out.update(corr=corr, d2=d2, M=M)
        return out


def liorf_pose_to_6dof(T):
    """pcr_liorf_pose_to_6dof (host only): [roll, pitch, yaw, x, y, z] as float32 -- pcl::getEulerAngles and the translation of the float cast of T."""
    c = _pose_in(T)
    out = np.zeros(6, np.float32)
    if load_library().pcr_liorf_pose_to_6dof(c.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise PcrError("pcr_liorf_pose_to_6dof failed")
    return out


def liorf_6dof_to_pose(six):
    """pcr_liorf_6dof_to_pose (host only): pcl::getTransformation of [roll, pitch, yaw, x, y, z], formed in float; a 4x4 float64 array of float values."""
    s = np.ascontiguousarray(six, dtype=np.float32).reshape(6)
    buf = np.zeros(16)
    if load_library().pcr_liorf_6dof_to_pose(s.ctypes.data_as(C.POINTER(C.c_float)), buf.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        raise PcrError("pcr_liorf_6dof_to_pose failed")
    return _pose_out(buf)


class LiorfRegister(PointCloudRegister):
    """LioScan2map of the reference's test/comp/liorf_scan2map.cpp: LIO-SAM's surface scan-to-map (5-NN, float plane fit, weighted point-to-plane
    rows, 6 x 6 normal equations on [roll, pitch, yaw, x, y, z]).  The liorf_* fields of pcr_params are keyword arguments; getFitnessScore() is the
    file's own score (mean squared 1-NN distance over d2 <= 1, -1 when there is none)."""
    method = "liorf"

    def result(self):
        """pcr_liorf_result of the last scan2Map / align: dict(six (6,) float32, degenerate bool, rows_last int)."""
        six = np.zeros(6, np.float32)
        deg, rows = C.c_int(0), C.c_int64(0)
        self._check(self._lib.pcr_liorf_result(self._h, six.ctypes.data_as(C.POINTER(C.c_float)), C.byref(deg), C.byref(rows)))
        return dict(six=six, degenerate=bool(deg.value), rows_last=int(rows.value))

    def isDegenerate(self):
        return self.result()["degenerate"]

    def linearize(self, src, six):
        """One linearisation at the six numbers against the kept target (setTarget; pcr_liorf_linearize): dict(T (4,4) float32 = the matrix the
        device built, kept (n,) bool, coeff (n,4) float32, AtA (6,6), AtB (6,), n)."""
        p, n, s, dev, _k = _cloud(src)
        s6 = np.ascontiguousarray(six, dtype=np.float32).reshape(6)
        T = np.zeros(16, np.float32)
        kept = np.zeros(n, np.uint8)
        coeff = np.zeros((n, 4), np.float32)
        AtA, AtB = np.zeros(36), np.zeros(6)
        nk = C.c_int64(0)
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        self._check(self._lib.pcr_liorf_linearize(self._h, p, n, s, dev, s6.ctypes.data_as(fp), T.ctypes.data_as(fp), kept.ctypes.data_as(C.c_void_p),
                                                  coeff.ctypes.data_as(C.c_void_p), AtA.ctypes.data_as(dp), AtB.ctypes.data_as(dp), C.byref(nk)))
        return dict(T=T.reshape(4, 4), kept=kept.astype(bool), coeff=coeff, AtA=AtA.reshape(6, 6), AtB=AtB, n=int(nk.value))

    def trace(self):
        """Per solved iteration of the last call (record_trace=1): dict(AtA (k,6,6), AtB (k,6), x (k,6), n (k,)) -- the float systems and steps."""
        iters = max(int(self.params.liorf_iters), 1)
        n_it = C.c_int32(0)
        A, b, x = np.zeros(iters * 36), np.zeros(iters * 6), np.zeros(iters * 6)
        n = np.zeros(iters, np.int64)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.pcr_get_trace(self._h, C.byref(n_it), A.ctypes.data_as(dp), b.ctypes.data_as(dp), n.ctypes.data_as(C.POINTER(C.c_int64)),
                                            x.ctypes.data_as(dp)))
        k = n_it.value
        return dict(AtA=A.reshape(-1, 6, 6)[:k], AtB=b.reshape(-1, 6)[:k], x=x.reshape(-1, 6)[:k], n=n[:k])


def make_register(pcr_type, **overrides):
    """The reference's factory on cfg["frontend"]["pcr"] (LidarOdometry.cpp:32,44-54), plus "gicp" and "liorf"."""
    table = {"loam": LoamRegister, "ndt": NdtRegister, "vgicp": VgicpRegister, "gicp": GicpRegister, "liorf": LiorfRegister}
    if pcr_type not in table:
        raise RuntimeError(f"such pcr type({pcr_type}) is not exist, please implemented your self!")
    return table[pcr_type](**overrides)


def host_pin(array):
    """pcr_host_pin on a numpy array's buffer (kept pinned until host_unpin(array); the array must stay alive and unresized)."""
    a = np.asarray(array)
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("only contiguous arrays can be pinned")
    if load_library().pcr_host_pin(a.ctypes.data_as(C.c_void_p), a.nbytes) != 0:
        raise PcrError(load_library().pcr_last_error(None).decode())


def host_unpin(array):
    a = np.asarray(array)
    if load_library().pcr_host_unpin(a.ctypes.data_as(C.c_void_p)) != 0:
        raise PcrError(load_library().pcr_last_error(None).decode())


def comm_unique_id():
    buf = (C.c_char * 128)()
    if load_library().pcr_comm_unique_id(C.cast(buf, C.c_void_p)) != 0:
        raise PcrError(load_library().pcr_last_error(None).decode())
    return bytes(buf)


TUM_OK, TUM_ERROR, TUM_SKIP = 0, 1, 2      # PCR_TUM_*: what pcr_tum_parse returns


def _session_error():
    return PcrError(load_library().pcr_session_last_error().decode())


def tum_format(stamp, pose, precise=False, capacity=512):
    """pcr_tum_format -> one line of tum.txt (bytes, with its newline): writeAsTum's "%.3f %.3f %.3f %.3f %.6f %.6f %.6f %.6f" of stamp, t and
    Eigen::Quaternion(R) as x y z w -- lossy; precise=True writes %.17g.  A non-finite pose or a capacity that cannot hold the line raises."""
    buf = C.create_string_buffer(max(int(capacity), 1))
    pc = _pose_in(pose)
    if load_library().pcr_tum_format(float(stamp), pc.ctypes.data_as(C.POINTER(C.c_double)), int(bool(precise)), buf, int(capacity)):
        raise _session_error()
    return buf.value


def tum_parse(line):
    """pcr_tum_parse -> (stamp, 4x4 pose) as loadFromTum reads a line (the quaternion is NOT normalised), or None for a blank line; fewer than
    eight numbers raise with the line in the message."""
    if isinstance(line, str):
        line = line.encode()
    stamp, pose = C.c_double(0), np.zeros(16)
    rc = load_library().pcr_tum_parse(line, C.byref(stamp), pose.ctypes.data_as(C.POINTER(C.c_double)))
    if rc == TUM_SKIP:
        return None
    if rc != TUM_OK:
        raise _session_error()
    return stamp.value, _pose_out(pose)


def pcd_write(path, cloud):
    """pcr_pcd_write: a host array (n, >=3) float32 as a binary "x y z intensity" PCD (pcp::savePCDFile); the intensity is column 3 of a
    4-column cloud, column 4 of a wider one."""
    a = np.ascontiguousarray(cloud, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("clouds must have shape (n, >=3)")
    if load_library().pcr_pcd_write(os.fsencode(path), a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1] * 4):
        raise _session_error()


def pcd_read(path, columns=4):
    """pcr_pcd_read -> (n, columns) float32 (pcp::loadPCDFile): 4 columns x y z intensity; 8 the pcl::PointXYZI layout x y z 1 intensity 0 0 0."""
    L = load_library()
    n = C.c_size_t(0)
    if L.pcr_pcd_read(os.fsencode(path), None, 0, int(columns) * 4, C.byref(n)):
        raise _session_error()
    out = np.zeros((n.value, int(columns)), np.float32)
    if L.pcr_pcd_read(os.fsencode(path), out.ctypes.data_as(C.c_void_p), n.value, int(columns) * 4, C.byref(n)):
        raise _session_error()
    return out


def _stamps_in(stamps, n):
    if stamps is None:
        return None, None
    a = np.ascontiguousarray(stamps, dtype=np.float64).reshape(-1)
    if a.size != n:
        raise ValueError(f"stamps holds {a.size} entries for {n} key frames")
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _tum_lines(directory):
    """how many key frames a tum.txt can name at most (the size of the stamps buffer a load hands over)"""
    try:
        with open(os.path.join(os.fspath(directory), "tum.txt"), "rb") as f:
            return sum(1 for _ in f)
    except OSError:
        return 0


class SubMap:
    """The key-frame store and sub-map of the reference's MapManager (frontend/src/MapManager.cpp:151-201), kept in HBM.

    addKeyFrame(points, pose); updateMap(position) selects the key frames within `radius` (8 m, MapManager.hpp:68), transforms
    and concatenates them and voxel-filters the result; `pointer()` is the device-resident sub-map that
    PointCloudRegister.scan2MapSubmap registers against without a host copy."""

    def __init__(self, device=-1, _view_of=None):
        self._lib = load_library()
        self._parent = _view_of      # (a view holds its parent: Python cannot collect the store before the sub-maps that read it)
        if _view_of is not None:
            self._m = self._lib.pcr_map_view(_view_of._m)
            if not self._m:
                raise PcrError(self._lib.pcr_map_last_error(_view_of._m).decode())
            return
        self._m = self._lib.pcr_map_create(int(device))
        if not self._m:
            raise PcrError(self._lib.pcr_map_last_error(None).decode())

    def view(self):
        """pcr_map_view: another sub-map over the same key frames (LoopClosureManager's lc_map_ beside MapManager's mSubmap) with its own stream,
        buffers, selection and generation.  It reads this store and cannot change it."""
        return SubMap(_view_of=self)

    def setPoses(self, first, poses):
        """pcr_map_set_poses (Backend::optimHandler, Backend.cpp:315-318): poses = (k, 4, 4) for key frames first .. first+k-1.  No sub-map and no
        generation changes; the next update selects and transforms with them."""
        P = np.asarray(poses, dtype=np.float64)
        if P.ndim == 2:
            P = P[None]
        if P.ndim != 3 or P.shape[1:] != (4, 4):
            raise ValueError("poses must have shape (k, 4, 4)")
        cm = np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(-1)      # column-major, one after the other
        self._check(self._lib.pcr_map_set_poses(self._m, int(first), P.shape[0], cm.ctypes.data_as(C.POINTER(C.c_double))))

    def keyFramePointer(self, i):
        """pcr_map_keyframe -> (device pointer, number of points, stride in bytes) of stored key frame i: a source for scan2MapSubmap."""
        if not 0 <= int(i) < self.keyframes():
            raise PcrError("key-frame index out of range")
        n, s = C.c_size_t(0), C.c_size_t(0)
        p = self._lib.pcr_map_keyframe(self._m, int(i), C.byref(n), C.byref(s), None)
        return p, n.value, s.value

    def keyFrame(self, i):
        """pcr_map_read_keyframe -> (host array of the stored points, 4x4 pose)."""
        _, cnt, stride = self.keyFramePointer(i)
        n, s = C.c_size_t(cnt), C.c_size_t(stride)
        pose = np.zeros(16)
        pp = pose.ctypes.data_as(C.POINTER(C.c_double))
        out = np.zeros((n.value, max(s.value // 4, 1)), np.float32)
        self._check(self._lib.pcr_map_read_keyframe(self._m, int(i), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n), pp))
        return out, _pose_out(pose)

    def downSampleKeyFrames(self, first, grid_size):
        """pcr_map_downsample_keyframes (MapManager::saveKfs :211, MapManager() :46): key frames first .. end replaced by their voxel-filtered
        clouds, the store compacted -> points in the store."""
        n = C.c_size_t(0)
        self._check(self._lib.pcr_map_downsample_keyframes(self._m, int(first), float(grid_size), C.byref(n)))
        return n.value

    def updateAll(self, grid_size=0.4):
        """pcr_map_update_all (test/vis_globalmap.cpp:33-66): the whole map -- every key frame under its pose, concatenated, voxel-filtered."""
        n = C.c_size_t(0)
        self._check(self._lib.pcr_map_update_all(self._m, float(grid_size), C.byref(n)))
        return n.value

    def updateAllSparse(self, grid_size=0.4):
        """pcr_map_update_all_sparse: updateAll with pcp::VoxelDownSampleV3 in place of pcl::VoxelGrid -- the whole map filtered whatever its extent."""
        n = C.c_size_t(0)
        self._check(self._lib.pcr_map_update_all_sparse(self._m, float(grid_size), C.byref(n)))
        return n.value

    def save(self, directory, first=0, stamps=None, precise=False):
        """pcr_map_save: {directory}/{i}.pcd for key frames first .. end as the store holds them now, and tum.txt for all of them (stamps: one
        per key frame, None: the index).  The default tum.txt rounds to the millimetre and to 1e-6; precise=True writes 17 digits."""
        _keep, sp = _stamps_in(stamps, self.keyframes())
        self._check(self._lib.pcr_map_save(self._m, os.fsencode(directory), int(first), sp, int(bool(precise))))

    def load(self, directory, grid_size=0.0):
        """pcr_map_load into a store without key frames: tum.txt's poses (quaternions as read, not normalised) and {i}.pcd, then with
        grid_size > 0 the in-place filter -> the stamps (one per loaded key frame; empty when there is no tum.txt)."""
        cap = _tum_lines(directory)
        stamps = np.zeros(max(cap, 1))
        n = C.c_size_t(0)
        self._check(self._lib.pcr_map_load(self._m, os.fsencode(directory), float(grid_size), stamps.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(n)))
        return stamps[:n.value].copy()

    def __del__(self):
        try:
            if self._m:
                self._lib.pcr_map_destroy(self._m)
                self._m = None
            self._parent = None
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise PcrError(self._lib.pcr_map_last_error(self._m).decode())

    def addKeyFrame(self, cloud, pose):
        p, n, s, dev, _keep = _cloud(cloud)
        pc = _pose_in(pose)
        self._check(self._lib.pcr_map_add_keyframe(self._m, p, n, s, dev, pc.ctypes.data_as(C.POINTER(C.c_double))))

    def generation(self):
        """(store id, generation of the sub-map it holds): every updateMap / loopFindNearKeyframes / updateAll starts a new generation; a view has an id of its own."""
        i, g = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.pcr_map_generation(self._m, C.byref(i), C.byref(g)))
        return int(i.value), int(g.value)

    def keyframes(self):
        n = C.c_size_t(0)
        self._check(self._lib.pcr_map_keyframes(self._m, C.byref(n)))
        return n.value

    def updateMap(self, position, radius=8.0, grid_size=0.4):
        pos = np.ascontiguousarray(position, np.float64).reshape(3)
        n = C.c_size_t(0)
        self._check(self._lib.pcr_map_update(self._m, pos.ctypes.data_as(C.POINTER(C.c_double)), float(radius), float(grid_size), C.byref(n)))
        return n.value

    def clear(self):
        """pcr_map_clear: forget the key frames and the sub-map, keep the device memory (a new session on a store that has grown)."""
        self._check(self._lib.pcr_map_clear(self._m))

    def updateMapBegin(self, position, radius=8.0, grid_size=0.4):
        """pcr_map_update_begin: select + queue the assembly (the reference's map thread works beside the front end); wait() -- or whatever asks for
        the sub-map first -- collects it."""
        pos = np.ascontiguousarray(position, np.float64).reshape(3)
        self._check(self._lib.pcr_map_update_begin(self._m, pos.ctypes.data_as(C.POINTER(C.c_double)), float(radius), float(grid_size)))

    def wait(self):
        """pcr_map_wait -> points of the sub-map."""
        n = C.c_size_t(0)
        self._check(self._lib.pcr_map_wait(self._m, C.byref(n)))
        return n.value

    def loopFindNearKeyframes(self, key, search_num, grid_size=0.4):
        """LoopClosureManager::loopFindNearKeyframes (backend/src/LoopClosureManager.cpp:40-60): the key frames key +- search_num,
        transformed, concatenated and voxel-filtered, as the device-resident target of the loop-closure registration."""
        n = C.c_size_t(0)
        self._check(self._lib.pcr_map_update_window(self._m, int(key), int(search_num), float(grid_size), C.byref(n)))
        return n.value

    def rankNear(self, first, count, radius, k=1, num_exclude_recent=0):
        """pcr_map_rank_near: key frames against key frames by the distance of their positions, on the device: for every query q of
        [first, first + count) the k nearest candidates of [0, q - num_exclude_recent) with d2 <= radius^2, by (d2, index) ascending
        -> (idx int64, d2 float64), each (count, k), row q - first; the tail is idx -1, d2 DBL_MAX.  Parent or view."""
        first, count, k = int(first), int(count), int(k)
        if first < 0 or count < 0:
            raise PcrError("first and count must not be negative")
        shape = (count, max(k, 0))
        idx, d2 = np.full(shape, -1, np.int64), np.full(shape, np.finfo(np.float64).max)
        self._check(self._lib.pcr_map_rank_near(self._m, first, count, int(num_exclude_recent), float(radius), k,
                                                idx.ctypes.data_as(C.POINTER(C.c_int64)), d2.ctypes.data_as(C.POINTER(C.c_double))))
        return idx, d2

    def pointer(self):
        """-> (device pointer, number of points, stride in bytes) of the assembled sub-map."""
        n, s = C.c_size_t(0), C.c_size_t(0)
        p = self._lib.pcr_map_submap(self._m, C.byref(n), C.byref(s))
        return p, n.value, s.value

    def submapIdx(self):
        n = C.c_size_t(0)
        self._check(self._lib.pcr_map_submap_indices(self._m, None, 0, C.byref(n)))
        idx = np.zeros(n.value, np.int64)
        if n.value:
            self._check(self._lib.pcr_map_submap_indices(self._m, idx.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return idx

    def download(self):
        """The sub-map as a host array (tests, visualisation)."""
        import torch
        p, n, s = self.pointer()
        out = torch.empty((n, s // 4), dtype=torch.float32, device="cuda")
        if n:
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            rc = hip.hipMemcpy(C.c_void_p(out.data_ptr()), C.c_void_p(p), n * s, 3)      # hipMemcpyDeviceToDevice
            if rc:
                raise PcrError(f"hipMemcpy failed: {rc}")
        return out.cpu().numpy()


def kf_rank_near_host(xyz, first, count, radius, k=1, num_exclude_recent=0):
    """pcr_kf_rank_near_host (host only, no GPU): the definition of SubMap.rankNear over positions xyz (n, 3) -> (idx, d2), each (count, k)."""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    first, count, k = int(first), int(count), int(k)
    if first < 0 or count < 0:
        raise PcrError("first and count must not be negative")
    shape = (count, max(k, 0))
    idx, d2 = np.full(shape, -1, np.int64), np.full(shape, np.finfo(np.float64).max)
    if load_library().pcr_kf_rank_near_host(xyz.ctypes.data_as(C.POINTER(C.c_double)), xyz.shape[0], first, count, int(num_exclude_recent), float(radius), k,
                                            idx.ctypes.data_as(C.POINTER(C.c_int64)), d2.ctypes.data_as(C.POINTER(C.c_double))):
        raise PcrError("pcr_kf_rank_near_host: refused")
    return idx, d2


def deskew_motion(poses, stamps, t0=0.0, t_ref=0.0):
    """-> (pcr_deskew_motion, keepalive): control poses (K, 4, 4) at stamps (K,), the offset t0 of every point time and the reference time."""
    P = np.asarray(poses, dtype=np.float64)
    if P.ndim != 3 or P.shape[1:] != (4, 4):
        raise ValueError("poses must have shape (K, 4, 4)")
    cm = np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(-1).copy()      # column-major, one pose after the other
    st = np.ascontiguousarray(np.asarray(stamps, dtype=np.float64).reshape(-1)).copy()
    if st.shape[0] != P.shape[0]:
        raise ValueError("one stamp per control pose")
    dp = C.POINTER(C.c_double)
    return DeskewMotion(cm.ctypes.data_as(dp), st.ctypes.data_as(dp), P.shape[0], float(t0), float(t_ref)), (cm, st)


def _deskew_times(times, time_kind, n, on_device):
    """-> (pointer or None, keepalive) of a packed time array that lives where the cloud lives."""
    if times is None:
        return None, None
    if time_kind not in _TIME_DTYPES:
        raise ValueError("time_kind must be TIME_F32_SECONDS, TIME_U32_NANOSECONDS or TIME_F64_SECONDS")
    if hasattr(times, "data_ptr"):
        if not (times.is_cuda and on_device):
            raise ValueError("times must live where the cloud lives")
        if times.numel() != n or not times.is_contiguous() or times.element_size() != np.dtype(_TIME_DTYPES[time_kind]).itemsize:
            raise ValueError("times must be a contiguous array of n elements of the time kind")
        return C.c_void_p(times.data_ptr()), times
    if on_device:
        raise ValueError("times must live where the cloud lives")
    t = np.ascontiguousarray(np.asarray(times).reshape(-1), dtype=_TIME_DTYPES[time_kind])
    if t.shape[0] != n:
        raise ValueError("one time per point")
    return t.ctypes.data_as(C.c_void_p), t


def _deskew_info(i):
    return dict(before=int(i.before), after=int(i.after), nonfinite=int(i.nonfinite), ref_clamped=int(i.ref_clamped))


def deskew_host(cloud, poses, stamps, times=None, time_kind=TIME_F32_SECONDS, time_offset=0, t0=0.0, t_ref=0.0, out=None):
    """pcr_deskew_host (host only, no GPU; the definition of deskew): every point of `cloud` (numpy (n, >= 4) float32) moved from the sensor frame at
    its own time into the sensor frame at t_ref, the sensor's motion given by control `poses` (K, 4, 4) at `stamps`.  times: a packed array of
    the kind, or None for the field at byte `time_offset` of every record.  out: None (a new array), or a float32 array of the cloud's shape --
    the cloud itself deskews in place.  -> (out, info dict: before, after, nonfinite, ref_clamped)."""
    p, n, s, dev, keep = _cloud(cloud)
    if dev:
        raise ValueError("deskew_host takes host arrays")
    if out is None:
        out = np.zeros_like(keep)
    if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == keep.shape and out.flags.c_contiguous):
        raise ValueError("out must be a contiguous float32 array of the cloud's shape")
    tp, _tk = _deskew_times(times, time_kind, n, 0)
    m, _mk = deskew_motion(poses, stamps, t0, t_ref)
    info = DeskewInfo()
    L = load_library()
    if L.pcr_deskew_host(p, n, s, tp, int(time_kind), int(time_offset), C.byref(m), out.ctypes.data_as(C.c_void_p), C.byref(info)):
        raise PcrError(L.pcr_last_error(None).decode())
    return out, _deskew_info(info)


def deskew(register, cloud, poses, stamps, times=None, time_kind=TIME_F32_SECONDS, time_offset=0, t0=0.0, t_ref=0.0, out=None):
    """pcr_deskew on `register`'s handle (any method): deskew_host on the device, bit for bit.  cloud (and times) numpy arrays or CUDA tensors;
    out: None -- a new array or tensor like the cloud --, or a float32 numpy array / CUDA tensor of the cloud's shape (the cloud itself: in
    place).  A CUDA cloud deskewed into a CUDA tensor never leaves HBM.  -> (out, info dict)."""
    p, n, s, dev, keep = _cloud(cloud)
    if out is None:
        if dev:
            import torch
            out = torch.empty_like(keep)
        else:
            out = np.zeros_like(keep)
    op, on, os_, odev, _ok = _cloud(out)
    if (on, os_) != (n, s):
        raise ValueError("out must have the cloud's shape")
    tp, _tk = _deskew_times(times, time_kind, n, dev)
    m, _mk = deskew_motion(poses, stamps, t0, t_ref)
    info = DeskewInfo()
    register._check(register._lib.pcr_deskew(register._h, p, n, s, dev, tp, int(time_kind), int(time_offset), C.byref(m), op, odev, C.byref(info)))
    return out, _deskew_info(info)


def pose_to_mobile(T):
    """pcr_pose_to_mobile (host only): trans::SixDof2Mobile (common/geometry/trans.hpp:68-86) -- x, y and the rotation about Z; the heading is
    dropped when the rotation's axis is not within |axis.z| > 0.95 of Z, as in the reference.  -> a new 4x4."""
    c = _pose_in(T)
    out = np.zeros(16)
    dp = C.POINTER(C.c_double)
    if load_library().pcr_pose_to_mobile(c.ctypes.data_as(dp), out.ctypes.data_as(dp)) != 0:
        raise PcrError("pcr_pose_to_mobile failed")
    return _pose_out(out)


def frontend_default_params():
    p = FrontendParams()
    load_library().pcr_frontend_default_params(C.byref(p))
    return p


class Frontend:
    """The per-scan loop of the reference's front end around scan2Map, in the library (pcr_frontend_*): voxel filter -> scan2Map against the sub-map ->
    SixDof2Mobile (mobile=True) -> setCurPose -> putKeyFrame -> updateMap, queued.  sequence.drive() over sequence.GpuFront is the same loop in Python;
    sequence.drive_frontend() drives this one.  The register and the sub-map are borrowed (and kept alive by this object)."""

    _INFO_INTS = ("registered", "converged", "iterations", "keyframe_added", "update_queued", "n_filtered", "n_submap", "keyframes", "updates")
    STEPS = ("voxel", "wait", "scan2map", "add_keyframe", "update_map")      # pcr_frontend_info.seconds

    def __init__(self, register, submap=None, grid=0.5, radius=8.0, kf_gap=1.0, mobile=False):
        self._lib = load_library()
        self._fe = None
        self.reg = register
        self.map = submap or SubMap()
        p = FrontendParams(float(grid), float(radius), float(kf_gap), 1 if mobile else 0)
        self._fe = self._lib.pcr_frontend_create(register._h, self.map._m, C.byref(p))
        if not self._fe:
            raise PcrError(self._lib.pcr_frontend_last_error(None).decode())
        # (per-call marshalling kept off the hot path, as in PointCloudRegister: persistent pose buffers and info block)
        self._in_buf, self._out_buf = (C.c_double * 16)(), (C.c_double * 16)()
        self._in_cm = np.frombuffer(self._in_buf, dtype=np.float64).reshape(4, 4)       # column-major 4x4 = transposed view
        self._out_cm = np.frombuffer(self._out_buf, dtype=np.float64).reshape(4, 4)
        self._info = FrontendInfo()
        self._info_ref = C.byref(self._info)

    def __del__(self):
        try:
            if self._fe:
                self._lib.pcr_frontend_destroy(self._fe)
                self._fe = None
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise PcrError(self._lib.pcr_frontend_last_error(self._fe).decode())

    def step(self, scan, init_pose):
        """pcr_frontend_step: one scan from `init_pose` (previous pose o odometry: the caller's) -> (pose 4x4, info dict: the fields of
        pcr_frontend_info, `seconds` as a dict by step name)."""
        p, n, s, dev, _keep = self.reg._cloud_cached(scan)
        T = np.asarray(init_pose, dtype=np.float64)
        if T.shape != (4, 4):
            raise ValueError("pose must be 4x4")
        self._in_cm[...] = T.T
        self._check(self._lib.pcr_frontend_step(self._fe, p, n, s, dev, self._in_buf, self._out_buf, self._info_ref))
        i = self._info
        info = {f: int(getattr(i, f)) for f in self._INFO_INTS}
        info["seconds"] = dict(zip(self.STEPS, i.seconds))
        return self._out_cm.T.copy(), info

    def stepTimed(self, scan, init_pose, poses, stamps, times=None, time_kind=TIME_F32_SECONDS, time_offset=0, t0=0.0, t_ref=0.0):
        """pcr_frontend_step_timed: deskew() of the scan into a device buffer of the front end's, then step() on that buffer (the key frame is
        the deskewed scan).  -> (pose 4x4, info dict as step(), with the deskew's counts under "deskew")."""
        p, n, s, dev, _keep = self.reg._cloud_cached(scan)
        tp, _tk = _deskew_times(times, time_kind, n, dev)
        m, _mk = deskew_motion(poses, stamps, t0, t_ref)
        T = np.asarray(init_pose, dtype=np.float64)
        if T.shape != (4, 4):
            raise ValueError("pose must be 4x4")
        self._in_cm[...] = T.T
        dinfo = DeskewInfo()
        self._check(self._lib.pcr_frontend_step_timed(self._fe, p, n, s, dev, tp, int(time_kind), int(time_offset), C.byref(m), self._in_buf, self._out_buf,
                                                      self._info_ref, C.byref(dinfo)))
        i = self._info
        info = {f: int(getattr(i, f)) for f in self._INFO_INTS}
        info["seconds"] = dict(zip(self.STEPS, i.seconds))
        info["deskew"] = _deskew_info(dinfo)
        return self._out_cm.T.copy(), info

    def prefetch(self, scan):
        """pcr_frontend_prefetch: queue the voxel filter of a scan that a LATER step takes (the same object must be passed to that step)."""
        p, n, s, dev, _keep = self.reg._cloud_cached(scan)
        self._check(self._lib.pcr_frontend_prefetch(self._fe, p, n, s, dev))

    def finish(self):
        """pcr_frontend_finish: collect a queued assembly -> points of the sub-map."""
        n = C.c_size_t(0)
        self._check(self._lib.pcr_frontend_finish(self._fe, C.byref(n)))
        return n.value

    def reset(self):
        """pcr_frontend_reset: a new session on the same handles (key frames, sub-map and the loop's state forgotten, device memory kept)."""
        self._check(self._lib.pcr_frontend_reset(self._fe))

    def closest(self):
        """pcr_frontend_closest -> int64 array, one entry per key frame this front end added: the key frame nearest to it when it was added
        (mClosestKfIdx, the `from` of Backend::addOdomFactor's edge), -1 for the first."""
        n = C.c_size_t(0)
        self._check(self._lib.pcr_frontend_closest(self._fe, None, 0, C.byref(n)))
        idx = np.zeros(n.value, np.int64)
        if n.value:
            self._check(self._lib.pcr_frontend_closest(self._fe, idx.ctypes.data_as(C.POINTER(C.c_int64)), n.value, C.byref(n)))
        return idx


class ScanContext:
    """context::ScanContext (backend/include/backend/ScanContext.hpp, backend/src/ScanContext.cpp): addContext(scan) builds the
    20 x 60 polar descriptor on the device; query(id) -> (match id or -1, yaw in rad), QueryResult of the reference."""

    def __init__(self, device=-1, **params):
        self._lib = load_library()
        p = ScParams()
        self._lib.pcr_sc_default_params(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise ValueError(f"unknown ScanContext parameter {k}")
            setattr(p, k, v)
        self._height = float(p.lidar_height)
        self._dist_thres = float(np.float32(p.dist_thres))            # the reference keeps scDistThres as a float
        self._s = self._lib.pcr_sc_create(int(device), C.byref(p))
        if not self._s:
            raise PcrError(self._lib.pcr_sc_last_error(None).decode())

    def __del__(self):
        try:
            if self._s:
                self._lib.pcr_sc_destroy(self._s)
                self._s = None
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise PcrError(self._lib.pcr_sc_last_error(self._s).decode())

    def addContext(self, cloud):
        p, n, s, dev, _keep = _cloud(cloud)
        self._check(self._lib.pcr_sc_add(self._s, p, n, s, dev))

    def addKeyFrames(self, submap, first=0, count=None, grid_size=0.0):
        """pcr_sc_add_keyframes: one context per stored key frame of [first, first + count) of a SubMap or a view of one (count=None: to the
        last one), in one batched pass on the device -- what keyFramePointer -> voxelDownSample(grid_size) -> addContext leaves for each,
        bit for bit; grid_size <= 0 bins the stored points as they are.  -> the number of contexts added."""
        first = int(first)
        if count is None:
            count = max(submap.keyframes() - first, 0) if submap is not None else 0      # (a missing map, a first past the end: the library's to refuse)
        count = int(count)
        if first < 0 or count < 0:
            raise PcrError("first and count must not be negative")
        n = C.c_size_t(0)
        self._check(self._lib.pcr_sc_add_keyframes(self._s, submap._m if submap is not None else None, first, count, float(grid_size), C.byref(n)))
        return n.value

    def __len__(self):
        n = C.c_size_t(0)
        self._check(self._lib.pcr_sc_size(self._s, C.byref(n)))
        return n.value

    def descriptor(self, i):
        """-> (20 x 60 descriptor, ring key, sector key)"""
        d, rk, sk = np.zeros((20, 60)), np.zeros(20), np.zeros(60)
        self._check(self._lib.pcr_sc_descriptor(self._s, int(i), d.ctypes.data_as(C.c_void_p), rk.ctypes.data_as(C.c_void_p), sk.ctypes.data_as(C.c_void_p)))
        return d, rk, sk

    def distance(self, i, j):
        d, sh = C.c_double(0), C.c_int(0)
        self._check(self._lib.pcr_sc_distance(self._s, int(i), int(j), C.byref(d), C.byref(sh)))
        return d.value, sh.value

    def distances(self, cloud):
        """distanceBtnScanContext of `cloud` (lidar frame; not added) against every stored context, on the device
        -> (dist float64[M], shift int32[M]): entry i is distance(q, i) had the cloud been added as context q."""
        p, n, s, dev, _keep = _cloud(cloud)
        m = len(self)
        dist, shift = np.zeros(m, np.float64), np.zeros(m, np.int32)
        self._check(self._lib.pcr_sc_distances(self._s, p, n, s, dev, dist.ctypes.data_as(C.POINTER(C.c_double)),
                                               shift.ctypes.data_as(C.POINTER(C.c_int32))))
        return dist, shift

    def query(self, i):
        """-> (match or -1, yaw as float32, best candidate distance or None when the search did not run)"""
        m, yaw, d = C.c_longlong(-1), C.c_float(0), C.c_double(0)
        self._check(self._lib.pcr_sc_query(self._s, int(i), C.byref(m), C.byref(yaw), C.byref(d)))
        return m.value, np.float32(yaw.value), (None if d.value == np.finfo(np.float64).max else d.value)

    def rankStored(self, first, count, k=1):
        """Stored contexts against stored contexts, on the device (pcr_sc_rank_stored): for every query q of [first, first + count)
        the k best candidates i of [0, q - num_exclude_recent) by (distance(q, i), i) ascending
        -> (idx int64, dist float64, shift int32), each (count, k), row q - first; the tail where fewer than k candidates exist is
        idx -1, dist DBL_MAX, shift 0.  The threshold is not applied."""
        first, count, k = int(first), int(count), int(k)
        shape = (max(count, 0), max(k, 0))
        idx, dist, shift = np.full(shape, -1, np.int64), np.full(shape, np.finfo(np.float64).max), np.zeros(shape, np.int32)
        if first < 0 or count < 0:
            raise PcrError("first and count must not be negative")
        self._check(self._lib.pcr_sc_rank_stored(self._s, first, count, k, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 dist.ctypes.data_as(C.POINTER(C.c_double)), shift.ctypes.data_as(C.POINTER(C.c_int32))))
        return idx, dist, shift

    def findLoops(self, first=0, count=None):
        """LoopClosureManager::lcHandler's walk over key frames [first, first + count) (count=None: to the last one) in one call: per
        query (id, match, yaw as float32, min_dist) from the k = 1 ranking.  match = -1, yaw = 0 when there is no candidate (min_dist
        None) or min_dist > dist_thres; otherwise yaw = deg2rad(6 * shift) as query forms it."""
        first = int(first)
        count = len(self) - first if count is None else int(count)
        idx, dist, shift = self.rankStored(first, count, 1)
        out = []
        for r in range(count):
            i, d, s = int(idx[r, 0]), float(dist[r, 0]), int(shift[r, 0])
            if i < 0:
                out.append((first + r, -1, np.float32(0), None))
            elif d > self._dist_thres:
                out.append((first + r, -1, np.float32(0), d))
            else:
                out.append((first + r, i, np.float32(self._lib.pcr_sc_shift_yaw(s)), d))
        return out


GRAPH_HOST = -2                                   # PCR_GRAPH_HOST: a graph without a device (no optimize)
GRAPH_PRIOR, GRAPH_ODOM, GRAPH_LOOP = 0, 1, 2     # pcr_graph_noise kinds
GRAPH_PRECOND_BLOCK_JACOBI, GRAPH_PRECOND_TREE = 0, 1      # PCR_GRAPH_PRECOND_*: pcr_graph_params.pcg_preconditioner
_GRAPH_PRECOND = {"block_jacobi": GRAPH_PRECOND_BLOCK_JACOBI, "tree": GRAPH_PRECOND_TREE}


def _graph_precond(kind):
    """a PCR_GRAPH_PRECOND_* value, or one of the strings "block_jacobi" and "tree" """
    if isinstance(kind, str):
        if kind not in _GRAPH_PRECOND:
            raise ValueError(f"unknown preconditioner {kind!r}: one of {sorted(_GRAPH_PRECOND)}")
        return _GRAPH_PRECOND[kind]
    return int(kind)


GRAPH_ROBUST_NONE, GRAPH_ROBUST_HUBER, GRAPH_ROBUST_GEMAN_MCCLURE, GRAPH_ROBUST_TUKEY = 0, 1, 2, 3      # PCR_GRAPH_ROBUST_*
_GRAPH_ROBUST = {"none": GRAPH_ROBUST_NONE, "huber": GRAPH_ROBUST_HUBER, "geman_mcclure": GRAPH_ROBUST_GEMAN_MCCLURE, "tukey": GRAPH_ROBUST_TUKEY}


def _graph_robust(kind):
    """a PCR_GRAPH_ROBUST_* value, or one of the strings "none", "huber", "geman_mcclure" and "tukey" """
    if isinstance(kind, str):
        if kind not in _GRAPH_ROBUST:
            raise ValueError(f"unknown robust kernel {kind!r}: one of {sorted(_GRAPH_ROBUST)}")
        return _GRAPH_ROBUST[kind]
    return int(kind)


def graph_robust_rho_w(kind, delta, s):
    """pcr_graph_robust_rho_w -> (rho(s), w(s)) by the function the linearise kernel compiles (host code)."""
    rho, w = C.c_double(0), C.c_double(0)
    if load_library().pcr_graph_robust_rho_w(_graph_robust(kind), float(delta), float(s), C.byref(rho), C.byref(w)):
        raise PcrError(f"pcr_graph_robust_rho_w: refused (kind {kind}, delta {delta}, s {s})")
    return rho.value, w.value


def graph_noise(kind):
    """pcr_graph_noise -> the 6 x 6 information matrix of one of the reference's noise models (Backend.cpp:90-97), [omega; v] order."""
    buf = np.zeros(21)
    if load_library().pcr_graph_noise(int(kind), buf.ctypes.data_as(C.POINTER(C.c_double))):
        raise PcrError(f"unknown noise kind {kind}")
    return _info_full(buf)


def _info21(info):
    a = np.asarray(info, dtype=np.float64)
    if a.shape == (6, 6):
        a = a[np.triu_indices(6)]
    if a.shape != (21,):
        raise ValueError("an information matrix is 6 x 6, or its 21 upper-triangular entries")
    return np.ascontiguousarray(a)


def _info_full(info21):
    m = np.zeros((6, 6))
    m[np.triu_indices(6)] = info21
    return m + np.triu(m, 1).T


class GraphResultView:
    """What PoseGraph.optimize() returns: pcr_graph_result with delta as a 4 x 4 matrix."""

    def __init__(self, r):
        self.iterations, self.accepted, self.pcg_iterations, self.pcg_capped = int(r.iterations), int(r.accepted), int(r.pcg_iterations), int(r.pcg_capped)
        self.converged = bool(r.converged)
        self.chi2_initial, self.chi2_final, self.lambda_ = float(r.chi2_initial), float(r.chi2_final), float(r.lambda_)
        self.delta = _pose_out(np.array(r.delta[:], dtype=np.float64))

    def __repr__(self):
        return (f"GraphResult(iterations={self.iterations}, accepted={self.accepted}, pcg_iterations={self.pcg_iterations}, pcg_capped={self.pcg_capped}, "
                f"converged={self.converged}, chi2_initial={self.chi2_initial:.6g}, chi2_final={self.chi2_final:.6g}, lambda_={self.lambda_:.3g})")


class PoseGraph:
    """Backend::Gtsam and Backend::optimHandler (backend/src/Backend.cpp:85-103, 224-347) on the device: an SE(3) pose graph of prior and
    between factors, Levenberg-Marquardt over a conjugate gradient that runs on the GPU (pcr_graph).  Poses are 4 x 4;
    information matrices are 6 x 6 in [omega; v] order (or their 21 upper-triangular entries); None takes the reference's preset.
    device=GRAPH_HOST builds a graph that touches no device: everything but optimize() and apply()."""

    def __init__(self, device=-1):
        self._lib = load_library()
        self._g = self._lib.pcr_graph_create(int(device))
        if not self._g:
            raise PcrError(self._lib.pcr_graph_last_error(None).decode())

    def __del__(self):
        try:
            if self._g:
                self._lib.pcr_graph_destroy(self._g)
                self._g = None
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise PcrError(self._lib.pcr_graph_last_error(self._g).decode())

    def _noise(self, kind, info):
        buf = np.zeros(21)
        if info is None:
            self._lib.pcr_graph_noise(kind, buf.ctypes.data_as(C.POINTER(C.c_double)))
        else:
            buf = _info21(info)
        return buf, buf.ctypes.data_as(C.POINTER(C.c_double))

    def addPoses(self, poses):
        """pcr_graph_add_poses: (k, 4, 4); their ids continue the graph's."""
        P = np.asarray(poses, dtype=np.float64)
        if P.ndim == 2:
            P = P[None]
        if P.ndim != 3 or P.shape[1:] != (4, 4):
            raise ValueError("poses must have shape (k, 4, 4)")
        cm = np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(-1)
        self._check(self._lib.pcr_graph_add_poses(self._g, cm.ctypes.data_as(C.POINTER(C.c_double)), P.shape[0]))

    def addEstimate(self, id, pose):
        if int(id) != self.size()[0]:
            raise PcrError("addEstimate: ids are consecutive from 0")
        self.addPoses(pose)

    def addPrior(self, pose, id=0, info=None):
        _k, ip = self._noise(GRAPH_PRIOR, info)
        pc = _pose_in(pose)
        self._check(self._lib.pcr_graph_add_prior(self._g, int(id), pc.ctypes.data_as(C.POINTER(C.c_double)), ip))

    def _between(self, kind, frm, to, between, info):
        _k, ip = self._noise(kind, info)
        pc = _pose_in(between)
        if int(frm) < 0 or int(to) < 0:
            raise PcrError("ids must not be negative")
        self._check(self._lib.pcr_graph_add_between(self._g, int(frm), int(to), pc.ctypes.data_as(C.POINTER(C.c_double)), ip))

    def addBetween(self, frm, to, between, info=None):
        self._between(GRAPH_ODOM, frm, to, between, info)

    def addLC(self, frm, to, between, info=None):
        """pcr_graph_add_loop: a between factor with the LOOP preset that carries the robust mark (under kernel "none" the mark changes nothing)."""
        _k, ip = self._noise(GRAPH_LOOP, info)
        pc = _pose_in(between)
        if int(frm) < 0 or int(to) < 0:
            raise PcrError("ids must not be negative")
        self._check(self._lib.pcr_graph_add_loop(self._g, int(frm), int(to), pc.ctypes.data_as(C.POINTER(C.c_double)), ip))

    def setRobustKernel(self, kind, delta=0.0):
        """pcr_graph_set_robust_kernel: GRAPH_ROBUST_* or "none", "huber", "geman_mcclure", "tukey"; delta in units of a residual's Mahalanobis length."""
        self._check(self._lib.pcr_graph_set_robust_kernel(self._g, _graph_robust(kind), float(delta)))

    def robustKernel(self):
        """-> (kind, delta)"""
        k, d = C.c_int(0), C.c_double(0)
        self._check(self._lib.pcr_graph_get_robust_kernel(self._g, C.byref(k), C.byref(d)))
        return k.value, d.value

    def setBetweenRobust(self, first, count=1, on=True):
        """pcr_graph_set_between_robust: by index among the between factors, in the order added."""
        self._check(self._lib.pcr_graph_set_between_robust(self._g, int(first), int(count), 1 if on else 0))

    def setBetweenEnabled(self, first, count=1, on=True):
        """pcr_graph_set_between_enabled: a factor that is off adds nothing and links nothing; it stays in size(), linearize()'s r and J, saveG2o()."""
        self._check(self._lib.pcr_graph_set_between_enabled(self._g, int(first), int(count), 1 if on else 0))

    def setFixed(self, first, count=1, on=True):
        """pcr_graph_set_fixed: poses first .. first+count-1 become constants of the problem (on=False frees them): optimize() moves the free
        poses only and hands the fixed ones back bit for bit.  A fixed pose anchors its component as a prior does."""
        if int(first) < 0 or int(count) < 0:
            raise PcrError("pcr_graph_set_fixed: first and count must not be negative")
        self._check(self._lib.pcr_graph_set_fixed(self._g, int(first), int(count), 1 if on else 0))

    def fixed(self):
        """pcr_graph_fixed -> (poses,) bool array: which poses are fixed."""
        n = self.size()[0]
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self._lib.pcr_graph_fixed(self._g, 0, n, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out[:n].astype(bool)

    def betweenWeights(self, first=0, count=None):
        """pcr_graph_between_weights -> (s, w, robust, enabled) per between factor at the current estimates: s = r^T Omega r, the kernel's
        weight at s (1 when unmarked), the mark and the switch as bool arrays."""
        if count is None:
            count = max(self.size()[2] - int(first), 0)
        n = max(int(count), 1)
        s, w, rb, en = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        d, u = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        self._check(self._lib.pcr_graph_between_weights(self._g, int(first), int(count), s.ctypes.data_as(d), w.ctypes.data_as(d), rb.ctypes.data_as(u),
                                                        en.ctypes.data_as(u)))
        c = int(count)
        return s[:c], w[:c], rb[:c].astype(bool), en[:c].astype(bool)

    def addOdomFactor(self, frm, to, info=None):
        """Backend::addOdomFactor: the between factor of the two current estimates."""
        _k, ip = self._noise(GRAPH_ODOM, info)
        if int(frm) < 0 or int(to) < 0:
            raise PcrError("ids must not be negative")
        self._check(self._lib.pcr_graph_add_between_poses(self._g, int(frm), int(to), ip))

    def size(self):
        """-> (poses, priors, between factors)"""
        a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pcr_graph_size(self._g, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def clear(self):
        self._check(self._lib.pcr_graph_clear(self._g))

    def optimize(self, **params):
        """pcr_graph_optimize with pcr_graph_params fields overridden (max_iterations, rel_tol, abs_tol, lambda_init, lambda_factor, lambda_max,
        pcg_max_iterations, pcg_rel_tol, pcg_preconditioner -- GRAPH_PRECOND_BLOCK_JACOBI (the default) or GRAPH_PRECOND_TREE, or the strings
        "block_jacobi" and "tree"; the tree serves an odometry tree with few loops at thousands of poses) -> GraphResultView."""
        p = GraphParams()
        self._lib.pcr_graph_default_params(C.byref(p))
        for k, v in params.items():
            if k == "struct_size" or not hasattr(p, k):
                raise ValueError(f"unknown pose-graph parameter {k}")
            setattr(p, k, _graph_precond(v) if k == "pcg_preconditioner" else v)
        r = GraphResult()
        self._check(self._lib.pcr_graph_optimize(self._g, C.byref(p), C.byref(r)))
        return GraphResultView(r)

    def poses(self, first=0, count=None):
        """-> (count, 4, 4), the current estimates."""
        n = self.size()[0]
        if count is None:
            count = max(n - int(first), 0)
        buf = np.zeros(16 * max(int(count), 1))
        self._check(self._lib.pcr_graph_poses(self._g, int(first), int(count), buf.ctypes.data_as(C.POINTER(C.c_double))))
        return buf[:16 * int(count)].reshape(-1, 4, 4).transpose(0, 2, 1).copy()

    def devicePoses(self):
        """pcr_graph_device_poses -> (device pointer, number of poses)"""
        n = C.c_size_t(0)
        p = self._lib.pcr_graph_device_poses(self._g, C.byref(n))
        return p, n.value

    def linearize(self):
        """pcr_graph_linearize -> (r (E, 6), J_from (E, 6, 6), J_to (E, 6, 6), chi2), priors first, then the between factors."""
        _n, a, b = self.size()
        E = a + b
        r, jf, jt, c = np.zeros((max(E, 1), 6)), np.zeros((max(E, 1), 6, 6)), np.zeros((max(E, 1), 6, 6)), C.c_double(0)
        d = C.POINTER(C.c_double)
        self._check(self._lib.pcr_graph_linearize(self._g, r.ctypes.data_as(d), jf.ctypes.data_as(d), jt.ctypes.data_as(d), C.byref(c)))
        return r[:E], jf[:E], jt[:E], c.value

    def apply(self, lam, x):
        """pcr_graph_apply -> y = (H + lam I) x, x of 6 entries per pose."""
        n = self.size()[0]
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
        if x.size != 6 * n:
            raise ValueError("x must hold 6 entries per pose")
        y = np.zeros(max(6 * n, 1))
        d = C.POINTER(C.c_double)
        self._check(self._lib.pcr_graph_apply(self._g, float(lam), x.ctypes.data_as(d), y.ctypes.data_as(d)))
        return y[:6 * n]

    def tree(self):
        """pcr_graph_tree -> (parent (poses,) int64 with -1 at the roots, between factors in the forest, the others): the spanning forest of
        the tree preconditioner.  Host code: it serves a GRAPH_HOST graph."""
        n = self.size()[0]
        parent = np.full(max(n, 1), -1, dtype=np.int64)
        a, b = C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pcr_graph_tree(self._g, parent.ctypes.data_as(C.POINTER(C.c_int64)), n, C.byref(a), C.byref(b)))
        return parent[:n], a.value, b.value

    def precondition(self, lam, r, kind=GRAPH_PRECOND_TREE):
        """pcr_graph_precondition -> z = M^-1 r at the current estimates, r of 6 entries per pose, by the solve's own factorisation and sweeps."""
        n = self.size()[0]
        r = np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1))
        if r.size != 6 * n:
            raise ValueError("r must hold 6 entries per pose")
        z = np.zeros(max(6 * n, 1))
        d = C.POINTER(C.c_double)
        self._check(self._lib.pcr_graph_precondition(self._g, float(lam), _graph_precond(kind), r.ctypes.data_as(d), z.ctypes.data_as(d)))
        return z[:6 * n]

    def applyTo(self, submap, first=0, count=None):
        """pcr_map_set_poses_from_graph (Backend.cpp:315-318): the estimates become the key frames' poses."""
        if count is None:
            count = max(self.size()[0] - int(first), 0)
        if self._lib.pcr_map_set_poses_from_graph(submap._m, self._g, int(first), int(count)):
            raise PcrError(self._lib.pcr_map_last_error(submap._m).decode())

    def loadG2o(self, path):
        self._check(self._lib.pcr_graph_load_g2o(self._g, os.fsencode(path)))

    def saveG2o(self, path):
        self._check(self._lib.pcr_graph_save_g2o(self._g, os.fsencode(path)))


BACKEND_SC_QUERY, BACKEND_SC_RANK, BACKEND_DISTANCE = 1, 2, 4      # PCR_BACKEND_*: pcr_backend_params.detectors
LC_VGICP, LC_GICP = 0, 1                                           # PCR_VGICP, PCR_GICP: pcr_backend_params.lc_method
_LC_METHOD = {"vgicp": LC_VGICP, "gicp": LC_GICP}


def backend_default_params():
    p = BackendParams()
    load_library().pcr_backend_default_params(C.byref(p))
    return p


def _borrowed(cls, owner, **fields):
    """An object of `cls` over a handle that `owner` owns: its methods work, it keeps the owner alive and destroys nothing."""
    class Borrowed(cls):
        def __del__(self):
            pass

        def close(self):
            pass
    Borrowed.__name__ = cls.__name__
    o = Borrowed.__new__(Borrowed)
    o._lib = load_library()
    o._owner = owner
    o.__dict__.update(fields)
    return o


class Backend:
    """The back end's key-frame and loop-closure loop in the library (pcr_backend_*): Backend::optimHandler's NewKFCome and LC events and
    LoopClosureManager::lcHandler over a SubMap (borrowed, a parent) -- contexts from the raw key frames, saveKfs, prior / poses / odometry
    factors, optimise, poses back into the store; loop candidates from ScanContext and / or the distance ranking, verified by VGICP or GICP
    against the history window, accepted ones as loop factors, optimise again.  Keyword arguments are pcr_backend_params fields
    (lc_method also as "vgicp" / "gicp"); sc=dict(...) and graph=dict(...) override fields of the nested pcr_sc_params / pcr_graph_params."""

    STEPS = ("contexts", "downsample", "factors", "detect", "window", "scan2map", "fitness", "optimize", "set_poses")      # pcr_backend_info.seconds
    _INFO_INTS = ("keyframes", "contexts", "keyframes_added", "candidates", "accepted", "factors_added", "optimized")

    def __init__(self, submap, sc=None, graph=None, **params):
        self._lib = load_library()
        self._be = None
        self.map = submap
        p = backend_default_params()
        for k, v in params.items():
            if k in ("sc", "graph", "pad_") or not hasattr(p, k):
                raise ValueError(f"unknown back-end parameter {k}")
            setattr(p, k, _LC_METHOD[v] if k == "lc_method" and isinstance(v, str) else v)
        for k, v in (sc or {}).items():
            if not hasattr(p.sc, k):
                raise ValueError(f"unknown ScanContext parameter {k}")
            setattr(p.sc, k, v)
        for k, v in (graph or {}).items():
            if k == "struct_size" or not hasattr(p.graph, k):
                raise ValueError(f"unknown pose-graph parameter {k}")
            setattr(p.graph, k, _graph_precond(v) if k == "pcg_preconditioner" else v)
        self.params = p
        self._be = self._lib.pcr_backend_create(submap._m, C.byref(p))
        if not self._be:
            raise PcrError(self._lib.pcr_backend_last_error(None).decode())

    def __del__(self):
        try:
            if self._be:
                self._lib.pcr_backend_destroy(self._be)
                self._be = None
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise PcrError(self._lib.pcr_backend_last_error(self._be).decode())

    @property
    def graph(self):
        """pcr_backend_graph as a PoseGraph (borrowed)."""
        return _borrowed(PoseGraph, self, _g=self._lib.pcr_backend_graph(self._be))

    @property
    def sc(self):
        """pcr_backend_sc as a ScanContext (borrowed; pcr_backend_reset replaces the handle, so ask again after a reset)."""
        return _borrowed(ScanContext, self, _s=self._lib.pcr_backend_sc(self._be), _height=float(self.params.sc.lidar_height),
                         _dist_thres=float(np.float32(self.params.sc.dist_thres)))

    @property
    def register(self):
        """pcr_backend_register as a VgicpRegister / GicpRegister (borrowed)."""
        h = self._lib.pcr_backend_register(self._be)
        prm = PcrParams()
        self._lib.pcr_get_params(h, C.byref(prm))
        buf, conv = (C.c_double * 16)(), C.c_int(0)
        return _borrowed(GicpRegister if self.params.lc_method == LC_GICP else VgicpRegister, self, _h=h, params=prm, isConverge=False, _pose_buf=buf,
                         _pose_cm=np.frombuffer(buf, dtype=np.float64).reshape(4, 4), _conv=conv, _conv_ref=C.byref(conv), _seen={})

    def _info(self, i):
        out = {f: int(getattr(i, f)) for f in self._INFO_INTS}
        out["graph"] = GraphResultView(i.graph)
        out["delta"] = _pose_out(np.array(i.delta[:], dtype=np.float64))
        out["seconds"] = dict(zip(self.STEPS, i.seconds))
        return out

    @staticmethod
    def _closest(closest):
        if closest is None:
            return None, None, 0
        a = np.ascontiguousarray(closest, dtype=np.int64).reshape(-1)
        return a, a.ctypes.data_as(C.POINTER(C.c_int64)), a.size

    def addKeyFrames(self, closest=None):
        """pcr_backend_add_keyframes: the NewKFCome event for the key frames the store has gained.  closest: Frontend.closest()'s entries for
        exactly those key frames (None: every odometry edge from i - 1) -> info dict (delta 4x4, graph: GraphResultView, seconds by step)."""
        _keep, ptr, n = self._closest(closest)
        i = BackendInfo()
        self._check(self._lib.pcr_backend_add_keyframes(self._be, ptr, n, C.byref(i)))
        return self._info(i)

    def closeLoops(self):
        """pcr_backend_close_loops: lcHandler over the contexts not yet walked, then the LC event when a loop was accepted -> info dict."""
        i = BackendInfo()
        self._check(self._lib.pcr_backend_close_loops(self._be, C.byref(i)))
        return self._info(i)

    def loops(self):
        """pcr_backend_loops -> the candidate records of the last closeLoops(): list of dict(cur, old, detector, converged, iterations,
        accepted, fitness, pose 4x4)."""
        n = C.c_size_t(0)
        self._check(self._lib.pcr_backend_loops(self._be, None, 0, C.byref(n)))
        raw = (BackendLoop * max(n.value, 1))()
        if n.value:
            self._check(self._lib.pcr_backend_loops(self._be, raw, n.value, C.byref(n)))
        return [dict(cur=int(r.cur), old=int(r.old), detector=int(r.detector), converged=int(r.converged), iterations=int(r.iterations),
                     accepted=int(r.accepted), fitness=float(r.fitness), pose=_pose_out(np.array(r.pose[:], dtype=np.float64))) for r in raw[:n.value]]

    def step(self, closest=None):
        """pcr_backend_step: addKeyFrames then closeLoops -> (info of the first, info of the second)."""
        _keep, ptr, n = self._closest(closest)
        a, b = BackendInfo(), BackendInfo()
        self._check(self._lib.pcr_backend_step(self._be, ptr, n, C.byref(a), C.byref(b)))
        return self._info(a), self._info(b)

    def reset(self):
        """pcr_backend_reset: the graph, the contexts and the counters start over; the store is left alone."""
        self._check(self._lib.pcr_backend_reset(self._be))

    LOAD_STEPS = ("read", "upload", "contexts", "downsample", "graph")      # pcr_backend_load_seconds

    def set_save_dir(self, directory):
        """pcr_backend_set_save_dir: the reference's saveMapDir.  None or "": off.  Set: addKeyFrames writes {directory}/{i}.pcd of every new
        key frame raw, before the in-place filter."""
        self._check(self._lib.pcr_backend_set_save_dir(self._be, None if directory is None else os.fsencode(directory)))

    def save(self, stamps=None, precise=False):
        """pcr_backend_save: tum.txt of all key frames and fg.g2o into the save directory (what ~Backend writes)."""
        _keep, sp = _stamps_in(stamps, self.map.keyframes())
        self._check(self._lib.pcr_backend_save(self._be, sp, int(bool(precise))))

    def load(self, directory):
        """pcr_backend_load into a fresh or reset back end over an empty store: the raw key frames, their contexts, the in-place filter, the
        graph; the next addKeyFrames / closeLoops take what comes after -> (stamps, info dict; info["load_seconds"]: host time by LOAD_STEPS)."""
        cap = _tum_lines(directory)
        stamps = np.zeros(max(cap, 1))
        i = BackendInfo()
        self._check(self._lib.pcr_backend_load(self._be, os.fsencode(directory), stamps.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(i)))
        sec = np.zeros(5)
        self._lib.pcr_backend_load_seconds(self._be, sec.ctypes.data_as(C.POINTER(C.c_double)))
        info = self._info(i)
        info["load_seconds"] = dict(zip(self.LOAD_STEPS, sec.tolist()))
        return stamps[:int(i.keyframes)].copy(), info
