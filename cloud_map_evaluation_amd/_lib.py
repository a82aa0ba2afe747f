"""ctypes binding of libmapeval_hip.so (include/mapeval_hip.h).  No fallback: a missing library is an error."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MAPEVAL_HIP_LIB: another build of the same library (e.g. the -DME_MME_STATS one, profiles/README.md); still no fallback
LIB_PATH = os.environ.get("MAPEVAL_HIP_LIB") or os.path.join(_HERE, "libmapeval_hip.so")

ME_OK = 0
ME_ERR_ARG = -1
ME_ERR_STATE = -3
ME_ERR_CAPACITY = -4
ME_SLOT_EST = 0
ME_SLOT_GT = 1
ME_GATE_LE_UNSQUARED = 0
ME_GATE_LT_SQUARED = 1
ME_FLAG_BORROW_DEVICE_INPUT = 1
ME_FLAG_MORTON_ORDER = 2
ME_SUITE_OVERLAP = 1
ME_SUITE_DEVICE_INPUT = 2
ME_SUITE_PIN_HOST_INPUT = 4
ME_LATTICE_BINS = 4096  # bins per axis of me_lattice_histograms_device

# every symbol include/mapeval_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "me_create", "me_destroy", "me_twin", "me_last_error", "me_version", "me_set_shard", "me_set_slab",
    "me_nn_unresolved", "me_nn_points", "me_nn_points_bounded", "me_nn_points_covered", "me_nn_cross_message", "me_nn_cross_answer", "me_nn_cross_patch", "me_nn_patch", "me_nn_fetch", "me_slab_points", "me_set_mme_result", "me_set_nn_result", "me_voxel_partials",
    "me_transform_points_device", "me_upload_slab_device", "me_halo_pack_device", "me_halo_pack_tagged_device", "me_lattice_histograms_device", "me_lattice_messages_device", "me_lattice_plan_device", "me_voxel_partial_rows_device", "me_voxel_merge_device",
    "me_upload_cloud", "me_upload_cloud_device", "me_cloud_size", "me_download_cloud", "me_voxel_downsample",
    "me_transform_cloud", "me_perturb_cloud", "me_voxel_downsample_into", "me_fpfh", "me_fpfh_match", "me_global_register",
    "me_statistical_outlier", "me_radius_outlier", "me_outlier_select_into",
    "me_cluster_dbscan", "me_cluster_sizes", "me_cluster_keep",
    "me_local_geometry", "me_local_geometry_fetch", "me_radius_normals", "me_nn_surface_error", "me_nn_surface_fetch",
    "me_m3c2", "me_m3c2_fetch",
    "me_mesh_upload", "me_mesh_clear", "me_mesh_info", "me_mesh_distance", "me_mesh_distance_fetch", "me_mesh_sample",
    "me_mesh_topology", "me_mesh_topology_fetch", "me_mesh_signed_distance", "me_mesh_signed_fetch",
    "me_mesh_raycast", "me_mesh_scan", "me_mesh_scan_fetch", "me_cloud_visibility", "me_cloud_visibility_fetch",
    "me_reconstruct", "me_isosurface", "me_reconstruct_fetch", "me_reconstruct_nodes_fetch", "me_reconstruct_install",
    "me_orient_normals", "me_orient_fetch",
    "me_knn_search", "me_hybrid_search", "me_radius_search", "me_search_sort_tile",
    "me_segment_planes", "me_plane_fetch", "me_plane_keep",
    "me_group_order_stats", "me_mom_select_axes", "me_mom", "me_mom_fetch",
    "me_rank_select", "me_sqrt_threshold", "me_nn_error_distribution", "me_fscore_finalize",
    "me_set_normals", "me_get_normals", "me_estimate_normals", "me_gicp_covariances", "me_get_covariances", "me_icp_lsq_sums",
    "me_icp_lsq_sums_robust", "me_icp_information",
    "me_nn1", "me_icp_p2p_sums", "me_render_distance", "me_render_entropy", "me_nn_stats", "me_nn_partial_sums", "me_nn_sigma_sums", "me_nn_finalize", "me_chamfer",
    "me_mme", "me_voxel_gaussians", "me_voxel_metrics", "me_voxel_deformation", "me_voxel_deformation_fetch", "me_voxel_distances", "me_voxel_transport", "me_awd_scs", "me_w2_batch", "me_scs_table", "me_run_suite", "me_run_suite_from", "me_mme_fetch",
    "me_set_voxel_hint", "me_cell_table_fetch", "me_timers_enable", "me_timers_reset", "me_timer_get",
]


class NNPartial(C.Structure):
    _fields_ = [
        ("n_query", C.c_int64),
        ("n_corr", C.c_int64),
        ("n_inl", C.c_int64 * 5),
        ("sum_d", C.c_double * 5),
        ("sum_d2", C.c_double * 5),
        ("sum_sqrt_all", C.c_double),
    ]


# me_nn_partial as a numpy record (the rows of me_voxel_metrics)
NN_PARTIAL_DTYPE = np.dtype([("n_query", "<i8"), ("n_corr", "<i8"), ("n_inl", "<i8", (5,)), ("sum_d", "<f8", (5,)), ("sum_d2", "<f8", (5,)),
                             ("sum_sqrt_all", "<f8")])
assert NN_PARTIAL_DTYPE.itemsize == C.sizeof(NNPartial)


# me_voxel_deformation
ME_DEFORM_FIT, ME_DEFORM_ROT_OK, ME_DEFORM_SUMS = 1, 2, 23


class DeformSummary(C.Structure):
    _fields_ = [
        ("n_voxels", C.c_int64),
        ("n_with_pairs", C.c_int64),
        ("n_fit", C.c_int64),
        ("n_rot", C.c_int64),
        ("n_pairs", C.c_int64),
        ("max_row", C.c_int64),
        ("max_key", C.c_int32 * 3),
        ("pad_", C.c_int32),
        ("sum_n_t0", C.c_double),
        ("sum_n_t0sq", C.c_double),
        ("max_t0", C.c_double),
        ("sum_e0", C.c_double),
        ("sum_e_t", C.c_double),
        ("sum_e0_fit", C.c_double),
        ("sum_e_R", C.c_double),
    ]


class VoxDistParams(C.Structure):
    _fields_ = [
        ("voxel_size", C.c_double),
        ("min_pts", C.c_int32),
        ("n_sigma", C.c_int32),
        ("sigma", C.c_double * 4),
        ("max_points", C.c_int64),
        ("eig_floor", C.c_double),
    ]


class VoxDistOut(C.Structure):
    _fields_ = [
        ("n_rows", C.c_int64),
        ("n_rows_subsampled", C.c_int64),
        ("n_pairs", C.c_int64),
        ("mean_mmd", C.c_double * 4),
        ("mean_mmd2_u", C.c_double * 4),
        ("mean_gauss", C.c_double * 4),
    ]


class VoxTransParams(C.Structure):
    _fields_ = [
        ("voxel_size", C.c_double),
        ("min_pts", C.c_int32),
        ("n_dir", C.c_int32),
        ("n_eps", C.c_int32),
        ("reserved", C.c_int32),
        ("max_points", C.c_int64),
    ]


class VoxTransOut(C.Structure):
    _fields_ = [
        ("n_rows", C.c_int64),
        ("n_rows_subsampled", C.c_int64),
        ("n_pairs", C.c_int64),
        ("n_used_est", C.c_int64),
        ("n_used_gt", C.c_int64),
        ("max_marginal_row", C.c_int64),
        ("mean_sw2", C.c_double),
        ("mean_max_sw2", C.c_double),
        ("mean_s", C.c_double),
        ("mean_sinkhorn", C.c_double),
        ("mean_marginal_err", C.c_double),
        ("max_marginal_err", C.c_double),
    ]

class IcpSums(C.Structure):
    _fields_ = [
        ("n_corr", C.c_int64),
        ("n_source", C.c_int64),
        ("origin", C.c_double * 3),
        ("sum_p", C.c_double * 3),
        ("sum_q", C.c_double * 3),
        ("sum_pq", C.c_double * 9),
        ("sum_d2", C.c_double),
    ]


class IcpLsq(C.Structure):
    _fields_ = [
        ("n_corr", C.c_int64),
        ("n_source", C.c_int64),
        ("JTJ", C.c_double * 36),
        ("JTr", C.c_double * 6),
        ("r2", C.c_double),
        ("sum_d2", C.c_double),
    ]


# me_icp_lsq_sums_robust: the loss kernels of Open3D's RobustKernel.cpp [upstream]
ME_ROBUST_L2, ME_ROBUST_L1, ME_ROBUST_HUBER, ME_ROBUST_CAUCHY, ME_ROBUST_GM, ME_ROBUST_TUKEY = range(6)
ROBUST_KERNELS = {"l2": ME_ROBUST_L2, "l1": ME_ROBUST_L1, "huber": ME_ROBUST_HUBER, "cauchy": ME_ROBUST_CAUCHY, "gm": ME_ROBUST_GM,
                  "tukey": ME_ROBUST_TUKEY}


class IcpRobust(C.Structure):
    _fields_ = [
        ("n_corr", C.c_int64),
        ("n_source", C.c_int64),
        ("n_zero_weight", C.c_int64),
        ("n_degenerate", C.c_int64),
        ("JTJ", C.c_double * 36),
        ("JTr", C.c_double * 6),
        ("r2", C.c_double),
        ("sum_d2", C.c_double),
        ("sum_w", C.c_double),
        ("sum_wr2", C.c_double),
    ]


class NNStatsOut(C.Structure):
    _fields_ = [
        ("n_src", C.c_int64),
        ("n_corr", C.c_int64),
        ("mean", C.c_double * 5),
        ("rmse", C.c_double * 5),
        ("fitness", C.c_double * 5),
        ("sigma", C.c_double * 5),
        ("number", C.c_double * 5),
        ("mean_nn_dist", C.c_double),
    ]


class SuiteParams(C.Structure):
    _fields_ = [
        ("icp_max_distance", C.c_double),
        ("gate_mode", C.c_int),
        ("trunc", C.c_double * 5),
        ("nn_radius", C.c_double),
        ("vmd_voxel_size", C.c_double),
        ("evaluate_mme", C.c_int),
        ("evaluate_gt_mme", C.c_int),
        ("min_pts", C.c_int),
        ("scs_radius", C.c_int),
    ]


class SuiteOut(C.Structure):
    _fields_ = [
        ("est_gt", NNStatsOut),
        ("gt_est", NNStatsOut),
        ("full_chamfer", C.c_double),
        ("mme_est", C.c_double),
        ("mme_gt", C.c_double),
        ("mme_est_valid", C.c_int64),
        ("mme_gt_valid", C.c_int64),
        ("awd", C.c_double),
        ("scs", C.c_double),
        ("n_w_voxels", C.c_int64),
        ("stage_ms", C.c_double * 8),
    ]


class PerturbParams(C.Structure):
    _fields_ = [
        ("noise_std", C.c_double),
        ("sparse_ratio", C.c_double),
        ("dense_ratio", C.c_double),
        ("region_size", C.c_double),
        ("outlier_ratio", C.c_double),
        ("outlier_range", C.c_double),
        ("deform_radius", C.c_double),
        ("deform_strength", C.c_double),
        ("deform_center", C.c_double * 3),
        ("seed", C.c_uint64),
    ]



class FpfhParams(C.Structure):
    _fields_ = [("radius", C.c_double), ("max_nn", C.c_int), ("normal_knn", C.c_int)]


class GlobRegParams(C.Structure):
    _fields_ = [
        ("fpfh", FpfhParams),
        ("max_corr_dist", C.c_double),
        ("edge_ratio", C.c_double),
        ("max_iterations", C.c_int64),
        ("validate_top", C.c_int),
        ("mutual", C.c_int),
        ("seed", C.c_uint64),
    ]


class GlobRegInfo(C.Structure):
    _fields_ = [
        ("n_corr", C.c_int64),
        ("n_valid_hypotheses", C.c_int64),
        ("best_hypothesis", C.c_int64),
        ("best_corr_inliers", C.c_int64),
        ("fitness", C.c_double),
        ("inlier_rmse", C.c_double),
    ]


class OutlierInfo(C.Structure):
    _fields_ = [
        ("n_in", C.c_int64),
        ("n_kept", C.c_int64),
        ("n_fallback", C.c_int64),
        ("mean", C.c_double),
        ("std_dev", C.c_double),
        ("threshold", C.c_double),
    ]


class ClusterInfo(C.Structure):
    _fields_ = [
        ("n_in", C.c_int64),
        ("n_clusters", C.c_int64),
        ("n_core", C.c_int64),
        ("n_border", C.c_int64),
        ("n_noise", C.c_int64),
        ("largest", C.c_int64),
    ]


class LocalGeomOut(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("n_valid", C.c_int64),
        ("sum_l3", C.c_double),
        ("sum_linearity", C.c_double),
        ("sum_planarity", C.c_double),
        ("sum_sphericity", C.c_double),
        ("sum_surface_variation", C.c_double),
        ("sum_k", C.c_int64),
    ]


class PlaneParams(C.Structure):
    _fields_ = [
        ("distance_threshold", C.c_double),
        ("num_iterations", C.c_int64),
        ("max_planes", C.c_int32),
        ("refit", C.c_int32),
        ("min_inliers", C.c_int64),
        ("seed", C.c_uint64),
    ]


class PlaneRecord(C.Structure):
    _fields_ = [
        ("count", C.c_int64),
        ("h", C.c_int64),
        ("score", C.c_int64),
        ("plane", C.c_double * 4),
        ("rms", C.c_double),
        ("mean_abs", C.c_double),
        ("max_abs", C.c_double),
        ("refit_degenerate", C.c_int32),
        ("reserved", C.c_int32),
    ]


class PlaneInfo(C.Structure):
    _fields_ = [
        ("n_in", C.c_int64),
        ("n_planes", C.c_int64),
        ("n_labelled", C.c_int64),
        ("n_valid_hypotheses", C.c_int64),
        ("rounds", C.c_int64),
    ]


class GroupStats(C.Structure):
    _fields_ = [
        ("count", C.c_int64),
        ("sum", C.c_double),
        ("min", C.c_double),
        ("max", C.c_double),
        ("lower", C.c_double),
        ("upper", C.c_double),
    ]


class MomParams(C.Structure):
    _fields_ = [("cos_parallel", C.c_double), ("cos_orthogonal", C.c_double), ("min_axis_points", C.c_int64)]


class MomAxisChoice(C.Structure):
    _fields_ = [("direction", C.c_int32), ("n_planes", C.c_int32), ("weight", C.c_int64), ("rep", C.c_double * 3)]


class MomAxes(C.Structure):
    _fields_ = [("n_axes", C.c_int32), ("n_directions", C.c_int32), ("axis", MomAxisChoice * 3)]


class MomAxis(C.Structure):
    _fields_ = [
        ("direction", C.c_int32),
        ("n_planes", C.c_int32),
        ("rep", C.c_double * 3),
        ("n_points", C.c_int64),
        ("n_valid", C.c_int64),
        ("sum_l3", C.c_double),
        ("min", C.c_double),
        ("max", C.c_double),
        ("lower", C.c_double),
        ("upper", C.c_double),
        ("median", C.c_double),
    ]


class MomOut(C.Structure):
    _fields_ = [("n_axes", C.c_int32), ("n_directions", C.c_int32), ("axis", MomAxis * 3), ("mom_median", C.c_double),
                ("mom_mean", C.c_double)]


ME_RANK_MAX = 16
ME_ERRDIST_MAX_THRESHOLDS = 8
ME_ERRDIST_MAX_BINS = 4096


class RankStats(C.Structure):
    _fields_ = [("count", C.c_int64), ("sum", C.c_double), ("min", C.c_double), ("max", C.c_double), ("value", C.c_double * ME_RANK_MAX)]


class ErrDistParams(C.Structure):
    _fields_ = [
        ("gate", C.c_double),
        ("gate_mode", C.c_int32),
        ("n_quantiles", C.c_int32),
        ("prob", C.c_double * ME_RANK_MAX),
        ("n_thresholds", C.c_int32),
        ("tau", C.c_double * ME_ERRDIST_MAX_THRESHOLDS),
        ("n_bins", C.c_int32),
        ("bin_width", C.c_double),
    ]


class ErrDistOut(C.Structure):
    _fields_ = [
        ("n_query", C.c_int64),
        ("n_used", C.c_int64),
        ("sum_d", C.c_double),
        ("sum_d2", C.c_double),
        ("min_d", C.c_double),
        ("max_d", C.c_double),
        ("argmax", C.c_int64),
        ("rank", C.c_int64 * ME_RANK_MAX),
        ("quantile_d", C.c_double * ME_RANK_MAX),
        ("quantile_d2", C.c_double * ME_RANK_MAX),
        ("n_within", C.c_int64 * ME_ERRDIST_MAX_THRESHOLDS),
        ("n_overflow", C.c_int64),
    ]


ME_SURFACE_MAX_ANGLES = 8


class RadiusNormalsOut(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_valid", C.c_int64), ("sum_k", C.c_int64)]


class M3c2Params(C.Structure):
    _fields_ = [
        ("projection_radius", C.c_double),
        ("max_depth", C.c_double),
        ("reg_error", C.c_double),
        ("min_points", C.c_int32),
        ("reserved", C.c_int32),
    ]


class M3c2Out(C.Structure):
    _fields_ = [
        ("n_core", C.c_int64),
        ("n_no_normal", C.c_int64),
        ("n_valid", C.c_int64),
        ("n_significant", C.c_int64),
        ("sum_dist", C.c_double),
        ("sum_abs_dist", C.c_double),
        ("sum_dist2", C.c_double),
        ("sum_lod", C.c_double),
        ("sum_n_own", C.c_int64),
        ("sum_n_other", C.c_int64),
        ("max_abs_dist", C.c_double),
        ("argmax", C.c_int64),
    ]


ME_MESH_MAX_THRESHOLDS = 8
# region codes of me_mesh_distance_fetch
MESH_FACE, MESH_EDGE_AB, MESH_EDGE_BC, MESH_EDGE_CA, MESH_VERTEX_A, MESH_VERTEX_B, MESH_VERTEX_C = range(7)


class MeshParams(C.Structure):
    _fields_ = [("max_distance", C.c_double), ("n_thresholds", C.c_int64), ("thresholds", C.c_double * ME_MESH_MAX_THRESHOLDS)]


class MeshOut(C.Structure):
    _fields_ = [
        ("n_query", C.c_int64),
        ("n_matched", C.c_int64),
        ("n_face", C.c_int64),
        ("sum_d", C.c_double),
        ("sum_d2", C.c_double),
        ("max_d", C.c_double),
        ("argmax", C.c_int64),
        ("n_within", C.c_int64 * ME_MESH_MAX_THRESHOLDS),
        ("sum_signed", C.c_double),
        ("sum_abs_signed", C.c_double),
    ]


# flags of me_mesh_topology_fetch (edges and vertices) and of me_mesh_signed_fetch (points)
MESH_TOPO_BOUNDARY, MESH_TOPO_NONMANIFOLD, MESH_TOPO_INCONSISTENT, MESH_TOPO_ZERO, MESH_TOPO_TAINTED = 1, 2, 4, 8, 16
MESH_SIGN_ON, MESH_SIGN_UNSIGNED, MESH_SIGN_UNRELIABLE = 1, 2, 4


class MeshTopoOut(C.Structure):
    _fields_ = [(k, C.c_int64) for k in (
        "n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_inconsistent_edges", "n_zero_edges", "n_zero_vertices",
        "n_tainted_vertices", "n_unreferenced_vertices", "closed", "oriented_manifold")]


class MeshSignParams(C.Structure):
    _fields_ = [("max_distance", C.c_double)]


class MeshSignOut(C.Structure):
    _fields_ = [(k, C.c_int64) for k in (
        "n_query", "n_matched", "n_signed", "n_inside", "n_outside", "n_on", "n_unsigned", "n_unreliable")] + [
        ("n_by_region", C.c_int64 * 3),
        ("sum_signed", C.c_double),
        ("sum_abs_signed", C.c_double),
        ("sum_signed2", C.c_double),
        ("min_signed", C.c_double),
        ("argmin", C.c_int64),
        ("max_signed", C.c_double),
        ("argmax", C.c_int64),
    ]


class MeshInfoOut(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_int64),
        ("n_triangles", C.c_int64),
        ("n_degenerate", C.c_int64),
        ("depth", C.c_int64),
        ("bbox_lo", C.c_double * 3),
        ("bbox_hi", C.c_double * 3),
        ("area", C.c_double),
    ]


# me_mesh_raycast: modes, per-ray flags
ME_RAY_CLOSEST, ME_RAY_ANY = 0, 1
RAY_HIT, RAY_BACKFACE, RAY_INVALID = 1, 2, 4
ME_VIS_MAX_ORIGINS = 65536


class RayOut(C.Structure):
    _fields_ = [("n_rays", C.c_int64), ("n_hit", C.c_int64), ("n_backface", C.c_int64), ("n_invalid", C.c_int64),
                ("min_t", C.c_double), ("max_t", C.c_double)]


class ScanParams(C.Structure):
    _fields_ = [("min_range", C.c_double), ("max_range", C.c_double), ("noise_std", C.c_double), ("seed", C.c_uint64)]


class ScanOut(C.Structure):
    _fields_ = [("n_rays", C.c_int64), ("n_hit", C.c_int64), ("n_backface", C.c_int64)]


class VisParams(C.Structure):
    _fields_ = [("min_range", C.c_double), ("max_range", C.c_double), ("tolerance", C.c_double), ("first_only", C.c_int64)]


class VisOut(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("n_visible", C.c_int64), ("n_in_range", C.c_int64), ("n_tests", C.c_int64)]


class ReconParams(C.Structure):
    _fields_ = [("voxel", C.c_double), ("radius", C.c_double), ("min_k", C.c_int32), ("band", C.c_int32)]


class ReconOut(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_occupied_cells", "n_active_cells", "n_nodes", "n_valid_nodes", "n_cells_extracted", "n_vertices",
                                         "n_triangles", "n_degenerate", "sum_k")]


class OrientParams(C.Structure):
    _fields_ = [("direction", C.c_double * 3), ("k", C.c_int32), ("inward", C.c_int32)]


class OrientOut(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n", "n_valid", "n_components", "largest_component", "n_tree_edges", "n_graph_edges", "n_flipped",
                                         "n_inconsistent_edges")]


class SurfaceParams(C.Structure):
    _fields_ = [
        ("gate", C.c_double),
        ("gate_mode", C.c_int32),
        ("n_thresholds", C.c_int32),
        ("tau", C.c_double * ME_ERRDIST_MAX_THRESHOLDS),
        ("n_angles", C.c_int32),
        ("reserved", C.c_int32),
        ("cos_min", C.c_double * ME_SURFACE_MAX_ANGLES),
    ]


class SurfaceOut(C.Structure):
    _fields_ = [
        ("n_query", C.c_int64),
        ("n_used", C.c_int64),
        ("n_normal_used", C.c_int64),
        ("sum_e", C.c_double),
        ("sum_e2", C.c_double),
        ("sum_t2", C.c_double),
        ("sum_c", C.c_double),
        ("max_e", C.c_double),
        ("argmax", C.c_int64),
        ("n_within", C.c_int64 * ME_ERRDIST_MAX_THRESHOLDS),
        ("sum_e2_within", C.c_double * ME_ERRDIST_MAX_THRESHOLDS),
        ("n_angle", C.c_int64 * ME_SURFACE_MAX_ANGLES),
    ]


_lib = None


def load():
    """Load libmapeval_hip.so and declare prototypes.  Raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C cloud_map_evaluation_amd/csrc).  There is no CPU fallback."
        )
    L = C.CDLL(LIB_PATH)
    vp, dp, ip = C.c_void_p, C.c_void_p, C.c_void_p  # raw addresses (host or device), passed as integers
    L.me_create.restype = C.c_void_p
    L.me_create.argtypes = [C.c_int, C.c_int]
    L.me_destroy.argtypes = [vp]
    L.me_destroy.restype = None
    L.me_twin.argtypes = [vp]
    L.me_twin.restype = C.c_void_p
    L.me_last_error.restype = C.c_char_p
    L.me_last_error.argtypes = [vp]
    L.me_version.restype = C.c_int
    L.me_set_shard.argtypes = [vp, C.c_int, C.c_int]
    L.me_set_slab.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double]
    L.me_nn_unresolved.argtypes = [vp, C.c_int, dp, dp, C.c_int64, C.POINTER(C.c_int64)]
    L.me_nn_points.argtypes = [vp, C.c_int, dp, C.c_int64, dp]
    L.me_nn_points_bounded.argtypes = [vp, C.c_int, dp, C.c_int64, dp]
    L.me_nn_points_covered.argtypes = [vp, C.c_int, dp, C.c_int64, dp, C.c_int, dp]
    L.me_nn_patch.argtypes = [vp, C.c_int, dp, C.c_int64]
    L.me_nn_cross_message.argtypes = [vp, dp, C.c_int64, C.c_int64, C.c_int64, dp]
    L.me_nn_cross_answer.argtypes = [vp, dp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, dp, C.c_double, dp]
    L.me_nn_cross_patch.argtypes = [vp, dp, C.c_int64, C.c_int]
    for f in ("me_nn_cross_message", "me_nn_cross_answer", "me_nn_cross_patch"):
        getattr(L, f).restype = C.c_int
    L.me_nn_fetch.argtypes = [vp, C.c_int, ip, dp]
    L.me_slab_points.argtypes = [vp, C.c_int, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.me_set_mme_result.argtypes = [vp, C.c_int, dp, vp]
    L.me_set_nn_result.argtypes = [vp, C.c_int, C.c_int, dp]
    L.me_voxel_partials.argtypes = [vp, C.c_int, C.c_double, ip, ip, dp, dp, C.POINTER(C.c_int64)]
    L.me_transform_points_device.argtypes = [vp, dp, C.c_int64, dp]
    L.me_upload_slab_device.argtypes = [vp, C.c_int, dp, C.c_int64, C.c_double]
    L.me_upload_slab_device.restype = C.c_int
    L.me_halo_pack_device.argtypes = [vp, dp, C.c_int64, C.c_int, dp, C.c_int, C.c_double, dp, C.c_int64, dp]
    L.me_halo_pack_tagged_device.argtypes = [vp, dp, C.c_int64, C.c_int, dp, C.c_int, C.c_double, dp, dp, C.c_int64, C.c_int64, dp]
    L.me_halo_pack_tagged_device.restype = C.c_int
    L.me_lattice_histograms_device.argtypes = [vp, dp, C.c_int64, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp]
    L.me_lattice_histograms_device.restype = C.c_int
    L.me_lattice_messages_device.argtypes = [vp, dp, C.c_int64, dp, C.c_int64, C.c_int, C.c_int, vp]
    L.me_lattice_messages_device.restype = C.c_int
    L.me_lattice_plan_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int64)]
    L.me_lattice_plan_device.restype = C.c_int
    L.me_voxel_partial_rows_device.argtypes = [vp, C.c_int, C.c_double, dp, C.c_int64, C.POINTER(C.c_int64)]
    L.me_voxel_merge_device.argtypes = [vp, C.c_int, C.c_double, dp, C.c_int64]
    for f in ("me_transform_points_device", "me_upload_slab_device", "me_halo_pack_device", "me_voxel_partial_rows_device", "me_voxel_merge_device"):
        getattr(L, f).restype = C.c_int
    L.me_set_voxel_hint.argtypes = [vp, C.c_double]
    L.me_set_voxel_hint.restype = C.c_int
    L.me_voxel_downsample.argtypes = [vp, C.c_int, C.c_double, C.POINTER(C.c_int64)]
    L.me_transform_cloud.argtypes = [vp, C.c_int, dp]
    L.me_perturb_cloud.argtypes = [vp, C.c_int, C.c_int, C.POINTER(PerturbParams), C.POINTER(C.c_int64)]
    L.me_perturb_cloud.restype = C.c_int
    L.me_voxel_downsample_into.argtypes = [vp, C.c_int, vp, C.c_int, C.c_double, C.POINTER(C.c_int64)]
    L.me_fpfh.argtypes = [vp, C.c_int, C.POINTER(FpfhParams), dp]
    L.me_fpfh_match.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, C.POINTER(C.c_int64)]
    L.me_global_register.argtypes = [vp, C.c_int, C.c_int, C.POINTER(GlobRegParams), dp, C.POINTER(GlobRegInfo), vp]
    for f in ("me_voxel_downsample_into", "me_fpfh", "me_fpfh_match", "me_global_register"):
        getattr(L, f).restype = C.c_int
    L.me_statistical_outlier.argtypes = [vp, C.c_int, C.c_int, C.c_double, dp, vp, C.POINTER(OutlierInfo)]
    L.me_radius_outlier.argtypes = [vp, C.c_int, C.c_int, C.c_double, ip, vp, C.POINTER(OutlierInfo)]
    L.me_outlier_select_into.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(C.c_int64)]
    for f in ("me_statistical_outlier", "me_radius_outlier", "me_outlier_select_into"):
        getattr(L, f).restype = C.c_int
    L.me_cluster_dbscan.argtypes = [vp, C.c_int, C.c_double, C.c_int, ip, ip, C.POINTER(ClusterInfo)]
    L.me_cluster_sizes.argtypes = [vp, C.c_int, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.me_cluster_keep.argtypes = [vp, C.c_int, C.c_int64, C.c_int64, vp, C.POINTER(OutlierInfo)]
    for f in ("me_cluster_dbscan", "me_cluster_sizes", "me_cluster_keep"):
        getattr(L, f).restype = C.c_int
    L.me_local_geometry.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.POINTER(LocalGeomOut)]
    L.me_local_geometry_fetch.argtypes = [vp, C.c_int, dp, ip, vp]
    for f in ("me_local_geometry", "me_local_geometry_fetch"):
        getattr(L, f).restype = C.c_int
    L.me_radius_normals.argtypes = [vp, C.c_int, C.c_double, C.c_int, dp, C.c_int, C.POINTER(RadiusNormalsOut)]
    L.me_nn_surface_error.argtypes = [vp, C.c_int, C.POINTER(SurfaceParams), C.POINTER(SurfaceOut)]
    L.me_nn_surface_fetch.argtypes = [vp, C.c_int, dp, dp]
    for f in ("me_radius_normals", "me_nn_surface_error", "me_nn_surface_fetch"):
        getattr(L, f).restype = C.c_int
    L.me_m3c2.argtypes = [vp, C.c_int, C.POINTER(M3c2Params), vp, C.POINTER(M3c2Out)]
    L.me_m3c2_fetch.argtypes = [vp, C.c_int, dp, dp, dp, dp, ip, ip, vp]
    for f in ("me_m3c2", "me_m3c2_fetch"):
        getattr(L, f).restype = C.c_int
    L.me_mesh_upload.argtypes = [vp, dp, C.c_int64, ip, C.c_int64, dp]
    L.me_mesh_clear.argtypes = [vp]
    L.me_mesh_info.argtypes = [vp, C.POINTER(MeshInfoOut)]
    L.me_mesh_distance.argtypes = [vp, C.c_int, C.POINTER(MeshParams), C.POINTER(MeshOut)]
    L.me_mesh_distance_fetch.argtypes = [vp, C.c_int, dp, ip, vp, dp, dp]
    L.me_mesh_sample.argtypes = [vp, C.c_int, C.c_int64, C.c_uint64]
    L.me_mesh_topology.argtypes = [vp, C.POINTER(MeshTopoOut)]
    L.me_mesh_topology_fetch.argtypes = [vp, dp, vp, dp, vp]
    L.me_mesh_signed_distance.argtypes = [vp, C.c_int, C.POINTER(MeshSignParams), C.POINTER(MeshSignOut)]
    L.me_mesh_signed_fetch.argtypes = [vp, C.c_int, dp, vp]
    for f in ("me_mesh_upload", "me_mesh_clear", "me_mesh_info", "me_mesh_distance", "me_mesh_distance_fetch", "me_mesh_sample",
              "me_mesh_topology", "me_mesh_topology_fetch", "me_mesh_signed_distance", "me_mesh_signed_fetch"):
        getattr(L, f).restype = C.c_int
    L.me_mesh_raycast.argtypes = [vp, dp, dp, C.c_int64, C.c_double, C.c_double, C.c_int, dp, ip, dp, dp, vp, C.POINTER(RayOut)]
    L.me_mesh_scan.argtypes = [vp, C.c_int, dp, C.c_int64, dp, C.c_int64, C.POINTER(ScanParams), vp, C.POINTER(ScanOut)]
    L.me_mesh_scan_fetch.argtypes = [vp, C.c_int, vp]
    L.me_cloud_visibility.argtypes = [vp, C.c_int, dp, C.c_int64, C.POINTER(VisParams), C.POINTER(VisOut)]
    L.me_cloud_visibility_fetch.argtypes = [vp, C.c_int, ip, ip]
    for f in ("me_mesh_raycast", "me_mesh_scan", "me_mesh_scan_fetch", "me_cloud_visibility", "me_cloud_visibility_fetch"):
        getattr(L, f).restype = C.c_int
    L.me_reconstruct.argtypes = [vp, C.c_int, C.POINTER(ReconParams), C.POINTER(ReconOut)]
    L.me_isosurface.argtypes = [vp, ip, dp, vp, C.c_int64, C.c_double, C.POINTER(ReconOut)]
    L.me_reconstruct_fetch.argtypes = [vp, dp, ip, ip]
    L.me_reconstruct_nodes_fetch.argtypes = [vp, ip, dp, ip, vp]
    L.me_reconstruct_install.argtypes = [vp]
    for f in ("me_reconstruct", "me_isosurface", "me_reconstruct_fetch", "me_reconstruct_nodes_fetch", "me_reconstruct_install"):
        getattr(L, f).restype = C.c_int
    L.me_orient_normals.argtypes = [vp, C.c_int, C.POINTER(OrientParams), C.POINTER(OrientOut)]
    L.me_orient_fetch.argtypes = [vp, C.c_int, ip, vp]
    for f in ("me_orient_normals", "me_orient_fetch"):
        getattr(L, f).restype = C.c_int
    L.me_knn_search.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, ip, dp]
    L.me_hybrid_search.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, vp, ip, ip, dp]
    L.me_radius_search.argtypes = [vp, C.c_int, C.c_int, C.c_double, vp, vp, ip, dp, C.c_int64, C.POINTER(C.c_int64)]
    L.me_search_sort_tile.argtypes = []
    for f in ("me_knn_search", "me_hybrid_search", "me_radius_search", "me_search_sort_tile"):
        getattr(L, f).restype = C.c_int
    L.me_segment_planes.argtypes = [vp, C.c_int, C.POINTER(PlaneParams), vp, ip, vp, C.POINTER(PlaneInfo)]
    L.me_plane_fetch.argtypes = [vp, C.c_int, vp, C.c_int64, C.POINTER(C.c_int64), ip]
    L.me_plane_keep.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(OutlierInfo)]
    for f in ("me_segment_planes", "me_plane_fetch", "me_plane_keep"):
        getattr(L, f).restype = C.c_int
    L.me_group_order_stats.argtypes = [vp, dp, ip, C.c_int64, C.c_int32, vp]
    L.me_mom_select_axes.argtypes = [vp, C.c_int32, C.POINTER(MomParams), ip, C.POINTER(MomAxes)]
    L.me_mom.argtypes = [vp, C.c_int, C.POINTER(MomParams), C.POINTER(MomOut)]
    L.me_mom_fetch.argtypes = [vp, C.c_int, vp]
    for f in ("me_group_order_stats", "me_mom_select_axes", "me_mom", "me_mom_fetch"):
        getattr(L, f).restype = C.c_int
    L.me_rank_select.argtypes = [vp, dp, vp, C.c_int64, vp, C.c_int32, C.POINTER(RankStats)]
    L.me_rank_select.restype = C.c_int
    L.me_sqrt_threshold.argtypes = [C.c_double]
    L.me_sqrt_threshold.restype = C.c_double
    L.me_nn_error_distribution.argtypes = [vp, C.c_int, C.POINTER(ErrDistParams), C.POINTER(ErrDistOut), vp]
    L.me_nn_error_distribution.restype = C.c_int
    L.me_fscore_finalize.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_double * 3)]
    L.me_fscore_finalize.restype = None
    L.me_upload_cloud.argtypes = [vp, C.c_int, dp, C.c_int64, dp, C.c_double]
    L.me_upload_cloud_device.argtypes = [vp, C.c_int, dp, C.c_int64, dp, C.c_double]
    L.me_cloud_size.restype = C.c_int64
    L.me_cloud_size.argtypes = [vp, C.c_int]
    L.me_download_cloud.argtypes = [vp, C.c_int, dp]
    L.me_nn1.argtypes = [vp, C.c_int, C.c_int, ip, dp]
    L.me_icp_p2p_sums.argtypes = [vp, C.c_int, C.c_double, C.POINTER(IcpSums)]
    L.me_icp_p2p_sums.restype = C.c_int
    L.me_set_normals.argtypes = [vp, C.c_int, dp]
    L.me_get_normals.argtypes = [vp, C.c_int, dp]
    L.me_estimate_normals.argtypes = [vp, C.c_int, C.c_int, dp, ip, dp]
    L.me_gicp_covariances.argtypes = [vp, C.c_int, C.c_double, dp]
    L.me_get_covariances.argtypes = [vp, C.c_int, dp]
    L.me_get_covariances.restype = C.c_int
    L.me_icp_lsq_sums.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.POINTER(IcpLsq)]
    L.me_icp_lsq_sums_robust.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.POINTER(IcpRobust)]
    L.me_icp_information.argtypes = [vp, C.c_int, C.c_double, dp, C.POINTER(C.c_int64)]
    for f in ("me_set_normals", "me_get_normals", "me_estimate_normals", "me_gicp_covariances", "me_icp_lsq_sums", "me_icp_lsq_sums_robust",
              "me_icp_information"):
        getattr(L, f).restype = C.c_int
    L.me_render_distance.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int, vp, vp]
    L.me_render_distance.restype = C.c_int
    L.me_render_entropy.argtypes = [vp, C.c_int, vp, vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double)]
    L.me_render_entropy.restype = C.c_int
    L.me_nn_stats.argtypes = [vp, C.c_int, C.c_double, C.c_int, dp, C.POINTER(NNStatsOut)]
    L.me_nn_partial_sums.argtypes = [vp, C.c_int, C.c_double, C.c_int, dp, C.POINTER(NNPartial)]
    L.me_nn_sigma_sums.argtypes = [vp, C.c_int, C.c_double, C.c_int, dp, dp]
    L.me_nn_finalize.restype = None
    L.me_nn_finalize.argtypes = [C.POINTER(NNPartial), dp, C.c_int64, C.POINTER(NNStatsOut)]
    L.me_chamfer.argtypes = [vp, C.POINTER(C.c_double)]
    L.me_mme.argtypes = [vp, C.c_int, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.me_voxel_gaussians.argtypes = [vp, C.c_int, C.c_double, ip, ip, dp, dp, dp, C.POINTER(C.c_int64)]
    L.me_voxel_metrics.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int, dp, ip, vp, dp, vp, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int64)]
    L.me_voxel_metrics.restype = C.c_int
    L.me_voxel_deformation.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.POINTER(DeformSummary)]
    L.me_voxel_deformation_fetch.argtypes = [vp, C.c_int, ip, vp, vp, dp, dp, dp, dp, dp, C.POINTER(C.c_int64)]
    for f in ("me_voxel_deformation", "me_voxel_deformation_fetch"):
        getattr(L, f).restype = C.c_int
    L.me_voxel_distances.argtypes = [vp, C.POINTER(VoxDistParams), ip, ip, ip, dp, dp, dp, C.POINTER(C.c_int64), C.POINTER(VoxDistOut)]
    L.me_voxel_distances.restype = C.c_int
    L.me_voxel_transport.argtypes = [vp, C.POINTER(VoxTransParams), dp, dp, ip, ip, ip, dp, dp, dp, dp, C.POINTER(C.c_int64), C.POINTER(VoxTransOut)]
    L.me_voxel_transport.restype = C.c_int
    L.me_awd_scs.argtypes = [vp, C.c_double, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                             C.POINTER(C.c_double), dp]
    L.me_run_suite.argtypes = [vp, C.POINTER(SuiteParams), C.POINTER(SuiteOut)]
    L.me_run_suite_from.argtypes = [vp, dp, C.c_int64, dp, C.c_int64, dp, C.POINTER(SuiteParams), C.c_int, C.POINTER(SuiteOut)]
    L.me_mme_fetch.argtypes = [vp, C.c_int, dp, dp]
    L.me_w2_batch.argtypes = [vp, dp, dp, ip, dp, dp, ip, C.c_int64, dp]
    L.me_scs_table.argtypes = [vp, ip, dp, C.c_int64, C.c_int, C.POINTER(C.c_double)]
    L.me_cell_table_fetch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp, vp, vp, vp]
    L.me_cell_table_fetch.restype = C.c_int
    L.me_timers_enable.argtypes = [vp, C.c_int]
    L.me_timers_reset.argtypes = [vp]
    L.me_timer_get.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    for f in ("me_voxel_downsample", "me_transform_cloud", "me_set_slab", "me_nn_unresolved", "me_nn_points", "me_nn_points_bounded", "me_nn_points_covered", "me_nn_patch", "me_nn_fetch", "me_slab_points", "me_set_mme_result", "me_set_nn_result", "me_voxel_partials", "me_set_shard", "me_upload_cloud", "me_upload_cloud_device", "me_download_cloud", "me_nn1", "me_icp_p2p_sums", "me_render_distance", "me_render_entropy", "me_nn_stats",
              "me_nn_partial_sums", "me_nn_sigma_sums", "me_chamfer", "me_mme", "me_voxel_gaussians", "me_awd_scs",
              "me_run_suite", "me_run_suite_from", "me_mme_fetch", "me_w2_batch", "me_scs_table", "me_timers_enable", "me_timers_reset", "me_timer_get"):
        getattr(L, f).restype = C.c_int
    _lib = L
    return L
