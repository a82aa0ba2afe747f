// map_eval.h — host side of the drop-in: the reference's Param / MapEval surface (map_eval/src/map_eval.h:60-362) with the
// metric hot path delegated to libmapeval_hip.so through the C ABI (include/mapeval_hip.h).  No Open3D / Eigen / PCL /
// TBB / yaml-cpp: clouds are std::vector<double> (AoS xyz, the same memory layout as open3d PointCloud::points_).
#pragma once

#include <cmath>
#include <array>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mapeval_hip.h"
#include "dist_comm.hpp"  // medist::Comm, medist::DevMem (multi-GPU: num_gpus > 1)

using Vector5d = std::array<double, 5>;

struct PointCloud {  // stands in for open3d::geometry::PointCloud on the hot path (points_ only)
    std::vector<double> points_;  // xyz xyz ...
    size_t size() const { return points_.size() / 3; }
    bool IsEmpty() const { return points_.empty(); }
};

// Same members and defaults as the reference's Param (map_eval.h:60-116); YAML keys in map_eval_main.cpp:120-208.
struct Param {
    std::string evaluation_map_pcd_path_ = "/data/map_evaluation/canteen/";
    std::string map_gt_path_ = "/data/map_evaluation/canteen/merged_scan.pcd";
    std::string result_path_ = "/home/hts/workspace/dataset/eva_results/";
    std::string pcd_file_name_ = "map.pcd";
    std::string name_;
    int evaluation_method_ = 2;
    double voxel_size_ = 1.0;
    double icp_max_distance_ = 2.5;
    double nn_radius_ = 0.2;
    bool save_immediate_result_ = false;
    bool evaluate_mme_ = true;
    bool evaluate_gt_mme_ = true;
    bool evaluate_using_initial_ = true;
    bool evaluate_noised_gt_ = false;
    bool use_visualization = false;
    bool enable_debug = false;
    bool use_tbb_mme = true;  // accepted; the GPU path has a single implementation
    Vector5d trunc_dist_{{0.2, 0.1, 0.08, 0.05, 0.01}};  // the reference leaves this uninitialised (map_eval.h:85)
    std::array<double, 16> initial_matrix_{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};  // row-major 4x4
    double noise_std_dev_ = 0.1;
    double vmd_voxel_size_ = 3.0;
    double downsample_size = 0.01;
    // ---- new, optional keys (absent in the reference's configs) ----
    int gpu_device = 0;             // `gpu_device:` HIP device ordinal
    bool strict_reference = false;  // `strict_reference:` true = reproduce FULL CD = 0 on the initial-matrix path
                                    // (the reference never calls computeChamferDistance there, map_eval.cpp:1204-1260)
    int num_gpus = 1;               // `num_gpus:` N > 1 = one process per GPU (devices gpu_device .. gpu_device + N - 1), the
                                    // clouds cut into N slabs, collectives over RCCL (map_eval_dist.cpp)
    bool save_voxel_metrics = false;  // `save_voxel_metrics:` true = also write map_results/voxel_metrics.txt, the per-voxel AC / COM / CD /
                                      // MME sums on the AWD lattice (single GPU only; saveVoxelMetrics)
    // simulation mode (evaluate_noised_gt: true): the map evaluated is a perturbed copy of the ground truth, made on the device
    // (me_perturb_cloud).  noise_std_dev_ above is the noise; these keys switch the reference's other three generators on
    // (map_eval.cpp:1757-1829; the defaults leave them off) and fix the Philox seed
    uint64_t noise_seed = 0;                                      // `noise_seed:`
    double noise_sparse_ratio = 1.0, noise_dense_ratio = 1.0;     // `noise_sparse_ratio:`, `noise_dense_ratio:` keep probabilities
    double noise_region_size = 0.0;                               // `noise_region_size:` (<= 0: no density stage)
    double noise_outlier_ratio = 0.0, noise_outlier_range = 0.0;  // `noise_outlier_ratio:`, `noise_outlier_range:`
    double noise_deform_radius = 0.0, noise_deform_strength = 0.0;  // `noise_deform_radius:`, `noise_deform_strength:`
    std::array<double, 3> noise_deform_center{{0, 0, 0}};         // `noise_deform_center: [x, y, z]`
    std::vector<double> noise_sweep;  // `noise_sweep: [s0, s1, ..]` after the run, one suite per noise level on the resident ground
                                      // truth -> map_results/noise_sweep.txt (single GPU, initial-matrix path; runNoiseSweep)
    // coarse global registration (global_registration: true; no reference counterpart): on the registration path, FPFH + RANSAC on
    // down-sampled copies finds T_c, and ICP starts from T_c * initial_matrix (me_global_register)
    bool global_registration = false;      // `global_registration:`
    double global_voxel_size = 1.0;        // `global_voxel_size:` coarse voxel
    double global_feature_radius = 0.0;    // `global_feature_radius:` FPFH radius (<= 0 in the struct: 5 x voxel)
    int global_max_nn = 40;                // `global_max_nn:` FPFH neighbour cap, 1..40
    int global_normal_knn = 30;            // `global_normal_knn:` k of the normal estimation
    double global_max_corr_dist = 0.0;     // `global_max_corr_dist:` inlier distance (<= 0 in the struct: 1.5 x voxel)
    int64_t global_max_iterations = 1000000;  // `global_max_iterations:` hypotheses drawn
    double global_edge_ratio = 0.9;        // `global_edge_ratio:`
    bool global_mutual_filter = true;      // `global_mutual_filter:`
    uint64_t global_seed = 0;              // `global_seed:` Philox seed
    double global_min_fitness = 0.0;       // `global_min_fitness:` below this fitness of T_c the run fails
    int global_outlier_nb_neighbors = 0;   // `global_outlier_nb_neighbors:` > 0: statistical outlier removal (this k) on full-resolution
                                           // copies of both clouds before global_voxel_size (me_statistical_outlier)
    double global_outlier_std_ratio = 2.0; // `global_outlier_std_ratio:`
    // robust / multi-scale ICP and the information matrix (no reference counterpart; registration path, single GPU; DESIGN.md section
    // 4.17): Open3D's robust loss on the point-to-plane / generalized step, a coarse-to-fine schedule, GetInformationMatrixFromPointClouds
    int icp_robust_kernel = 0;             // `icp_robust_kernel:` none | l1 | huber | cauchy | gm | tukey (an ME_ROBUST_* id; 0 = none)
    double icp_robust_scale = 0.0;         // `icp_robust_scale:` k of huber / cauchy / gm / tukey (required for them: no default)
    std::vector<double> icp_multi_scale_voxels;     // `icp_multi_scale_voxels: [v0, v1, ..]` (<= 0: the resident clouds themselves)
    std::vector<double> icp_multi_scale_distances;  // `icp_multi_scale_distances: [..]` the level's correspondence distance
    std::vector<int> icp_multi_scale_iterations;    // `icp_multi_scale_iterations: [..]` the level's iteration cap
    bool icp_information_matrix = false;   // `icp_information_matrix:` -> map_results/registration_information.txt
    // outlier removal in front of the evaluation (remove_outliers: statistical | radius; no reference counterpart): the map, and with
    // outlier_filter_gt the ground truth, filtered in place on the device after downsample_size -> map_results/outlier_removal.txt
    std::string remove_outliers = "none";  // `remove_outliers:` none | statistical | radius | cluster | plane (the largest plane: plane_* keys)
    int outlier_nb_neighbors = 20;         // `outlier_nb_neighbors:` statistical: k, 1..40
    double outlier_std_ratio = 2.0;        // `outlier_std_ratio:`
    int outlier_nb_points = -1;            // `outlier_nb_points:` radius: keep points with more than this many within the radius (required)
    double outlier_radius = 0.0;           // `outlier_radius:` radius (required)
    bool outlier_filter_gt = false;        // `outlier_filter_gt:` filter the ground truth as well
    double outlier_eps = 0.0;              // `outlier_eps:` cluster: DBSCAN eps (required, > 0)
    int outlier_min_points = 10;           // `outlier_min_points:` cluster: DBSCAN min_points, >= 1
    int outlier_min_cluster_size = 1;      // `outlier_min_cluster_size:` cluster: clusters below this size are dropped (noise always is)
    int outlier_keep_largest = 0;          // `outlier_keep_largest:` cluster: > 0 keeps only that many of the largest clusters
    // mean plane variance and the eigenvalue shape features (optional keys; no reference counterpart): me_local_geometry on the clouds
    // as loaded, where computeMME runs; an `MPV:` and a `LocalGeometry` line after `MME:`, and local_geometry.txt
    bool evaluate_mpv = false;             // `evaluate_mpv:`
    double mpv_radius = 0.0;               // `mpv_radius:` neighbourhood radius, > 0 (default: nn_radius)
    int mpv_min_points = 5;                // `mpv_min_points:` neighbours a point needs to count, >= 2
    bool evaluate_gt_mpv = false;          // `evaluate_gt_mpv:` also on the ground truth (default: evaluate_gt_mme)
    // RANSAC plane segmentation (optional keys; no reference counterpart): me_segment_planes on the clouds as loaded, where
    // computeMME runs; a `Planes est-gt:` line after the MPV lines, and plane_segmentation.txt
    bool segment_planes = false;             // `segment_planes:`
    double plane_distance_threshold = 0.05;  // `plane_distance_threshold:` > 0
    int64_t plane_num_iterations = 1000;     // `plane_num_iterations:` hypotheses per round, >= 1
    int plane_max_planes = 8;                // `plane_max_planes:` 1..64
    int64_t plane_min_inliers = 1000;        // `plane_min_inliers:` >= 3
    uint64_t plane_seed = 0;                 // `plane_seed:` Philox seed
    bool plane_refit = true;                 // `plane_refit:` least-squares plane of the inliers
    bool segment_gt_planes = false;          // `segment_gt_planes:` also on the ground truth (default: evaluate_gt_mme)
    // MOM, the plane variance on mutually orthogonal planes (optional keys; no reference counterpart): me_mom on the clouds as loaded,
    // from me_local_geometry (the mpv_* keys) and me_segment_planes (the plane_* keys), which it runs itself when their own keys are
    // off; a `MOM est-gt:` line after the `Planes` line, and mom.txt
    bool evaluate_mom = false;               // `evaluate_mom:`
    double mom_parallel_deg = 10.0;          // `mom_parallel_deg:` planes within this angle share a direction
    double mom_orthogonal_deg = 10.0;        // `mom_orthogonal_deg:` directions within this angle of a right angle are orthogonal
    int64_t mom_min_axis_points = 1000;      // `mom_min_axis_points:` labelled points a direction needs, >= 1
    bool evaluate_gt_mom = false;            // `evaluate_gt_mom:` also on the ground truth (default: evaluate_gt_mme)
    // the error distribution of both directions (optional keys; no reference counterpart): me_nn_error_distribution on the 1-NN results
    // the metric path leaves resident, after its two me_nn_stats calls (single GPU); three lines after `FULL CD`, and
    // error_distribution.txt
    bool evaluate_error_distribution = false;  // `evaluate_error_distribution:`
    std::vector<double> error_quantiles{0.5, 0.9, 0.95, 0.99};  // `error_quantiles: [..]` at most 16, each in [0, 1]
    std::vector<double> error_thresholds;      // `error_thresholds: [..]` at most 8, each >= 0 (default: accuracy_level)
    // the normal-aware map error (optional keys; no reference counterpart): me_radius_normals on both clouds as loaded, where the MPV
    // stage runs, then me_nn_surface_error on the 1-NN results the initial-matrix metric path leaves resident (single GPU, with
    // evaluate_using_initial); three lines after the error-distribution lines, and surface_error.txt
    bool evaluate_surface_error = false;       // `evaluate_surface_error:`
    double normal_radius = 0.0;                // `normal_radius:` > 0 (default: nn_radius)
    int normal_min_points = 5;                 // `normal_min_points:` neighbours a point needs for a normal, >= 2
    std::vector<double> surface_thresholds;    // `surface_thresholds: [..]` at most 8, each >= 0 (default: accuracy_level)
    std::vector<double> surface_angles_deg{5.0, 10.0, 20.0};  // `surface_angles_deg: [..]` at most 8, each in [0, 90]
    bool surface_gated = false;                // `surface_gated:` the metric path's correspondence gate (default: every pair)
    int error_cdf_bins = 1000;                 // `error_cdf_bins:` 0 .. 4096 (0: no CDF)
    double error_cdf_max = 0;                  // `error_cdf_max:` the last bin edge (default: icp_max_distance); bin width = max / bins
    bool error_gated = false;                  // `error_gated:` true = the metric path's own gate and gate mode apply
    // M3C2, the signed cloud-to-cloud distance (optional keys; no reference counterpart): on the resident clouds with the map moved by
    // initial_matrix, before every other stage — me_radius_normals on both clouds, me_m3c2 in both directions — after which both clouds
    // are uploaded again as loaded (single GPU, with evaluate_using_initial); one line before `VMD`, and m3c2.txt
    bool evaluate_m3c2 = false;                // `evaluate_m3c2:`
    bool evaluate_deformation = false;         // `evaluate_deformation:` true = the per-voxel rigid deformation field of the map against the
                                               // ground truth (me_voxel_deformation; single GPU only): a result line and deformation_field.txt
    double deformation_voxel_size = 0;         // `deformation_voxel_size:` (default vmd_voxel_size)
    double deformation_max_distance = 0;       // `deformation_max_distance:` a DISTANCE (d2 < max^2); default sqrt(icp_max_distance) when that is > 0, else inf
    int deformation_min_pairs = 30;            // `deformation_min_pairs:` (>= 3)
    double deformation_min_spread = 0;         // `deformation_min_spread:` (default deformation_voxel_size / 20)
    bool evaluate_voxel_distances = false;     // `evaluate_voxel_distances:` true = per AWD voxel the point-set MMD and the Gaussian KL / Bhattacharyya /
                                               // textbook W2 of the two clouds (me_voxel_distances; single GPU only): two result lines and voxel_distances.txt
    std::vector<double> mmd_sigmas;            // `mmd_sigmas:` 1 - 4 kernel bandwidths (default [nn_radius])
    long long mmd_max_points = 2048;           // `mmd_max_points:` a fuller voxel is sub-sampled by a stride (0: never; else >= 11)
    double voxel_distance_eig_floor = 1e-6;    // `voxel_distance_eig_floor:` the eigenvalue floor of the closed forms (> 0)
    bool evaluate_voxel_transport = false;     // `evaluate_voxel_transport:` true = per AWD voxel the sliced 2-Wasserstein distance and the debiased Sinkhorn
                                               // divergence of the two clouds' points (me_voxel_transport; single GPU only): two result lines and voxel_transport.txt
    double transport_blur = 0;                 // `transport_blur:` metres, > 0 (default nn_radius): the schedule ends at blur^2
    int transport_directions = 32;             // `transport_directions:` 0 .. 64 directions of a Fibonacci half sphere (0: no sliced part)
    long long transport_max_points = 512;      // `transport_max_points:` 11 .. 1024: a fuller voxel is sub-sampled by a stride
    double transport_scaling = 0.5;            // `transport_scaling:` in (0, 1): eps shrinks by its square per iteration down to blur^2
    double m3c2_normal_radius = 0.0;           // `m3c2_normal_radius:` > 0 (default: nn_radius)
    double m3c2_projection_radius = 0.0;       // `m3c2_projection_radius:` the cylinder's radius, > 0 (default: nn_radius)
    double m3c2_max_depth = 0.0;               // `m3c2_max_depth:` the cylinder's half-length, > 0 (default: 4 nn_radius)
    int m3c2_min_points = 5;                   // `m3c2_min_points:` points either cloud needs inside the cylinder, >= 2
    double m3c2_reg_error = 0.0;               // `m3c2_reg_error:` the registration error added to the level of detection, >= 0
    int m3c2_core_every = 1;                   // `m3c2_core_every:` every k-th point of a cloud, in file order, is a core point, >= 1
    // cloud-to-mesh distance against a ground-truth triangle mesh (optional keys; the role of the reference's mesh branch with a mesh
    // the user supplies): the map moved by initial_matrix against the mesh of `gt_mesh_path` as it is in the file (like the ground-truth
    // cloud, the mesh is not moved), on the resident clouds before every other stage, after which both clouds are uploaded again as
    // loaded (single GPU); two lines before `VMD`, and mesh_distance.txt
    bool evaluate_mesh_distance = false;       // `evaluate_mesh_distance:`
    std::string gt_mesh_path;                  // `gt_mesh_path:` a PLY with a face element (required with evaluate_mesh_distance)
    std::vector<double> mesh_thresholds;       // `mesh_thresholds: [..]` at most 8, each >= 0 (default: accuracy_level)
    double mesh_max_distance = INFINITY;       // `mesh_max_distance:` matched iff d <= this; <= 0 or absent: every point
    int64_t mesh_sample_points = 0;            // `mesh_sample_points:` > 0: also the mesh sampled into the ground-truth slot, 1-NN both ways
    uint64_t mesh_seed = 0;                    // `mesh_seed:` the sampler's seed
    bool mesh_signed = false;                  // `mesh_signed:` also the sign at edges and vertices (me_mesh_signed_distance; needs evaluate_mesh_distance)
    // surface reconstruction of both clouds (optional keys; the reference's createMeshFromPCD, map_eval.cpp:777-826, with the library's
    // IMLS field + marching tetrahedra instead of Poisson): radius normals turned towards a viewpoint on each cloud as loaded,
    // me_reconstruct, gt_mesh.ply / est_mesh.ply (the reference's names) and reconstruction.txt in the results folder (single GPU).
    // With evaluate_mesh_distance and no gt_mesh_path the map is measured against the reconstructed ground-truth mesh.
    bool evaluate_mesh = false;                // `evaluate_mesh:` the reference's hard-coded eva_mesh
    double mesh_voxel_size = 0.0;              // `mesh_voxel_size:` the lattice's voxel (required with evaluate_mesh)
    double mesh_radius = 0.0;                  // `mesh_radius:` the field's support (default 3 mesh_voxel_size), >= mesh_voxel_size
    int mesh_min_points = 8;                   // `mesh_min_points:` points a node needs, >= 1
    int mesh_band = 1;                         // `mesh_band:` cells around the occupied ones, 0 .. 2
    double mesh_normal_radius = 0.0;           // `mesh_normal_radius:` radius of the normals (default nn_radius)
    std::vector<double> mesh_viewpoint;        // `mesh_viewpoint: [x, y, z]` the normals point towards it (default: each cloud's bbox centre)
    std::string mesh_orient = "viewpoint";     // `mesh_orient: viewpoint | propagate`: propagate = me_orient_normals after unoriented radius normals
    int mesh_orient_k = 12;                    // `mesh_orient_k`: neighbours of the orientation graph, 1 .. 39
    bool mesh_orient_inward = false;           // `mesh_orient_inward`: the roots are turned against +z instead of towards it
    // completeness against the OBSERVABLE ground truth (optional keys; no reference counterpart): the ground-truth points that some pose
    // of `trajectory_path` sees past the ground-truth mesh (gt_mesh_path, or the reconstruction of evaluate_mesh) by me_cloud_visibility,
    // and the recall of the map (moved by initial_matrix) over all and over the observable ground-truth points; afterwards both clouds are
    // uploaded again as loaded (single GPU); one line before `VMD`, and observable.txt
    bool evaluate_observable = false;          // `evaluate_observable:`
    std::string trajectory_path;               // `trajectory_path:` TUM text `t x y z qx qy qz qw` (required with evaluate_observable; positions only)
    int observable_pose_stride = 1;            // `observable_pose_stride:` every k-th pose, >= 1
    double observable_max_range = INFINITY;    // `observable_max_range:` metres (absent or <= 0: inf)
    double observable_tolerance = 0.05;        // `observable_tolerance:` metres short of the point at which the segment ends, >= 0
    std::vector<double> observable_thresholds; // `observable_thresholds: [..]` recall thresholds, at most 8 (default: accuracy_level)
    int dist_rank = 0;              // (set by the launcher, not a YAML key)
    void printParam() const;
};

Param loadParametersFromYAML(const std::string &yaml_file_path);  // map_eval_main.cpp:120-208
std::string paramToJson(const Param &p);                          // for tests (--parse-config); an infinite value prints as Infinity

class MapEval {
public:
    explicit MapEval(Param &param);  // map_eval.h:123-189: results folder + map_results.txt header (append mode)
    ~MapEval();

    int process();                                         // map_eval.cpp:4-102
    int processOneCall(bool from_host, double t_loaded);   // its metric phase (:52-85) as one me_run_suite_from call
    void computeMME(PointCloud &cloud, PointCloud &gt);    // map_eval.cpp:149-189
    void calculateMetricsWithInitialMatrix();              // map_eval.cpp:1204-1260
    void finishInitialMatrixMetrics(const me_nn_stats_out &eg, const me_nn_stats_out &ge, double t_acc_s);  // its tail (:1238-1259)
    // map_eval.cpp:191-237, registration_methods 0 / 1 / 2; with a communicator: queries sharded, sums all-reduced (map_eval_dist.cpp);
    // metrics = false: stop after the loop (the distributed host computes the ICP-path statistics on its slabs)
    int performRegistration(bool metrics = true);
    void finishRegistrationMetrics(const me_nn_stats_out &eg, const me_nn_stats_out &ge, double t_acc_s);  // calculateMetrics' tail
    void calculateMetrics();                               // map_eval.cpp:1147-1202
    double computeChamferDistance();                       // map_eval.cpp:1398-1431
    void calculateVMD(bool tables_ready = false, bool write_files = true);  // map_eval.cpp:240-390
    bool renderEntropy(int slot, std::vector<double> &xyz, std::vector<double> &rgb, bool want_points);  // :686-735
    void saveMmeResults();                                 // map_eval.cpp:392-421
    void saveRegistrationResults();                        // map_eval.cpp:424-482 (text lines; renderers out of scope)
    void saveVoxelMetrics(int gate_mode);                  // voxel_metrics.txt (save_voxel_metrics; no reference counterpart)
    me_perturb_params perturbParams(double noise_std) const;  // the noise_* keys as me_perturb_cloud's parameters
    int runNoiseSweep();
    int computeMPV();                                       // evaluate_mpv: me_local_geometry on both clouds (no reference counterpart)
    void saveMpvResults();                                  // its result lines and local_geometry.txt
    int removeOutliers();                                   // outlier_removal.txt (remove_outliers; no reference counterpart)
    int removeSmallClusters();                              // ... remove_outliers: cluster
    int removeLargestPlane();                               // ... remove_outliers: plane
    me_plane_params planeParams(int max_planes) const;      // the plane_* keys as me_segment_planes' parameters
    int segmentPlanes();                                    // segment_planes: me_segment_planes on both clouds (no reference counterpart)
    void savePlaneResults();                                // its result line and plane_segmentation.txt
    me_mom_params momParams() const;                        // the mom_* keys (degrees) as me_mom's cosines
    int computeMOM();                                       // evaluate_mom: me_mom on both clouds (no reference counterpart)
    void saveMomResults();                                  // its result line and mom.txt
    int computeErrorDistribution(int gate_mode);            // evaluate_error_distribution: both directions (no reference counterpart)
    int computeSurfaceNormals();                            // evaluate_surface_error: me_radius_normals on both clouds as loaded
    int computeSurfaceError(int gate_mode);                 // ... me_nn_surface_error on both directions (no reference counterpart)
    void saveSurfaceError();                                // its three result lines and surface_error.txt
    int computeM3C2();                                      // evaluate_m3c2: normals and me_m3c2 on both clouds, the map moved (no reference counterpart)
    void saveM3C2();                                        // its result line and m3c2.txt
    int computeDeformation();                               // evaluate_deformation: me_voxel_deformation with the map as the query (no reference counterpart)
    int computeVoxelDistances();                            // evaluate_voxel_distances: me_voxel_distances on the AWD lattice (no reference counterpart)
    void saveDeformation();                                 // its result line and deformation_field.txt
    void saveVoxelDistances();                              // its two result lines and voxel_distances.txt
    int computeVoxelTransport();                            // evaluate_voxel_transport: me_voxel_transport on the AWD lattice (no reference counterpart)
    void saveVoxelTransport();                              // its two result lines and voxel_transport.txt
    int computeMeshDistance();                              // evaluate_mesh_distance: me_mesh_distance of the moved map (no reference counterpart)
    void saveMeshDistance();                                // its two result lines and mesh_distance.txt
    int computeObservable();                                // evaluate_observable: me_cloud_visibility of the ground truth, recall for all / observable points
    void saveObservable();                                  // its result line and observable.txt
    int computeReconstruction();                            // evaluate_mesh: radius normals + me_reconstruct on both clouds as loaded
    void saveReconstruction();                              // gt_mesh.ply, est_mesh.ply, reconstruction.txt
    void saveErrorDistribution();                           // its three result lines and error_distribution.txt
    int writeRegistrationInformation();                     // registration_information.txt (icp_information_matrix; no reference counterpart)
    int globalRegistration(double T_c[16]);                 // global_registration.txt (global_registration; no reference counterpart)                                   // noise_sweep.txt (noise_sweep; no reference counterpart)

    // multi-GPU (map_eval_dist.cpp): the communicator of this rank; forced = take the distributed path with one rank too
    void setComm(medist::Comm *comm, bool forced) {
        comm_ = comm;
        dist_forced_ = forced;
    }
    int processDist(double t_loaded);

    Param param_;
    // results, same names as the reference (map_eval.h:328-353)
    std::vector<Vector5d> est_gt_results, gt_est_results;
    Vector5d f1_vec{{0, 0, 0, 0, 0}}, cd_vec{{0, 0, 0, 0, 0}}, iou_vec{{0, 0, 0, 0, 0}};
    std::array<double, 16> trans{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};  // ICP result (row-major), map_eval.h:332
    double vmd = 0.0, full_chamfer_dist = 0.0, scs_overall = 0.0;
    double mme_est = 0.0, mme_gt = 0.0, max_abs_entropy = 0.0, min_abs_entropy = 0.0;
    std::vector<me_plane_record> plane_rec[2];  // segment_planes: [ME_SLOT_EST], [ME_SLOT_GT] (the latter with segment_gt_planes)
    me_errdist_params errdist_params = {};  // evaluate_error_distribution: what both directions were asked for
    me_errdist_out errdist_out[2] = {};     // ... [ME_SLOT_EST], [ME_SLOT_GT]
    std::vector<int64_t> errdist_hist[2];
    me_surface_params surface_params = {};      // evaluate_surface_error: what both directions were asked for
    me_surface_out surface_out[2] = {};         // ... [ME_SLOT_EST], [ME_SLOT_GT]
    me_radius_normals_out surface_normals[2] = {};
    me_m3c2_out m3c2_out[2] = {};               // evaluate_m3c2: [ME_SLOT_EST], [ME_SLOT_GT] as the query
    me_deform_summary deform_out = {};          // evaluate_deformation
    me_voxdist_out voxdist_out = {};            // evaluate_voxel_distances: the summary and the rows (keys | n_pop | n_used | ksum | mmd2 | gauss)
    std::vector<int32_t> voxdist_keys, voxdist_pop, voxdist_used;
    std::vector<double> voxdist_ksum, voxdist_mmd2, voxdist_gauss;
    me_voxtrans_out voxtrans_out = {};          // evaluate_voxel_transport: the summary, the directions and the schedule as used, and the rows
    std::vector<int32_t> voxtrans_keys, voxtrans_pop, voxtrans_used;
    std::vector<double> voxtrans_dirs, voxtrans_eps, voxtrans_sliced, voxtrans_sinkhorn;
    me_radius_normals_out m3c2_normals[2] = {};
    me_mesh_info_out mesh_info = {};            // evaluate_mesh_distance: the mesh, the totals, the quantiles of d, the sampled block
    me_mesh_out mesh_out = {};
    me_mesh_topo_out mesh_topo = {};            // ... with mesh_signed: the mesh's connectivity and the signed totals
    me_mesh_sign_out mesh_sign = {};
    std::vector<int64_t> mesh_rank;
    std::vector<double> mesh_quantile;
    me_errdist_out mesh_sampled[2] = {};        // ... with mesh_sample_points: 1-NN error of the map in the sample and the reverse
    double mesh_prf[ME_MESH_MAX_THRESHOLDS][3] = {};
    me_vis_out obs_vis = {};                    // evaluate_observable: the visibility totals, the poses used, the ground truth's error
    int64_t obs_poses = 0, obs_poses_file = 0;  // distribution at the thresholds over all points [0] and over the observable ones [1]
    me_errdist_out obs_gt[2] = {};
    me_recon_out recon_out[2] = {};             // evaluate_mesh: per slot the counts, the normals' info, the viewpoint used and the mesh
    me_radius_normals_out recon_normals[2] = {};
    double recon_viewpoint[2][3] = {};
    me_orient_out recon_orient[2] = {};
    std::vector<double> recon_vertices[2];
    std::vector<int32_t> recon_triangles[2];
    me_mom_out mom_out[2] = {};  // evaluate_mom: [ME_SLOT_EST], [ME_SLOT_GT] (the latter with evaluate_gt_mom)
    me_local_geom_out mpv_out[2] = {};  // evaluate_mpv: [ME_SLOT_EST], [ME_SLOT_GT] (the latter with evaluate_gt_mpv)
    std::vector<double> est_entropies, gt_entropies;
    std::vector<uint8_t> valid_entropy_points, gt_valid_entropy_points;
    std::vector<double> map_entropy_xyz, map_entropy_rgb, gt_entropy_xyz, gt_entropy_rgb;  // map_3d_entropy / gt_3d_entropy (:330)
    std::string last_error;

private:
    int fail(const std::string &msg);
    int allReduceHost(std::vector<double> &v, bool min_op);
    int gatherPerPoint(int slot, size_t n_global, const std::vector<int64_t> &tags, const std::vector<double> *vals,
                       const std::vector<uint8_t> *flags, std::vector<double> *vals_out, std::vector<uint8_t> *flags_out);
    int exchangeCloud(const std::vector<double> &pts, size_t i0, size_t i1, const double *T, int axis, const std::vector<double> &cuts,
                      double halo, medist::DevMem &recv, std::vector<int64_t> &tags_out, int64_t *n_recv);
    int reduceIcp(me_icp_sums &s, me_icp_lsq &q, int method);  // all-reduce of the registration step's additive sums
    medist::DevMem pool_[7];  // device buffers of the collectives, kept for the run
    medist::Comm *comm_ = nullptr;
    bool dist_forced_ = false;
    me_ctx *render_ctx_ = nullptr;  // rank 0 of a multi-GPU run: the whole clouds, for the colour renderers
    std::shared_ptr<PointCloud> map_3d_, gt_3d_;
    me_ctx *ctx_ = nullptr;
    double t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0, t_fcd = 0, t_acc = 0;
    double t_vmd = 0, t_v = 0, t_cdf = 0, t_scs = 0;
    std::string subfolder, results_subfolder, results_file_path;
    std::ofstream file_result;
};
