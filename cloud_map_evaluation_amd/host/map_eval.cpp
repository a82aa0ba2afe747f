// map_eval.cpp — host orchestration mirroring MapEval::process (map_eval/src/map_eval.cpp:4-102): same config keys,
// same result-file lines, same output file names; every metric comes from libmapeval_hip.so (no CPU metric path).
#include "map_eval.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <ctime>
#include <filesystem>
#include <iomanip>
#include <iostream>
#include <numeric>
#include <sstream>

#include "../csrc/me_horn.hpp"
#include <cerrno>

#include "pcd_io.hpp"
#include "tum_io.hpp"
#include "yaml_lite.hpp"

namespace fs = std::filesystem;

namespace {

struct TicToc {  // include/tic_toc.h:10-24 — milliseconds since construction
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double toc() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Eigen's default IOFormat for `os << v.transpose()`: entries right-aligned to the widest one, separated by one space.
std::string eigen_row(const Vector5d &v, int precision) {
    std::vector<std::string> s;
    size_t w = 0;
    for (double x : v) {
        std::ostringstream o;
        o << std::fixed << std::setprecision(precision) << x;
        s.push_back(o.str());
        w = std::max(w, s.back().size());
    }
    std::string out;
    for (size_t i = 0; i < s.size(); ++i) {
        if (i) out += " ";
        out += std::string(w - s[i].size(), ' ') + s[i];
    }
    return out;
}

// Eigen's default IOFormat for `os << Matrix4d` (row-major input): common width over all 16 coefficients
std::string eigen_matrix4(const double *m, int precision) {
    std::string s[16];
    size_t w = 0;
    for (int i = 0; i < 16; ++i) {
        std::ostringstream o;
        o << std::fixed << std::setprecision(precision) << m[i];
        s[i] = o.str();
        w = std::max(w, s[i].size());
    }
    std::string out;
    for (int r = 0; r < 4; ++r) {
        for (int c = 0; c < 4; ++c) out += (c ? " " : "") + std::string(w - s[4 * r + c].size(), ' ') + s[4 * r + c];
        if (r < 3) out += "\n";
    }
    return out;
}

Vector5d to5(const double *p) { return Vector5d{{p[0], p[1], p[2], p[3], p[4]}}; }

void push_results(std::vector<Vector5d> &dst, const me_nn_stats_out &o) {
    // result.push_back(mean, rmse, fitness, sigma, number) (map_eval.cpp:1140-1144)
    dst.clear();
    dst.push_back(to5(o.mean));
    dst.push_back(to5(o.rmse));
    dst.push_back(to5(o.fitness));
    dst.push_back(to5(o.sigma));
    dst.push_back(to5(o.number));
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
void Param::printParam() const {
    std::cout << "\n[==================== Experiment Configuration ====================]\n"
              << "Experiment Name: " << name_ << "\n"
              << "Evaluation Map Path: " << evaluation_map_pcd_path_ << "\n"
              << "Ground Truth Map Path: " << map_gt_path_ << "\n"
              << "Result Save Path: " << result_path_ << "\n"
              << "ICP Maximum Distance: " << icp_max_distance_ << "\n"
              << "Evaluation Method: " << evaluation_method_ << "\n"
              << "Truncation Distance: " << eigen_row(trunc_dist_, 6) << "\n"
              << "Save Immediate Result: " << save_immediate_result_ << "\n"
              << "Evaluate MME: " << evaluate_mme_ << "\n"
              << "Evaluate Ground Truth MME: " << evaluate_gt_mme_ << "\n"
              << "Nearest Neighbor Radius: " << nn_radius_ << "\n"
              << "Use Initial Matrix for Evaluation: " << evaluate_using_initial_ << "\n"
              << "Voxel Size for VMD: " << vmd_voxel_size_ << "\n"
              << "GPU device: " << gpu_device << "\n"
              << "[====================================================================]\n";
}

Param loadParametersFromYAML(const std::string &yaml_file_path) {
    // Same required / optional key split as map_eval_main.cpp:120-208 (a missing required key throws).
    const yaml_lite::Document config = yaml_lite::Document::load_file(yaml_file_path);
    Param param;
    param.evaluation_method_ = config.as_int("registration_methods");
    param.icp_max_distance_ = config.as_double("icp_max_distance");
    if (config.has("accuracy_level") && config.at("accuracy_level").seq.size() >= 5)
        for (int i = 0; i < 5; ++i) param.trunc_dist_[i] = yaml_lite::Document::to_double(config.at("accuracy_level").seq[i], "accuracy_level");
    if (config.has("initial_matrix") && config.at("initial_matrix").rows.size() >= 4)
        for (int i = 0; i < 4; ++i) {
            const auto &row = config.at("initial_matrix").rows[i];
            if (row.size() < 4) throw std::runtime_error("initial_matrix: each row needs 4 numbers");
            for (int j = 0; j < 4; ++j) param.initial_matrix_[4 * i + j] = yaml_lite::Document::to_double(row[j], "initial_matrix");
        }
    param.save_immediate_result_ = config.as_bool("save_immediate_result");
    param.evaluate_mme_ = config.as_bool("evaluate_mme");
    param.evaluate_gt_mme_ = config.as_bool("evaluate_gt_mme");
    param.evaluate_using_initial_ = config.as_bool("evaluate_using_initial");
    param.nn_radius_ = config.as_double("nn_radius");
    param.vmd_voxel_size_ = config.as_double("vmd_voxel_size");
    param.downsample_size = config.as_double("downsample_size");
    param.evaluation_map_pcd_path_ = config.as_string("estimate_map_path");
    param.map_gt_path_ = config.as_string("gt_map_path");
    param.name_ = config.as_string("scene_name");
    if (!param.evaluation_map_pcd_path_.empty() && param.evaluation_map_pcd_path_.back() != '/') param.evaluation_map_pcd_path_ += '/';
    param.result_path_ = param.evaluation_map_pcd_path_ + "map_results/";
    if (config.has("pcd_file_name")) param.pcd_file_name_ = config.as_string("pcd_file_name");
    if (config.has("evaluate_noised_gt")) param.evaluate_noised_gt_ = config.as_bool("evaluate_noised_gt");
    if (config.has("noise_std_dev")) param.noise_std_dev_ = config.as_double("noise_std_dev");
    if (config.has("voxel_size")) param.voxel_size_ = config.as_double("voxel_size");
    if (config.has("use_visualization")) param.use_visualization = config.as_bool("use_visualization");
    param.enable_debug = config.as_bool("enable_debug");
    if (config.has("use_tbb_mme")) param.use_tbb_mme = config.as_bool("use_tbb_mme");
    if (config.has("gpu_device")) param.gpu_device = config.as_int("gpu_device");
    if (config.has("strict_reference")) param.strict_reference = config.as_bool("strict_reference");
    if (config.has("num_gpus")) param.num_gpus = config.as_int("num_gpus");
    if (param.num_gpus < 1 || param.num_gpus > 64) throw std::runtime_error("num_gpus must be in 1..64");
    if (config.has("save_voxel_metrics")) param.save_voxel_metrics = config.as_bool("save_voxel_metrics");
    if (param.save_voxel_metrics && param.num_gpus > 1)
        throw std::runtime_error("save_voxel_metrics: single GPU only (num_gpus must be 1)");
    // simulation mode (the reference reads evaluate_noised_gt and noise_std_dev only; the misspelt evaluate_noise_gt of its shipped
    // configs is not read there either)
    auto as_seed = [&config](const char *key) -> uint64_t {
        const std::string &v = config.at(key).scalar;
        size_t used = 0;
        unsigned long long seed = 0;
        try {
            seed = std::stoull(v, &used, 0);
        } catch (const std::exception &) {
            used = 0;
        }
        if (v.empty() || v[0] == '-' || used != v.size())
            throw std::runtime_error(std::string(key) + ": expected an unsigned integer, got '" + v + "'");
        return seed;
    };
    if (config.has("noise_seed")) param.noise_seed = as_seed("noise_seed");
    if (config.has("noise_sparse_ratio")) param.noise_sparse_ratio = config.as_double("noise_sparse_ratio");
    if (config.has("noise_dense_ratio")) param.noise_dense_ratio = config.as_double("noise_dense_ratio");
    if (config.has("noise_region_size")) param.noise_region_size = config.as_double("noise_region_size");
    if (config.has("noise_outlier_ratio")) param.noise_outlier_ratio = config.as_double("noise_outlier_ratio");
    if (config.has("noise_outlier_range")) param.noise_outlier_range = config.as_double("noise_outlier_range");
    if (config.has("noise_deform_radius")) param.noise_deform_radius = config.as_double("noise_deform_radius");
    if (config.has("noise_deform_strength")) param.noise_deform_strength = config.as_double("noise_deform_strength");
    if (config.has("noise_deform_center")) {
        const auto &c = config.at("noise_deform_center").seq;
        if (c.size() != 3) throw std::runtime_error("noise_deform_center: expected a flow list of three numbers");
        for (int a = 0; a < 3; ++a) param.noise_deform_center[a] = yaml_lite::Document::to_double(c[a], "noise_deform_center");
    }
    if (config.has("noise_sweep")) {
        const auto &c = config.at("noise_sweep").seq;
        if (c.empty()) throw std::runtime_error("noise_sweep: expected a flow list of noise levels");
        for (const auto &v : c) param.noise_sweep.push_back(yaml_lite::Document::to_double(v, "noise_sweep"));
    }
    if (param.evaluate_noised_gt_ && param.num_gpus > 1)
        throw std::runtime_error("evaluate_noised_gt: single GPU only (num_gpus must be 1)");
    if (!param.noise_sweep.empty() && !(param.evaluate_noised_gt_ && param.evaluate_using_initial_ && param.num_gpus == 1))
        throw std::runtime_error("noise_sweep: needs evaluate_noised_gt: true, evaluate_using_initial: true and num_gpus: 1");
    // coarse global registration (no reference counterpart)
    if (config.has("global_registration")) param.global_registration = config.as_bool("global_registration");
    if (config.has("global_voxel_size")) param.global_voxel_size = config.as_double("global_voxel_size");
    if (config.has("global_feature_radius")) param.global_feature_radius = config.as_double("global_feature_radius");
    else param.global_feature_radius = 5.0 * param.global_voxel_size;
    if (config.has("global_max_nn")) param.global_max_nn = config.as_int("global_max_nn");
    if (config.has("global_normal_knn")) param.global_normal_knn = config.as_int("global_normal_knn");
    if (config.has("global_max_corr_dist")) param.global_max_corr_dist = config.as_double("global_max_corr_dist");
    else param.global_max_corr_dist = 1.5 * param.global_voxel_size;
    if (config.has("global_max_iterations")) param.global_max_iterations = (int64_t) config.as_double("global_max_iterations");
    if (config.has("global_edge_ratio")) param.global_edge_ratio = config.as_double("global_edge_ratio");
    if (config.has("global_mutual_filter")) param.global_mutual_filter = config.as_bool("global_mutual_filter");
    if (config.has("global_seed")) param.global_seed = as_seed("global_seed");
    if (config.has("global_min_fitness")) param.global_min_fitness = config.as_double("global_min_fitness");
    if (param.global_registration) {
        if (param.evaluate_using_initial_)
            throw std::runtime_error("global_registration: needs the registration path (evaluate_using_initial: false): there is no ICP to start");
        if (param.num_gpus > 1) throw std::runtime_error("global_registration: single GPU only (num_gpus must be 1)");
    }
    if (!(param.global_voxel_size > 0)) throw std::runtime_error("global_voxel_size: must be > 0");
    if (!(param.global_feature_radius > 0)) throw std::runtime_error("global_feature_radius: must be > 0");
    if (!(param.global_max_corr_dist > 0)) throw std::runtime_error("global_max_corr_dist: must be > 0");
    if (param.global_max_iterations < 1) throw std::runtime_error("global_max_iterations: must be >= 1");
    if (!(param.global_edge_ratio > 0 && param.global_edge_ratio <= 1)) throw std::runtime_error("global_edge_ratio: must lie in (0, 1]");
    if (param.global_max_nn < 1 || param.global_max_nn > 40) throw std::runtime_error("global_max_nn: must lie in 1..40");
    if (param.global_normal_knn < 1 || param.global_normal_knn > 40) throw std::runtime_error("global_normal_knn: must lie in 1..40");
    if (config.has("icp_robust_kernel")) {
        const std::string k = config.as_string("icp_robust_kernel");
        const char *names[6] = {"none", "l1", "huber", "cauchy", "gm", "tukey"};  // (ME_ROBUST_L2 .. ME_ROBUST_TUKEY)
        int id = -1;
        for (int i = 0; i < 6; ++i)
            if (k == names[i]) id = i;
        if (id < 0) throw std::runtime_error("icp_robust_kernel: expected none, l1, huber, cauchy, gm or tukey, got '" + k + "'");
        param.icp_robust_kernel = id;
    }
    if (config.has("icp_robust_scale")) {
        param.icp_robust_scale = config.as_double("icp_robust_scale");
        if (!(param.icp_robust_scale > 0) || !std::isfinite(param.icp_robust_scale))
            throw std::runtime_error("icp_robust_scale: must be finite and > 0");
    } else if (param.icp_robust_kernel >= ME_ROBUST_HUBER) {
        throw std::runtime_error("icp_robust_kernel: " + config.as_string("icp_robust_kernel") + " needs icp_robust_scale (no default is invented)");
    }
    {
        const char *keys[3] = {"icp_multi_scale_voxels", "icp_multi_scale_distances", "icp_multi_scale_iterations"};
        const int given = (int) config.has(keys[0]) + (int) config.has(keys[1]) + (int) config.has(keys[2]);
        if (given != 0 && given != 3)
            throw std::runtime_error("icp_multi_scale_voxels, icp_multi_scale_distances and icp_multi_scale_iterations: give all three or none");
        if (given == 3) {
            for (const auto &v : config.at(keys[0]).seq) param.icp_multi_scale_voxels.push_back(yaml_lite::Document::to_double(v, keys[0]));
            for (const auto &v : config.at(keys[1]).seq) param.icp_multi_scale_distances.push_back(yaml_lite::Document::to_double(v, keys[1]));
            for (const auto &v : config.at(keys[2]).seq) param.icp_multi_scale_iterations.push_back((int) yaml_lite::Document::to_double(v, keys[2]));
            const size_t n = param.icp_multi_scale_voxels.size();
            if (n == 0 || param.icp_multi_scale_distances.size() != n || param.icp_multi_scale_iterations.size() != n)
                throw std::runtime_error("icp_multi_scale_*: three flow lists of the same, non-zero length are expected");
            for (size_t l = 0; l < n; ++l)
                if (!(param.icp_multi_scale_distances[l] > 0) || param.icp_multi_scale_iterations[l] < 0)
                    throw std::runtime_error("icp_multi_scale_*: distances must be > 0 and iterations >= 0");
        }
    }
    if (config.has("icp_information_matrix")) param.icp_information_matrix = config.as_bool("icp_information_matrix");
    if (param.icp_robust_kernel != 0 || !param.icp_multi_scale_voxels.empty() || param.icp_information_matrix) {
        const char *who = param.icp_robust_kernel != 0 ? "icp_robust_kernel" : !param.icp_multi_scale_voxels.empty() ? "icp_multi_scale_voxels"
                                                                                                                      : "icp_information_matrix";
        if (param.evaluate_using_initial_)
            throw std::runtime_error(std::string(who) + ": needs the registration path (evaluate_using_initial: false): there is no ICP to run");
        if (param.num_gpus > 1) throw std::runtime_error(std::string(who) + ": single GPU only (num_gpus must be 1)");
    }
    if (config.has("global_outlier_nb_neighbors")) param.global_outlier_nb_neighbors = config.as_int("global_outlier_nb_neighbors");
    if (config.has("global_outlier_std_ratio")) param.global_outlier_std_ratio = config.as_double("global_outlier_std_ratio");
    if (param.global_outlier_nb_neighbors < 0 || param.global_outlier_nb_neighbors > 40)
        throw std::runtime_error("global_outlier_nb_neighbors: must lie in 0..40 (0 = off)");
    if (!(param.global_outlier_std_ratio > 0)) throw std::runtime_error("global_outlier_std_ratio: must be > 0");
    // outlier removal in front of the evaluation (no reference counterpart)
    if (config.has("remove_outliers")) param.remove_outliers = config.as_string("remove_outliers");
    if (param.remove_outliers != "none" && param.remove_outliers != "statistical" && param.remove_outliers != "radius" &&
        param.remove_outliers != "cluster" && param.remove_outliers != "plane")
        throw std::runtime_error("remove_outliers: expected none, statistical, radius, cluster or plane, got '" + param.remove_outliers + "'");
    if (config.has("outlier_nb_neighbors")) param.outlier_nb_neighbors = config.as_int("outlier_nb_neighbors");
    if (config.has("outlier_std_ratio")) param.outlier_std_ratio = config.as_double("outlier_std_ratio");
    if (config.has("outlier_nb_points")) param.outlier_nb_points = config.as_int("outlier_nb_points");
    if (config.has("outlier_radius")) param.outlier_radius = config.as_double("outlier_radius");
    if (config.has("outlier_filter_gt")) param.outlier_filter_gt = config.as_bool("outlier_filter_gt");
    if (param.outlier_nb_neighbors < 1 || param.outlier_nb_neighbors > 40) throw std::runtime_error("outlier_nb_neighbors: must lie in 1..40");
    if (!(param.outlier_std_ratio > 0)) throw std::runtime_error("outlier_std_ratio: must be > 0");
    if (param.remove_outliers == "radius") {
        if (!config.has("outlier_nb_points") || param.outlier_nb_points < 0)
            throw std::runtime_error("outlier_nb_points: remove_outliers: radius needs it, >= 0");
        if (!config.has("outlier_radius") || !(param.outlier_radius > 0))
            throw std::runtime_error("outlier_radius: remove_outliers: radius needs it, > 0");
    }
    if (config.has("outlier_eps")) param.outlier_eps = config.as_double("outlier_eps");
    if (config.has("outlier_min_points")) param.outlier_min_points = config.as_int("outlier_min_points");
    if (config.has("outlier_min_cluster_size")) param.outlier_min_cluster_size = config.as_int("outlier_min_cluster_size");
    if (config.has("outlier_keep_largest")) param.outlier_keep_largest = config.as_int("outlier_keep_largest");
    if (param.outlier_min_points < 1) throw std::runtime_error("outlier_min_points: must be >= 1");
    if (param.outlier_min_cluster_size < 1) throw std::runtime_error("outlier_min_cluster_size: must be >= 1");
    if (param.outlier_keep_largest < 0) throw std::runtime_error("outlier_keep_largest: must be >= 0 (0 = no limit)");
    if (param.remove_outliers == "cluster") {
        if (!config.has("outlier_eps") || !(param.outlier_eps > 0) || !std::isfinite(param.outlier_eps))
            throw std::runtime_error("outlier_eps: remove_outliers: cluster needs it, > 0");
    }
    if (param.remove_outliers != "none") {
        if (param.num_gpus > 1)
            throw std::runtime_error("remove_outliers: single GPU only for now (num_gpus must be 1; the multi-GPU path is out of scope)");
        if (param.evaluate_noised_gt_)
            throw std::runtime_error("remove_outliers: not with evaluate_noised_gt for now (the simulated map is out of scope)");
    }
    // mean plane variance and the eigenvalue shape features (no reference counterpart)
    if (config.has("evaluate_mpv")) param.evaluate_mpv = config.as_bool("evaluate_mpv");
    param.mpv_radius = config.has("mpv_radius") ? config.as_double("mpv_radius") : param.nn_radius_;
    if (config.has("mpv_min_points")) param.mpv_min_points = config.as_int("mpv_min_points");
    param.evaluate_gt_mpv = config.has("evaluate_gt_mpv") ? config.as_bool("evaluate_gt_mpv") : param.evaluate_gt_mme_;
    if (param.evaluate_mpv) {
        if (!(param.mpv_radius > 0) || !std::isfinite(param.mpv_radius)) throw std::runtime_error("mpv_radius: must be > 0");
        if (param.mpv_min_points < 2) throw std::runtime_error("mpv_min_points: must be >= 2 (the covariance divides by k - 1)");
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_mpv: single GPU only (num_gpus must be 1)");
    }
    // RANSAC plane segmentation (no reference counterpart); remove_outliers: plane takes the same plane_* keys
    if (config.has("segment_planes")) param.segment_planes = config.as_bool("segment_planes");
    if (config.has("plane_distance_threshold")) param.plane_distance_threshold = config.as_double("plane_distance_threshold");
    if (config.has("plane_num_iterations")) param.plane_num_iterations = (int64_t) config.as_double("plane_num_iterations");
    if (config.has("plane_max_planes")) param.plane_max_planes = config.as_int("plane_max_planes");
    if (config.has("plane_min_inliers")) param.plane_min_inliers = (int64_t) config.as_double("plane_min_inliers");
    if (config.has("plane_seed")) param.plane_seed = as_seed("plane_seed");
    if (config.has("plane_refit")) param.plane_refit = config.as_bool("plane_refit");
    param.segment_gt_planes = config.has("segment_gt_planes") ? config.as_bool("segment_gt_planes") : param.evaluate_gt_mme_;
    if (param.segment_planes || param.remove_outliers == "plane") {
        if (!(param.plane_distance_threshold > 0) || !std::isfinite(param.plane_distance_threshold))
            throw std::runtime_error("plane_distance_threshold: must be > 0");
        if (param.plane_num_iterations < 1 || param.plane_num_iterations > (1 << 24))
            throw std::runtime_error("plane_num_iterations: must lie in 1..2^24");
        if (param.plane_max_planes < 1 || param.plane_max_planes > 64) throw std::runtime_error("plane_max_planes: must lie in 1..64");
        if (param.plane_min_inliers < 3) throw std::runtime_error("plane_min_inliers: must be >= 3");
        if (param.segment_planes && param.num_gpus > 1) throw std::runtime_error("segment_planes: single GPU only (num_gpus must be 1)");
    }
    // MOM (no reference counterpart): its two inputs take the mpv_* and plane_* keys, checked here when their own stages are off
    if (config.has("evaluate_mom")) param.evaluate_mom = config.as_bool("evaluate_mom");
    if (config.has("mom_parallel_deg")) param.mom_parallel_deg = config.as_double("mom_parallel_deg");
    if (config.has("mom_orthogonal_deg")) param.mom_orthogonal_deg = config.as_double("mom_orthogonal_deg");
    if (config.has("mom_min_axis_points")) param.mom_min_axis_points = (int64_t) config.as_double("mom_min_axis_points");
    param.evaluate_gt_mom = config.has("evaluate_gt_mom") ? config.as_bool("evaluate_gt_mom") : param.evaluate_gt_mme_;
    if (param.evaluate_mom) {
        if (!(param.mom_parallel_deg >= 0) || !(param.mom_parallel_deg < 90)) throw std::runtime_error("mom_parallel_deg: must lie in [0, 90)");
        if (!(param.mom_orthogonal_deg >= 0) || !(param.mom_orthogonal_deg < 90))
            throw std::runtime_error("mom_orthogonal_deg: must lie in [0, 90)");
        if (!(param.mom_parallel_deg + param.mom_orthogonal_deg < 90))
            throw std::runtime_error("mom_parallel_deg + mom_orthogonal_deg: must be < 90 (a direction cannot be parallel and orthogonal to another)");
        if (param.mom_min_axis_points < 1) throw std::runtime_error("mom_min_axis_points: must be >= 1");
        if (!(param.mpv_radius > 0) || !std::isfinite(param.mpv_radius)) throw std::runtime_error("mpv_radius: must be > 0");
        if (param.mpv_min_points < 2) throw std::runtime_error("mpv_min_points: must be >= 2 (the covariance divides by k - 1)");
        if (!(param.plane_distance_threshold > 0) || !std::isfinite(param.plane_distance_threshold))
            throw std::runtime_error("plane_distance_threshold: must be > 0");
        if (param.plane_num_iterations < 1 || param.plane_num_iterations > (1 << 24))
            throw std::runtime_error("plane_num_iterations: must lie in 1..2^24");
        if (param.plane_max_planes < 1 || param.plane_max_planes > 64) throw std::runtime_error("plane_max_planes: must lie in 1..64");
        if (param.plane_min_inliers < 3) throw std::runtime_error("plane_min_inliers: must be >= 3");
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_mom: single GPU only (num_gpus must be 1)");
    }
    // the error distribution of both directions (no reference counterpart)
    if (config.has("evaluate_error_distribution")) param.evaluate_error_distribution = config.as_bool("evaluate_error_distribution");
    std::string error_not_a_list;  // a list key that holds a scalar or a block sequence: refused below, when the stage is on
    for (const char *key : {"error_quantiles", "error_thresholds"})
        if (config.has(key) && (!config.at(key).scalar.empty() || !config.at(key).rows.empty()) && error_not_a_list.empty()) error_not_a_list = key;
    if (config.has("error_quantiles")) {
        param.error_quantiles.clear();
        for (const auto &v : config.at("error_quantiles").seq) param.error_quantiles.push_back(yaml_lite::Document::to_double(v, "error_quantiles"));
    }
    if (config.has("error_thresholds")) {
        for (const auto &v : config.at("error_thresholds").seq) param.error_thresholds.push_back(yaml_lite::Document::to_double(v, "error_thresholds"));
    } else {
        param.error_thresholds.assign(param.trunc_dist_.begin(), param.trunc_dist_.end());
    }
    if (config.has("error_cdf_bins")) param.error_cdf_bins = config.as_int("error_cdf_bins");
    param.error_cdf_max = config.has("error_cdf_max") ? config.as_double("error_cdf_max") : param.icp_max_distance_;
    if (config.has("error_gated")) param.error_gated = config.as_bool("error_gated");
    if (param.evaluate_error_distribution) {
        if (!error_not_a_list.empty()) throw std::runtime_error(error_not_a_list + ": must be a list [a, b, ...]");
        if (param.error_quantiles.size() > ME_RANK_MAX) throw std::runtime_error("error_quantiles: at most 16 values");
        for (const double q : param.error_quantiles)
            if (!(q >= 0.0 && q <= 1.0)) throw std::runtime_error("error_quantiles: every value must lie in [0, 1]");
        if (param.error_thresholds.size() > ME_ERRDIST_MAX_THRESHOLDS) throw std::runtime_error("error_thresholds: at most 8 values");
        for (const double t : param.error_thresholds)
            if (!(t >= 0.0) || !std::isfinite(t)) throw std::runtime_error("error_thresholds: every value must be finite and >= 0");
        if (param.error_cdf_bins < 0 || param.error_cdf_bins > ME_ERRDIST_MAX_BINS) throw std::runtime_error("error_cdf_bins: must lie in 0..4096");
        if (param.error_cdf_bins > 0 && (!(param.error_cdf_max > 0) || !std::isfinite(param.error_cdf_max)))
            throw std::runtime_error("error_cdf_max: must be > 0");
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_error_distribution: single GPU only (num_gpus must be 1)");
    }
    // the normal-aware map error (no reference counterpart)
    if (config.has("evaluate_surface_error")) param.evaluate_surface_error = config.as_bool("evaluate_surface_error");
    param.normal_radius = config.has("normal_radius") ? config.as_double("normal_radius") : param.nn_radius_;
    if (config.has("normal_min_points")) param.normal_min_points = config.as_int("normal_min_points");
    std::string surface_not_a_list;
    for (const char *key : {"surface_thresholds", "surface_angles_deg"})
        if (config.has(key) && (!config.at(key).scalar.empty() || !config.at(key).rows.empty()) && surface_not_a_list.empty()) surface_not_a_list = key;
    if (config.has("surface_thresholds")) {
        for (const auto &v : config.at("surface_thresholds").seq) param.surface_thresholds.push_back(yaml_lite::Document::to_double(v, "surface_thresholds"));
    } else {
        param.surface_thresholds.assign(param.trunc_dist_.begin(), param.trunc_dist_.end());
    }
    if (config.has("surface_angles_deg")) {
        param.surface_angles_deg.clear();
        for (const auto &v : config.at("surface_angles_deg").seq) param.surface_angles_deg.push_back(yaml_lite::Document::to_double(v, "surface_angles_deg"));
    }
    if (config.has("surface_gated")) param.surface_gated = config.as_bool("surface_gated");
    if (param.evaluate_surface_error) {
        if (!surface_not_a_list.empty()) throw std::runtime_error(surface_not_a_list + ": must be a list [a, b, ...]");
        if (!(param.normal_radius > 0) || !std::isfinite(param.normal_radius)) throw std::runtime_error("normal_radius: must be > 0");
        if (param.normal_min_points < 2) throw std::runtime_error("normal_min_points: must be >= 2 (the covariance divides by k - 1)");
        if (param.surface_thresholds.size() > ME_ERRDIST_MAX_THRESHOLDS) throw std::runtime_error("surface_thresholds: at most 8 values");
        for (const double t : param.surface_thresholds)
            if (!(t >= 0.0) || !std::isfinite(t)) throw std::runtime_error("surface_thresholds: every value must be finite and >= 0");
        if (param.surface_angles_deg.size() > ME_SURFACE_MAX_ANGLES) throw std::runtime_error("surface_angles_deg: at most 8 values");
        for (const double a : param.surface_angles_deg)
            if (!(a >= 0.0 && a <= 90.0)) throw std::runtime_error("surface_angles_deg: every value must lie in [0, 90]");
        if (!param.evaluate_using_initial_)
            throw std::runtime_error("evaluate_surface_error: needs evaluate_using_initial (the registration path estimates and uses normals of its own)");
        if (param.evaluate_noised_gt_) throw std::runtime_error("evaluate_surface_error: not with evaluate_noised_gt");
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_surface_error: single GPU only (num_gpus must be 1)");
    }
    // M3C2 (no reference counterpart)
    if (config.has("evaluate_m3c2")) param.evaluate_m3c2 = config.as_bool("evaluate_m3c2");
    param.m3c2_normal_radius = config.has("m3c2_normal_radius") ? config.as_double("m3c2_normal_radius") : param.nn_radius_;
    param.m3c2_projection_radius = config.has("m3c2_projection_radius") ? config.as_double("m3c2_projection_radius") : param.nn_radius_;
    param.m3c2_max_depth = config.has("m3c2_max_depth") ? config.as_double("m3c2_max_depth") : 4.0 * param.nn_radius_;
    if (config.has("m3c2_min_points")) param.m3c2_min_points = config.as_int("m3c2_min_points");
    if (config.has("m3c2_reg_error")) param.m3c2_reg_error = config.as_double("m3c2_reg_error");
    if (config.has("m3c2_core_every")) param.m3c2_core_every = config.as_int("m3c2_core_every");
    if (param.evaluate_m3c2) {
        if (!(param.m3c2_normal_radius > 0) || !std::isfinite(param.m3c2_normal_radius)) throw std::runtime_error("m3c2_normal_radius: must be > 0");
        if (!(param.m3c2_projection_radius > 0) || !std::isfinite(param.m3c2_projection_radius))
            throw std::runtime_error("m3c2_projection_radius: must be > 0");
        if (!(param.m3c2_max_depth > 0) || !std::isfinite(param.m3c2_max_depth)) throw std::runtime_error("m3c2_max_depth: must be > 0");
        if (param.m3c2_min_points < 2) throw std::runtime_error("m3c2_min_points: must be >= 2 (the variance divides by n - 1)");
        if (!(param.m3c2_reg_error >= 0) || !std::isfinite(param.m3c2_reg_error)) throw std::runtime_error("m3c2_reg_error: must be >= 0");
        if (param.m3c2_core_every < 1) throw std::runtime_error("m3c2_core_every: must be >= 1");
        if (!param.evaluate_using_initial_)
            throw std::runtime_error("evaluate_m3c2: needs evaluate_using_initial (the clouds are compared where initial_matrix puts them)");
        if (param.evaluate_noised_gt_) throw std::runtime_error("evaluate_m3c2: not with evaluate_noised_gt");
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_m3c2: single GPU only (num_gpus must be 1)");
    }
    // per-voxel rigid deformation field (me_voxel_deformation; no reference counterpart)
    if (config.has("evaluate_deformation")) param.evaluate_deformation = config.as_bool("evaluate_deformation");
    param.deformation_voxel_size = config.has("deformation_voxel_size") ? config.as_double("deformation_voxel_size") : param.vmd_voxel_size_;
    param.deformation_max_distance = config.has("deformation_max_distance") ? config.as_double("deformation_max_distance")
                                     : (param.icp_max_distance_ > 0 ? std::sqrt(param.icp_max_distance_) : INFINITY);
    if (config.has("deformation_min_pairs")) param.deformation_min_pairs = (int) config.as_double("deformation_min_pairs");
    param.deformation_min_spread = config.has("deformation_min_spread") ? config.as_double("deformation_min_spread") : param.deformation_voxel_size / 20.0;
    if (param.evaluate_deformation) {
        if (!(param.deformation_voxel_size > 0) || !std::isfinite(param.deformation_voxel_size)) throw std::runtime_error("deformation_voxel_size: must be > 0");
        if (!(param.deformation_max_distance > 0)) throw std::runtime_error("deformation_max_distance: must be > 0");
        if (param.deformation_min_pairs < 3) throw std::runtime_error("deformation_min_pairs: must be >= 3");
        if (!(param.deformation_min_spread >= 0)) throw std::runtime_error("deformation_min_spread: must be >= 0");
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_deformation: single GPU only (num_gpus must be 1)");
    }
    // per-voxel distribution distances on the AWD lattice (me_voxel_distances; no reference counterpart)
    if (config.has("evaluate_voxel_distances")) param.evaluate_voxel_distances = config.as_bool("evaluate_voxel_distances");
    if (config.has("mmd_sigmas")) {
        if (!config.at("mmd_sigmas").scalar.empty() || !config.at("mmd_sigmas").rows.empty()) throw std::runtime_error("mmd_sigmas: must be a list of 1 to 4 numbers");
        for (const auto &v : config.at("mmd_sigmas").seq) param.mmd_sigmas.push_back(yaml_lite::Document::to_double(v, "mmd_sigmas"));
    } else {
        param.mmd_sigmas.assign(1, param.nn_radius_);
    }
    if (config.has("mmd_max_points")) param.mmd_max_points = (long long) config.as_double("mmd_max_points");
    if (config.has("voxel_distance_eig_floor")) param.voxel_distance_eig_floor = config.as_double("voxel_distance_eig_floor");
    if (param.evaluate_voxel_distances) {
        if (param.mmd_sigmas.empty() || param.mmd_sigmas.size() > 4) throw std::runtime_error("mmd_sigmas: must be a list of 1 to 4 numbers");
        for (const double sg : param.mmd_sigmas)
            if (!(sg > 0) || !std::isfinite(sg)) throw std::runtime_error("mmd_sigmas: every bandwidth must be > 0");
        if (param.mmd_max_points < 0 || (param.mmd_max_points >= 1 && param.mmd_max_points <= 10))
            throw std::runtime_error("mmd_max_points: must be 0 (all points) or >= 11");
        if (!(param.voxel_distance_eig_floor > 0) || !std::isfinite(param.voxel_distance_eig_floor))
            throw std::runtime_error("voxel_distance_eig_floor: must be > 0");
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_voxel_distances: single GPU only (num_gpus must be 1)");
    }
    // per-voxel point-set Wasserstein distances on the AWD lattice (me_voxel_transport; no reference counterpart)
    if (config.has("evaluate_voxel_transport")) param.evaluate_voxel_transport = config.as_bool("evaluate_voxel_transport");
    param.transport_blur = config.has("transport_blur") ? config.as_double("transport_blur") : param.nn_radius_;
    if (config.has("transport_directions")) param.transport_directions = (int) config.as_double("transport_directions");
    if (config.has("transport_max_points")) param.transport_max_points = (long long) config.as_double("transport_max_points");
    if (config.has("transport_scaling")) param.transport_scaling = config.as_double("transport_scaling");
    if (param.evaluate_voxel_transport) {
        if (!(param.transport_blur > 0) || !std::isfinite(param.transport_blur)) throw std::runtime_error("transport_blur: must be > 0");
        if (param.transport_directions < 0 || param.transport_directions > 64) throw std::runtime_error("transport_directions: must be in 0 .. 64");
        if (param.transport_max_points < 11 || param.transport_max_points > 1024) throw std::runtime_error("transport_max_points: must be in 11 .. 1024");
        if (!(param.transport_scaling > 0 && param.transport_scaling < 1)) throw std::runtime_error("transport_scaling: must be in (0, 1)");
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_voxel_transport: single GPU only (num_gpus must be 1)");
    }
    // cloud-to-mesh distance (the role of the reference's mesh branch, with a supplied mesh)
    if (config.has("evaluate_mesh_distance")) param.evaluate_mesh_distance = config.as_bool("evaluate_mesh_distance");
    if (config.has("gt_mesh_path")) param.gt_mesh_path = config.as_string("gt_mesh_path");
    const bool mesh_not_a_list = config.has("mesh_thresholds") && (!config.at("mesh_thresholds").scalar.empty() || !config.at("mesh_thresholds").rows.empty());
    if (config.has("mesh_thresholds")) {
        for (const auto &v : config.at("mesh_thresholds").seq) param.mesh_thresholds.push_back(yaml_lite::Document::to_double(v, "mesh_thresholds"));
    } else {
        param.mesh_thresholds.assign(param.trunc_dist_.begin(), param.trunc_dist_.end());
    }
    if (config.has("mesh_max_distance")) param.mesh_max_distance = config.as_double("mesh_max_distance");
    if (!(param.mesh_max_distance > 0)) param.mesh_max_distance = INFINITY;
    // whole non-negative numbers, read as integers (a seed uses all 64 bits; as_double would round it above 2^53)
    auto as_u64 = [&](const char *key, uint64_t &out) {
        const std::string v = config.as_string(key);
        char *end = nullptr;
        errno = 0;
        const unsigned long long x = std::strtoull(v.c_str(), &end, 10);
        if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || end != v.c_str() + v.size() || errno == ERANGE)
            throw std::runtime_error(std::string(key) + ": must be a whole number >= 0 (got '" + v + "')");
        out = (uint64_t) x;
    };
    if (config.has("mesh_sample_points")) {
        uint64_t n = 0;
        as_u64("mesh_sample_points", n);
        if (n >= (1ull << 31)) throw std::runtime_error("mesh_sample_points: must lie in 0 .. 2^31 - 1");
        param.mesh_sample_points = (int64_t) n;
    }
    if (config.has("mesh_seed")) as_u64("mesh_seed", param.mesh_seed);
    if (config.has("mesh_signed")) param.mesh_signed = config.as_bool("mesh_signed");
    if (param.mesh_signed && !param.evaluate_mesh_distance) throw std::runtime_error("mesh_signed: requires evaluate_mesh_distance: true");
    if (param.evaluate_mesh_distance) {
        if (mesh_not_a_list) throw std::runtime_error("mesh_thresholds: must be a list [a, b, ...]");
        if (param.gt_mesh_path.empty() && !(config.has("evaluate_mesh") && config.as_bool("evaluate_mesh")))
            throw std::runtime_error("gt_mesh_path: required with evaluate_mesh_distance");
        if (param.mesh_thresholds.size() > ME_MESH_MAX_THRESHOLDS) throw std::runtime_error("mesh_thresholds: at most 8 values");
        for (const double t : param.mesh_thresholds)
            if (!(t >= 0.0) || !std::isfinite(t)) throw std::runtime_error("mesh_thresholds: every value must be finite and >= 0");
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_mesh_distance: single GPU only (num_gpus must be 1)");
    }
    // surface reconstruction (the reference's eva_mesh / createMeshFromPCD)
    if (config.has("evaluate_mesh")) param.evaluate_mesh = config.as_bool("evaluate_mesh");
    if (config.has("mesh_voxel_size")) param.mesh_voxel_size = config.as_double("mesh_voxel_size");
    param.mesh_radius = config.has("mesh_radius") ? config.as_double("mesh_radius") : 3.0 * param.mesh_voxel_size;
    if (config.has("mesh_min_points")) param.mesh_min_points = config.as_int("mesh_min_points");
    if (config.has("mesh_band")) param.mesh_band = config.as_int("mesh_band");
    param.mesh_normal_radius = config.has("mesh_normal_radius") ? config.as_double("mesh_normal_radius") : param.nn_radius_;
    const bool viewpoint_not_a_list = config.has("mesh_viewpoint") && (!config.at("mesh_viewpoint").scalar.empty() || !config.at("mesh_viewpoint").rows.empty());
    if (config.has("mesh_viewpoint"))
        for (const auto &v : config.at("mesh_viewpoint").seq) param.mesh_viewpoint.push_back(yaml_lite::Document::to_double(v, "mesh_viewpoint"));
    if (config.has("mesh_orient")) param.mesh_orient = config.as_string("mesh_orient");
    const double orient_k = config.has("mesh_orient_k") ? config.as_double("mesh_orient_k") : (double) param.mesh_orient_k;
    const bool orient_k_ok = orient_k >= 1.0 && orient_k <= 39.0 && orient_k == std::floor(orient_k);
    if (orient_k_ok) param.mesh_orient_k = (int) orient_k;  // (judged below, with the stage on; the stage off, a bad value leaves the default)
    if (config.has("mesh_orient_inward")) param.mesh_orient_inward = config.as_bool("mesh_orient_inward");
    if (param.evaluate_mesh) {
        if (param.mesh_orient != "viewpoint" && param.mesh_orient != "propagate")
            throw std::runtime_error("mesh_orient: expected viewpoint or propagate, got '" + param.mesh_orient + "'");
        if (!orient_k_ok) throw std::runtime_error("mesh_orient_k: must be an integer in 1 .. 39");
        if (param.mesh_orient == "propagate" && config.has("mesh_viewpoint"))
            throw std::runtime_error("mesh_viewpoint: not with mesh_orient: propagate (the orientation is propagated from a root, no viewpoint is used)");
        if (!config.has("mesh_voxel_size")) throw std::runtime_error("mesh_voxel_size: required with evaluate_mesh");
        if (!(param.mesh_voxel_size > 0) || !std::isfinite(param.mesh_voxel_size)) throw std::runtime_error("mesh_voxel_size: must be finite and > 0");
        if (!(param.mesh_radius >= param.mesh_voxel_size) || !std::isfinite(param.mesh_radius))
            throw std::runtime_error("mesh_radius: must be finite and >= mesh_voxel_size");
        if (param.mesh_min_points < 1) throw std::runtime_error("mesh_min_points: must be >= 1");
        if (param.mesh_band < 0 || param.mesh_band > 2) throw std::runtime_error("mesh_band: must be 0, 1 or 2");
        if (!(param.mesh_normal_radius > 0) || !std::isfinite(param.mesh_normal_radius)) throw std::runtime_error("mesh_normal_radius: must be finite and > 0");
        if (param.normal_min_points < 2) throw std::runtime_error("normal_min_points: must be >= 2 (the covariance divides by k - 1)");
        if (viewpoint_not_a_list || (config.has("mesh_viewpoint") && param.mesh_viewpoint.size() != 3))
            throw std::runtime_error("mesh_viewpoint: must be a list of 3 values [x, y, z]");
        for (const double v : param.mesh_viewpoint)
            if (!std::isfinite(v)) throw std::runtime_error("mesh_viewpoint: every value must be finite");
        if (param.evaluate_noised_gt_) throw std::runtime_error("evaluate_mesh: not with evaluate_noised_gt");
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_mesh: single GPU only (num_gpus must be 1)");
    }
    // completeness against the observable ground truth (me_cloud_visibility from the poses of a trajectory)
    if (config.has("evaluate_observable")) param.evaluate_observable = config.as_bool("evaluate_observable");
    if (config.has("trajectory_path")) param.trajectory_path = config.as_string("trajectory_path");
    const double obs_stride = config.has("observable_pose_stride") ? config.as_double("observable_pose_stride") : 1.0;
    const bool obs_stride_ok = obs_stride >= 1.0 && obs_stride <= 2147483647.0 && obs_stride == std::floor(obs_stride);
    if (obs_stride_ok) param.observable_pose_stride = (int) obs_stride;  // (judged below, with the stage on)
    if (config.has("observable_max_range")) param.observable_max_range = config.as_double("observable_max_range");
    if (!(param.observable_max_range > 0)) param.observable_max_range = INFINITY;
    if (config.has("observable_tolerance")) param.observable_tolerance = config.as_double("observable_tolerance");
    const bool obs_not_a_list =
        config.has("observable_thresholds") && (!config.at("observable_thresholds").scalar.empty() || !config.at("observable_thresholds").rows.empty());
    if (config.has("observable_thresholds")) {
        for (const auto &v : config.at("observable_thresholds").seq)
            param.observable_thresholds.push_back(yaml_lite::Document::to_double(v, "observable_thresholds"));
    } else {
        param.observable_thresholds.assign(param.trunc_dist_.begin(), param.trunc_dist_.end());
    }
    if (param.evaluate_observable) {
        if (param.num_gpus > 1) throw std::runtime_error("evaluate_observable: single GPU only (num_gpus must be 1)");
        if (param.trajectory_path.empty()) throw std::runtime_error("trajectory_path: required with evaluate_observable");
        if (param.gt_mesh_path.empty() && !param.evaluate_mesh)
            throw std::runtime_error("evaluate_observable: needs a mesh (gt_mesh_path, or evaluate_mesh: true for the reconstructed ground-truth mesh)");
        if (!obs_stride_ok) throw std::runtime_error("observable_pose_stride: must be an integer >= 1");
        if (!(param.observable_tolerance >= 0) || !std::isfinite(param.observable_tolerance))
            throw std::runtime_error("observable_tolerance: must be finite and >= 0");
        if (obs_not_a_list) throw std::runtime_error("observable_thresholds: must be a list [a, b, ...]");
        if (param.observable_thresholds.size() > ME_ERRDIST_MAX_THRESHOLDS) throw std::runtime_error("observable_thresholds: at most 8 values");
        for (const double t : param.observable_thresholds)
            if (!(t >= 0.0) || !std::isfinite(t)) throw std::runtime_error("observable_thresholds: every value must be finite and >= 0");
    }
    return param;
}

std::string paramToJson(const Param &p) {
    std::ostringstream o;
    o << std::setprecision(17);
    auto b = [](bool v) { return v ? "true" : "false"; };
    o << "{\"registration_methods\": " << p.evaluation_method_ << ", \"icp_max_distance\": " << p.icp_max_distance_
      << ", \"accuracy_level\": [";
    for (int i = 0; i < 5; ++i) o << (i ? ", " : "") << p.trunc_dist_[i];
    o << "], \"initial_matrix\": [";
    for (int i = 0; i < 16; ++i) o << (i ? ", " : "") << p.initial_matrix_[i];
    o << "], \"save_immediate_result\": " << b(p.save_immediate_result_) << ", \"evaluate_mme\": " << b(p.evaluate_mme_)
      << ", \"evaluate_gt_mme\": " << b(p.evaluate_gt_mme_) << ", \"evaluate_using_initial\": " << b(p.evaluate_using_initial_)
      << ", \"nn_radius\": " << p.nn_radius_ << ", \"vmd_voxel_size\": " << p.vmd_voxel_size_
      << ", \"downsample_size\": " << p.downsample_size << ", \"estimate_map_path\": \"" << p.evaluation_map_pcd_path_
      << "\", \"gt_map_path\": \"" << p.map_gt_path_ << "\", \"scene_name\": \"" << p.name_ << "\", \"pcd_file_name\": \""
      << p.pcd_file_name_ << "\", \"enable_debug\": " << b(p.enable_debug) << ", \"use_tbb_mme\": " << b(p.use_tbb_mme)
      << ", \"use_visualization\": " << b(p.use_visualization) << ", \"result_path\": \"" << p.result_path_
      << "\", \"gpu_device\": " << p.gpu_device << ", \"strict_reference\": " << b(p.strict_reference) << ", \"num_gpus\": " << p.num_gpus
      << ", \"save_voxel_metrics\": " << b(p.save_voxel_metrics) << ", \"evaluate_noised_gt\": " << b(p.evaluate_noised_gt_)
      << ", \"noise_std_dev\": " << p.noise_std_dev_ << ", \"noise_seed\": " << p.noise_seed << ", \"noise_sparse_ratio\": " << p.noise_sparse_ratio
      << ", \"noise_dense_ratio\": " << p.noise_dense_ratio << ", \"noise_region_size\": " << p.noise_region_size
      << ", \"noise_outlier_ratio\": " << p.noise_outlier_ratio << ", \"noise_outlier_range\": " << p.noise_outlier_range
      << ", \"noise_deform_radius\": " << p.noise_deform_radius << ", \"noise_deform_strength\": " << p.noise_deform_strength
      << ", \"noise_deform_center\": [" << p.noise_deform_center[0] << ", " << p.noise_deform_center[1] << ", " << p.noise_deform_center[2]
      << "], \"noise_sweep\": [";
    for (size_t i = 0; i < p.noise_sweep.size(); ++i) o << (i ? ", " : "") << p.noise_sweep[i];
    o << "], \"global_registration\": " << b(p.global_registration) << ", \"global_voxel_size\": " << p.global_voxel_size
      << ", \"global_feature_radius\": " << p.global_feature_radius << ", \"global_max_nn\": " << p.global_max_nn
      << ", \"global_normal_knn\": " << p.global_normal_knn << ", \"global_max_corr_dist\": " << p.global_max_corr_dist
      << ", \"global_max_iterations\": " << p.global_max_iterations << ", \"global_edge_ratio\": " << p.global_edge_ratio
      << ", \"global_mutual_filter\": " << b(p.global_mutual_filter) << ", \"global_seed\": " << p.global_seed
      << ", \"global_min_fitness\": " << p.global_min_fitness << ", \"global_outlier_nb_neighbors\": " << p.global_outlier_nb_neighbors
      << ", \"global_outlier_std_ratio\": " << p.global_outlier_std_ratio << ", \"remove_outliers\": \"" << p.remove_outliers
      << "\", \"outlier_nb_neighbors\": " << p.outlier_nb_neighbors << ", \"outlier_std_ratio\": " << p.outlier_std_ratio
      << ", \"outlier_nb_points\": " << p.outlier_nb_points << ", \"outlier_radius\": " << p.outlier_radius
      << ", \"outlier_filter_gt\": " << b(p.outlier_filter_gt) << ", \"outlier_eps\": " << p.outlier_eps
      << ", \"outlier_min_points\": " << p.outlier_min_points << ", \"outlier_min_cluster_size\": " << p.outlier_min_cluster_size
      << ", \"outlier_keep_largest\": " << p.outlier_keep_largest << ", \"evaluate_mpv\": " << b(p.evaluate_mpv)
      << ", \"mpv_radius\": " << p.mpv_radius << ", \"mpv_min_points\": " << p.mpv_min_points << ", \"evaluate_gt_mpv\": " << b(p.evaluate_gt_mpv)
      << ", \"segment_planes\": " << b(p.segment_planes) << ", \"plane_distance_threshold\": " << p.plane_distance_threshold
      << ", \"plane_num_iterations\": " << p.plane_num_iterations << ", \"plane_max_planes\": " << p.plane_max_planes
      << ", \"plane_min_inliers\": " << p.plane_min_inliers << ", \"plane_seed\": " << p.plane_seed << ", \"plane_refit\": " << b(p.plane_refit)
      << ", \"segment_gt_planes\": " << b(p.segment_gt_planes) << ", \"evaluate_mom\": " << b(p.evaluate_mom)
      << ", \"mom_parallel_deg\": " << p.mom_parallel_deg << ", \"mom_orthogonal_deg\": " << p.mom_orthogonal_deg
      << ", \"mom_min_axis_points\": " << p.mom_min_axis_points << ", \"evaluate_gt_mom\": " << b(p.evaluate_gt_mom)
      << ", \"evaluate_error_distribution\": " << b(p.evaluate_error_distribution) << ", \"error_quantiles\": [";
    for (size_t i = 0; i < p.error_quantiles.size(); ++i) o << (i ? ", " : "") << p.error_quantiles[i];
    o << "], \"error_thresholds\": [";
    for (size_t i = 0; i < p.error_thresholds.size(); ++i) o << (i ? ", " : "") << p.error_thresholds[i];
    o << "], \"error_cdf_bins\": " << p.error_cdf_bins << ", \"error_cdf_max\": " << p.error_cdf_max << ", \"error_gated\": " << b(p.error_gated)
      << ", \"evaluate_surface_error\": " << b(p.evaluate_surface_error) << ", \"normal_radius\": " << p.normal_radius
      << ", \"normal_min_points\": " << p.normal_min_points << ", \"surface_thresholds\": [";
    for (size_t i = 0; i < p.surface_thresholds.size(); ++i) o << (i ? ", " : "") << p.surface_thresholds[i];
    o << "], \"surface_angles_deg\": [";
    for (size_t i = 0; i < p.surface_angles_deg.size(); ++i) o << (i ? ", " : "") << p.surface_angles_deg[i];
    o << "], \"surface_gated\": " << b(p.surface_gated) << ", \"evaluate_m3c2\": " << b(p.evaluate_m3c2) << ", \"evaluate_deformation\": " << b(p.evaluate_deformation)
      << ", \"m3c2_normal_radius\": " << p.m3c2_normal_radius << ", \"m3c2_projection_radius\": " << p.m3c2_projection_radius
      << ", \"m3c2_max_depth\": " << p.m3c2_max_depth << ", \"m3c2_min_points\": " << p.m3c2_min_points
      << ", \"m3c2_reg_error\": " << p.m3c2_reg_error << ", \"m3c2_core_every\": " << p.m3c2_core_every
      << ", \"evaluate_mesh_distance\": " << b(p.evaluate_mesh_distance) << ", \"gt_mesh_path\": \"";
    for (const char c : p.gt_mesh_path) {  // (a path may hold a quote or a backslash)
        if (c == '"' || c == '\\') o << '\\' << c;
        else if ((unsigned char) c < 0x20) o << "\\u00" << "0123456789abcdef"[(c >> 4) & 15] << "0123456789abcdef"[c & 15];
        else o << c;
    }
    o << "\", \"mesh_thresholds\": [";
    for (size_t i = 0; i < p.mesh_thresholds.size(); ++i) o << (i ? ", " : "") << p.mesh_thresholds[i];
    o << "], \"mesh_max_distance\": ";
    if (std::isinf(p.mesh_max_distance)) o << "Infinity";  // (what Python's json reads as inf)
    else o << p.mesh_max_distance;
    o << ", \"mesh_sample_points\": " << p.mesh_sample_points << ", \"mesh_seed\": " << p.mesh_seed
      << ", \"mesh_signed\": " << b(p.mesh_signed);
    o << ", \"evaluate_mesh\": " << b(p.evaluate_mesh) << ", \"mesh_voxel_size\": " << p.mesh_voxel_size << ", \"mesh_radius\": " << p.mesh_radius
      << ", \"mesh_min_points\": " << p.mesh_min_points << ", \"mesh_band\": " << p.mesh_band << ", \"mesh_normal_radius\": "
      << p.mesh_normal_radius << ", \"mesh_viewpoint\": ";
    if (p.mesh_viewpoint.empty()) o << "null";  // (the centre of each cloud's bounding box)
    else o << "[" << p.mesh_viewpoint[0] << ", " << p.mesh_viewpoint[1] << ", " << p.mesh_viewpoint[2] << "]";
    o << ", \"mesh_orient\": \"";
    for (const char c : p.mesh_orient) {  // (judged only with evaluate_mesh: the stage off, any text passes through)
        if (c == '"' || c == '\\') o << '\\' << c;
        else if ((unsigned char) c < 0x20) o << ' ';
        else o << c;
    }
    o << "\", \"mesh_orient_k\": " << p.mesh_orient_k << ", \"mesh_orient_inward\": " << b(p.mesh_orient_inward);
    o << ", \"evaluate_voxel_distances\": " << b(p.evaluate_voxel_distances) << ", \"mmd_sigmas\": [";
    for (size_t i = 0; i < p.mmd_sigmas.size(); ++i) o << (i ? ", " : "") << p.mmd_sigmas[i];
    o << "], \"mmd_max_points\": " << p.mmd_max_points << ", \"voxel_distance_eig_floor\": " << p.voxel_distance_eig_floor;
    o << ", \"evaluate_voxel_transport\": " << b(p.evaluate_voxel_transport) << ", \"transport_blur\": " << p.transport_blur
      << ", \"transport_directions\": " << p.transport_directions << ", \"transport_max_points\": " << p.transport_max_points
      << ", \"transport_scaling\": " << p.transport_scaling;
    o << ", \"evaluate_observable\": " << b(p.evaluate_observable) << ", \"trajectory_path\": \"";
    for (const char c : p.trajectory_path) {
        if (c == '"' || c == '\\') o << '\\' << c;
        else if ((unsigned char) c < 0x20) o << ' ';
        else o << c;
    }
    o << "\", \"observable_pose_stride\": " << p.observable_pose_stride << ", \"observable_max_range\": ";
    if (std::isinf(p.observable_max_range)) o << "Infinity";
    else o << p.observable_max_range;
    o << ", \"observable_tolerance\": " << p.observable_tolerance << ", \"observable_thresholds\": [";
    for (size_t i = 0; i < p.observable_thresholds.size(); ++i) o << (i ? ", " : "") << p.observable_thresholds[i];
    o << "]";
    o << "}";
    return o.str();
}

// ---------------------------------------------------------------------------------------------------------------
MapEval::MapEval(Param &param) : param_(param), map_3d_(new PointCloud), gt_3d_(new PointCloud) {
    // results sub-folder by file name (map_eval.h:143-155), created next to the estimated map (:158-164)
    if (param_.pcd_file_name_ == "merged_maps_all_trans.pcd") subfolder = "merged_maps_all_results/";
    else if (param_.pcd_file_name_ == "merged_maps_s0_trans.pcd") subfolder = "merged_maps_s0_results/";
    else if (param_.pcd_file_name_ == "merged_maps_s1_trans.pcd") subfolder = "merged_maps_s1_results/";
    else subfolder = "map_results/";
    results_subfolder = param_.evaluation_map_pcd_path_ + subfolder;
    std::cout << "INFO: Saving results to: " << results_subfolder << std::endl;
    std::error_code ec;
    if (!fs::exists(results_subfolder)) fs::create_directory(results_subfolder, ec);
    results_file_path = results_subfolder + "map_results.txt";
    if (param_.dist_rank > 0) results_file_path = "/dev/null";  // multi-GPU: rank 0 alone writes the result files
    file_result.open(results_file_path, std::ios::app);  // append mode (:168)
    if (!file_result.is_open()) std::cerr << "ERROR: Failed to open results file at " << results_file_path << std::endl;
    const std::time_t now_c = std::chrono::system_clock::to_time_t(std::chrono::system_clock::now());
    std::stringstream time_stream;
    time_stream << std::put_time(std::localtime(&now_c), "%Y-%m-%d %X");
    file_result << param_.name_ << " ===================== " << time_stream.str() << " ===================== " << std::endl;
    file_result << "Ground Truth Path: " << param_.map_gt_path_ << std::endl;
    file_result << "Evaluation Map Path: " << param_.evaluation_map_pcd_path_ + param_.pcd_file_name_ << std::endl;
    std::cout << "INFO: Evaluation details saved to " << results_file_path << std::endl;
}

MapEval::~MapEval() {
    if (render_ctx_) me_destroy(render_ctx_);
    if (ctx_) me_destroy(ctx_);
    file_result.close();
}

int MapEval::fail(const std::string &msg) {
    last_error = msg;
    std::cerr << "ERROR: " << msg << std::endl;
    return -1;
}

int MapEval::process() {
    TicToc tic_toc;
    std::string err;
    // ground truth: .pcd or .ply by extension (map_eval.cpp:9-17)
    const std::string ext = param_.map_gt_path_.substr(param_.map_gt_path_.find_last_of(".") + 1);
    bool ok_gt;
    std::vector<double> gt_normals;  // normal_x/y/z of the ground truth, if the file has them (point-to-plane ICP needs them)
    if (ext == "pcd") ok_gt = pcio::read_pcd(param_.map_gt_path_, gt_3d_->points_, &err, &gt_normals);
    else if (ext == "ply") ok_gt = pcio::read_ply(param_.map_gt_path_, gt_3d_->points_, &err, &gt_normals);
    else return fail("Unsupported ground truth file format: " + param_.map_gt_path_);
    if (!ok_gt) std::cerr << "WARNING: " << err << std::endl;
    // the estimated map's own normal_x/y/z, if its PCD has them: Open3D's InitializePointCloudForGeneralizedICP uses a
    // cloud's normals when it carries them and estimates them (KNN 20) only otherwise
    std::vector<double> map_normals;
    // evaluate_noised_gt: "the system do not load the estimate map, instead the noise gt_map will be used" (config.yaml): the map is
    // made from the resident ground truth below (me_perturb_cloud), so its file may be absent
    const bool noised = param_.evaluate_noised_gt_;
    if (!noised) {
        const bool success = pcio::read_pcd(param_.evaluation_map_pcd_path_ + param_.pcd_file_name_, map_3d_->points_, &err, &map_normals);
        if (param_.enable_debug)
            std::cout << "INFO: Loading map point cloud from: " << param_.evaluation_map_pcd_path_ + param_.pcd_file_name_ << std::endl;
        if (!success) return fail("Failed to load point cloud from the specified path.");
    }
    if ((!noised && map_3d_->IsEmpty()) || gt_3d_->IsEmpty()) return fail("One or both point clouds are empty!");

    // ---- the GPU engine: no CPU fallback ----
    ctx_ = me_create(param_.gpu_device, 0);
    if (!ctx_) {
        file_result << std::fixed << std::setprecision(15) << "Estimated-Ground Truth point count: " << map_3d_->size() << " / "
                    << gt_3d_->size() << std::endl;
        return fail(std::string("GPU engine unavailable: ") + me_last_error(nullptr));
    }
    // The initial-matrix evaluation on one GPU is ONE library call (processOneCall: me_run_suite_from): without down-sampling it
    // starts from the host clouds as they were read — the uploads are part of the call's two-lane schedule.
    const bool one_call = param_.evaluate_using_initial_ && !comm_;
    if (noised && comm_) return fail("evaluate_noised_gt: single GPU only (the multi-GPU path reads both maps from disk)");
    const bool filter = param_.remove_outliers != "none";  // (the filter runs on resident clouds: the uploads below, not the one call's)
    if (filter && (noised || comm_)) return fail("remove_outliers: single GPU only, and not with evaluate_noised_gt, for now");
    const bool mpv = param_.evaluate_mpv;  // (on resident clouds too, before the one call transforms the map)
    if (mpv && comm_) return fail("evaluate_mpv: single GPU only (num_gpus must be 1)");
    const bool planes = param_.segment_planes;  // (likewise)
    if (planes && comm_) return fail("segment_planes: single GPU only (num_gpus must be 1)");
    const bool mom = param_.evaluate_mom;  // (likewise)
    if (mom && comm_) return fail("evaluate_mom: single GPU only (num_gpus must be 1)");
    if (param_.evaluate_error_distribution && comm_) return fail("evaluate_error_distribution: single GPU only (num_gpus must be 1)");
    const bool surf = param_.evaluate_surface_error;  // (its normals are estimated on resident clouds, before the one call transforms the map)
    if (surf && comm_) return fail("evaluate_surface_error: single GPU only (num_gpus must be 1)");
    const bool m3c2 = param_.evaluate_m3c2;  // (on resident clouds, the map moved by initial_matrix for it alone)
    if (m3c2 && (comm_ || noised || !param_.evaluate_using_initial_))
        return fail("evaluate_m3c2: single GPU only, with evaluate_using_initial and not with evaluate_noised_gt");
    const bool mesh = param_.evaluate_mesh_distance;  // (on resident clouds, the map moved by initial_matrix for it alone)
    if (mesh && comm_) return fail("evaluate_mesh_distance: single GPU only (num_gpus must be 1)");
    const bool recon = param_.evaluate_mesh;  // (on resident clouds as loaded, first of all)
    if (recon && (comm_ || noised)) return fail("evaluate_mesh: single GPU only (num_gpus must be 1), and not with evaluate_noised_gt");
    const bool obs = param_.evaluate_observable;  // (on resident clouds, the map moved by initial_matrix for it alone, like the mesh stage)
    if (obs && comm_) return fail("evaluate_observable: single GPU only (num_gpus must be 1)");
    if (one_call && !noised && !filter && !mpv && !planes && !mom && !surf && !m3c2 && !mesh && !obs && !recon && !(param_.downsample_size > 0)) {
        file_result << std::fixed << std::setprecision(15) << "Estimated-Ground Truth point count: " << map_3d_->size() << " / "
                    << gt_3d_->size() << std::endl;
        if (param_.enable_debug)
            std::cout << "INFO: Loaded point clouds: " << map_3d_->size() << " points (Map), " << gt_3d_->size()
                      << " points (Ground Truth)." << std::endl;
        return processOneCall(true, tic_toc.toc());
    }
    if (me_upload_cloud(ctx_, ME_SLOT_GT, gt_3d_->points_.data(), (int64_t) gt_3d_->size(), nullptr, param_.nn_radius_) != ME_OK ||
        (!noised &&
         me_upload_cloud(ctx_, ME_SLOT_EST, map_3d_->points_.data(), (int64_t) map_3d_->size(), nullptr, param_.nn_radius_) != ME_OK))
        return fail(me_last_error(ctx_));
    if (gt_normals.size() == gt_3d_->points_.size() && !gt_normals.empty() &&
        me_set_normals(ctx_, ME_SLOT_GT, gt_normals.data()) != ME_OK)
        return fail(me_last_error(ctx_));
    if (map_normals.size() == map_3d_->points_.size() && !map_normals.empty() &&
        me_set_normals(ctx_, ME_SLOT_EST, map_normals.data()) != ME_OK)
        return fail(me_last_error(ctx_));
    // map_3d_ = map_3d_->VoxelDownSample(downsample_size) (:38-39), on the device (normals are averaged with the points)
    if (param_.downsample_size > 0) {
        int64_t ne = 0, ng = 0;
        if ((!noised && me_voxel_downsample(ctx_, ME_SLOT_EST, param_.downsample_size, &ne) != ME_OK) ||
            me_voxel_downsample(ctx_, ME_SLOT_GT, param_.downsample_size, &ng) != ME_OK)
            return fail(me_last_error(ctx_));
        map_3d_->points_.resize((size_t) ne * 3);
        gt_3d_->points_.resize((size_t) ng * 3);
        if ((!noised && me_download_cloud(ctx_, ME_SLOT_EST, map_3d_->points_.data()) != ME_OK) ||
            me_download_cloud(ctx_, ME_SLOT_GT, gt_3d_->points_.data()) != ME_OK)
            return fail(me_last_error(ctx_));
    }
    if (filter && removeOutliers() != 0) return -1;  // (right after the down-sample, before everything else)
    if (noised) {  // map_3d_ = the perturbed ground truth (map_eval.cpp:1745-1829); the host copy is what the writers read
        const me_perturb_params pp = perturbParams(param_.noise_std_dev_);
        int64_t ne = 0;
        if (me_perturb_cloud(ctx_, ME_SLOT_EST, ME_SLOT_GT, &pp, &ne) != ME_OK) return fail(me_last_error(ctx_));
        map_3d_->points_.resize((size_t) ne * 3);
        if (me_download_cloud(ctx_, ME_SLOT_EST, map_3d_->points_.data()) != ME_OK) return fail(me_last_error(ctx_));
    }
    file_result << std::fixed << std::setprecision(15) << "Estimated-Ground Truth point count: " << map_3d_->size() << " / "
                << gt_3d_->size() << std::endl;
    if (param_.enable_debug)
        std::cout << "INFO: Loaded point clouds: " << map_3d_->size() << " points (Map), " << gt_3d_->size()
                  << " points (Ground Truth)." << std::endl;
    if (recon) {
        // before every other stage, on the clouds as loaded: it replaces both clouds' normals and may re-index them at mesh_radius.  Both
        // clouds are then uploaded again from the host's copies with the normals their files brought (the restoration of the M3C2 block).
        if (computeReconstruction() != 0) return -1;
        if (me_upload_cloud(ctx_, ME_SLOT_GT, gt_3d_->points_.data(), (int64_t) gt_3d_->size(), nullptr, param_.nn_radius_) != ME_OK ||
            me_upload_cloud(ctx_, ME_SLOT_EST, map_3d_->points_.data(), (int64_t) map_3d_->size(), nullptr, param_.nn_radius_) != ME_OK)
            return fail(me_last_error(ctx_));
        if (!(param_.downsample_size > 0) && !filter) {
            if (gt_normals.size() == gt_3d_->points_.size() && !gt_normals.empty() && me_set_normals(ctx_, ME_SLOT_GT, gt_normals.data()) != ME_OK)
                return fail(me_last_error(ctx_));
            if (map_normals.size() == map_3d_->points_.size() && !map_normals.empty() &&
                me_set_normals(ctx_, ME_SLOT_EST, map_normals.data()) != ME_OK)
                return fail(me_last_error(ctx_));
        }
    }
    if (m3c2 || mesh || obs) {
        // (the mesh stage, like M3C2, moves the map and may replace the ground-truth slot by the mesh's sample: same restoration)
        // FIRST of the stages on the resident clouds: it moves the map, replaces both clouds' normals and re-indexes both at the
        // cylinder's bounding radius.  Both clouds are then uploaded again from the host's copies (the clouds as loaded: the map's is
        // still untransformed) with the normals their files brought, so that every later stage — the surface-error normals, the
        // one call's MME, transform and searches — starts from exactly the state it finds without this key.
        if (m3c2 && computeM3C2() != 0) return -1;
        if (m3c2 && mesh &&  // (M3C2 has moved the map already: the mesh stage starts from the map as loaded)
            me_upload_cloud(ctx_, ME_SLOT_EST, map_3d_->points_.data(), (int64_t) map_3d_->size(), nullptr, param_.nn_radius_) != ME_OK)
            return fail(me_last_error(ctx_));
        if (mesh && computeMeshDistance() != 0) return -1;
        if (obs) {  // (after the stages above, from the clouds as loaded: they moved the map and may have replaced the ground-truth slot)
            if ((m3c2 || mesh) &&
                (me_upload_cloud(ctx_, ME_SLOT_GT, gt_3d_->points_.data(), (int64_t) gt_3d_->size(), nullptr, param_.nn_radius_) != ME_OK ||
                 me_upload_cloud(ctx_, ME_SLOT_EST, map_3d_->points_.data(), (int64_t) map_3d_->size(), nullptr, param_.nn_radius_) != ME_OK))
                return fail(me_last_error(ctx_));
            if (computeObservable() != 0) return -1;
        }
        if (me_upload_cloud(ctx_, ME_SLOT_GT, gt_3d_->points_.data(), (int64_t) gt_3d_->size(), nullptr, param_.nn_radius_) != ME_OK ||
            me_upload_cloud(ctx_, ME_SLOT_EST, map_3d_->points_.data(), (int64_t) map_3d_->size(), nullptr, param_.nn_radius_) != ME_OK)
            return fail(me_last_error(ctx_));
        if (!(param_.downsample_size > 0) && !filter) {  // (a down-sampled or filtered cloud carried its normals on the device only: none of
            // the initial-matrix stages reads them)
            if (gt_normals.size() == gt_3d_->points_.size() && !gt_normals.empty() && me_set_normals(ctx_, ME_SLOT_GT, gt_normals.data()) != ME_OK)
                return fail(me_last_error(ctx_));
            if (map_normals.size() == map_3d_->points_.size() && !map_normals.empty() &&
                me_set_normals(ctx_, ME_SLOT_EST, map_normals.data()) != ME_OK)
                return fail(me_last_error(ctx_));
        }
    }
    if (mpv && computeMPV() != 0) return -1;  // (the clouds as loaded, where computeMME runs: before the transform)
    if (planes && segmentPlanes() != 0) return -1;  // (likewise)
    if (mom && computeMOM() != 0) return -1;  // (likewise; after its two inputs)
    // (last of the stages on the clouds as loaded: it may rebuild the indices at its own radius, and its normals then ride
    // me_transform_cloud and the one call — me_run_suite_from uploads nothing on this resident path, so it keeps them)
    if (surf && computeSurfaceNormals() != 0) return -1;
    if (comm_) return processDist(tic_toc.toc());  // num_gpus > 1 (map_eval_dist.cpp)
    if (one_call) {  // (the down-sampled or perturbed clouds are resident)
        const int rc = processOneCall(false, tic_toc.toc());
        if (rc != 0 || param_.noise_sweep.empty()) return rc;
        return runNoiseSweep();
    }
    t1 = tic_toc.toc();
    // The reference computes MME on the map as loaded (:56) and transforms it afterwards, inside
    // calculateMetricsWithInitialMatrix (:1206): same order here (me_transform_cloud below), skipped for an identity matrix.
    const double *T = param_.evaluate_using_initial_ ? param_.initial_matrix_.data() : nullptr;
    bool identity = true;
    for (int i = 0; i < 16 && T; ++i) identity = identity && (T[i] == ((i % 5 == 0) ? 1.0 : 0.0));

    if (param_.evaluate_mme_) {
        if (param_.enable_debug) std::cout << "INFO: Starting MME calculation..." << std::endl;
        computeMME(*map_3d_, *gt_3d_);
        if (!last_error.empty()) return -1;
        if (param_.save_immediate_result_) saveMmeResults();
        t2 = tic_toc.toc();
        if (param_.enable_debug) std::cout << "INFO: MME calculation completed in: " << (t2 - t1) / 1000.0 << " seconds." << std::endl;
    } else {
        t2 = t1;
    }
    if (mpv && param_.save_immediate_result_) saveMpvResults();
    if (planes && param_.save_immediate_result_) savePlaneResults();
    if (mom && param_.save_immediate_result_) saveMomResults();

    if (param_.evaluate_using_initial_) {
        if (param_.enable_debug) std::cout << "INFO: Using initial matrix without registration." << std::endl;
        if (T && !identity) {  // *map_3d_ = map_3d_->Transform(param_.initial_matrix_) (:1206)
            if (me_transform_cloud(ctx_, ME_SLOT_EST, T) != ME_OK ||
                me_download_cloud(ctx_, ME_SLOT_EST, map_3d_->points_.data()) != ME_OK)
                return fail(me_last_error(ctx_));
        }
        calculateMetricsWithInitialMatrix();
        if (!last_error.empty()) return -1;
    } else {
        // performRegistration (map_eval.cpp:191-237): point-to-point (0), point-to-plane (1) and generalized ICP (2) all run
        // on the device-side correspondence + reduction step; the small solve per iteration is done here.
        if (param_.evaluation_method_ < 0 || param_.evaluation_method_ > 2)
            return fail("Invalid registration type specified");  // (:1385-1387)
        if (performRegistration() != 0) return -1;
    }
    if (param_.evaluate_using_initial_) t5 = t4 = t3 = tic_toc.toc();

    calculateVMD();
    if (!last_error.empty()) return -1;
    if (param_.evaluate_deformation && computeDeformation() != 0) return -1;
    if (param_.evaluate_voxel_distances && computeVoxelDistances() != 0) return -1;
    if (param_.evaluate_voxel_transport && computeVoxelTransport() != 0) return -1;
    if (param_.save_voxel_metrics) {  // (only the registration path gets here on one GPU: the initial-matrix one is processOneCall)
        // the transforms of the registration discarded the map's MME result on the device: hand back the entropies computeMME
        // fetched (those of map_entropy.txt), and the ground truth's with them
        if (param_.evaluate_mme_ &&
            me_set_mme_result(ctx_, ME_SLOT_EST, est_entropies.data(), valid_entropy_points.data()) != ME_OK)
            return fail(me_last_error(ctx_));
        if (param_.evaluate_mme_ && param_.evaluate_gt_mme_ &&
            me_set_mme_result(ctx_, ME_SLOT_GT, gt_entropies.data(), gt_valid_entropy_points.data()) != ME_OK)
            return fail(me_last_error(ctx_));
        saveVoxelMetrics(ME_GATE_LT_SQUARED);  // the gate of calculateMetrics (:1168)
        if (!last_error.empty()) return -1;
    }
    if (param_.enable_debug) std::cout << "INFO: VMD calculation completed." << std::endl;
    if (param_.save_immediate_result_) saveRegistrationResults();
    if (param_.enable_debug) std::cout << "INFO: Results saved successfully." << std::endl;
    return 0;
}

namespace {

// Optimal rigid update (row-major 4x4, absolute coordinates) from the me_icp_sums block: Horn's closed form, which gives
// the same rotation as Eigen::umeyama without scaling (TransformationEstimationPointToPoint [Open3D, upstream]).
void kabsch_from_sums(const me_icp_sums &s, double T[16]) {
    const double n = (double) s.n_corr;
    double pb[3], qb[3], S[9];
    for (int k = 0; k < 3; ++k) {
        pb[k] = s.sum_p[k] / n;
        qb[k] = s.sum_q[k] / n;
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) S[3 * r + c] = s.sum_pq[3 * r + c] - n * pb[r] * qb[c];  // sum (p-pb)(q-qb)^T
    double R[9];
    me::horn_rotation(S, R);  // csrc/me_horn.hpp (shared with the device RANSAC fit)
    // x -> o + R (x - o - pb) + qb
    for (int i = 0; i < 16; ++i) T[i] = (i == 15) ? 1.0 : 0.0;
    for (int r = 0; r < 3; ++r) {
        double t = s.origin[r] + qb[r];
        for (int c = 0; c < 3; ++c) {
            T[4 * r + c] = R[3 * r + c];
            t -= R[3 * r + c] * (s.origin[c] + pb[c]);
        }
        T[4 * r + 3] = t;
    }
}

// utility::SolveJacobianSystemAndObtainExtrinsicMatrix [Open3D, upstream]: x = solve(JTJ, -JTr) (LDLT there, Gaussian
// elimination with partial pivoting here), then TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0), t = x[3..5].
// A singular system leaves the identity (ComputeTransformation's failure value).
void lsq_update(const me_icp_lsq &q, double T[16]) {
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    double A[6][7];
    for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) A[r][c] = q.JTJ[6 * r + c];
        A[r][6] = -q.JTr[r];
    }
    for (int k = 0; k < 6; ++k) {
        int piv = k;
        for (int r = k + 1; r < 6; ++r)
            if (std::fabs(A[r][k]) > std::fabs(A[piv][k])) piv = r;
        if (A[piv][k] == 0.0 || !std::isfinite(A[piv][k])) return;
        if (piv != k)
            for (int c = 0; c < 7; ++c) std::swap(A[piv][c], A[k][c]);
        for (int r = k + 1; r < 6; ++r) {
            const double f = A[r][k] / A[k][k];
            for (int c = k; c < 7; ++c) A[r][c] -= f * A[k][c];
        }
    }
    double x[6];
    for (int k = 5; k >= 0; --k) {
        double acc = A[k][6];
        for (int c = k + 1; c < 6; ++c) acc -= A[k][c] * x[c];
        x[k] = acc / A[k][k];
        if (!std::isfinite(x[k])) return;
    }
    const double ca = std::cos(x[0]), sa = std::sin(x[0]), cb = std::cos(x[1]), sb = std::sin(x[1]), cg = std::cos(x[2]),
                 sg = std::sin(x[2]);
    // Rz(g) * Ry(b) * Rx(a)
    T[0] = cg * cb;
    T[1] = cg * sb * sa - sg * ca;
    T[2] = cg * sb * ca + sg * sa;
    T[4] = sg * cb;
    T[5] = sg * sb * sa + cg * ca;
    T[6] = sg * sb * ca - cg * sa;
    T[8] = -sb;
    T[9] = cb * sa;
    T[10] = cb * ca;
    T[3] = x[3];
    T[7] = x[4];
    T[11] = x[5];
}

void matmul4(const double A[16], const double B[16], double C[16]) {
    double out[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double acc = 0;
            for (int k = 0; k < 4; ++k) acc += A[4 * r + k] * B[4 * k + c];
            out[4 * r + c] = acc;
        }
    for (int i = 0; i < 16; ++i) C[i] = out[i];
}

}  // namespace

int MapEval::performRegistration(bool metrics) {
    // RegistrationICP(*map_3d_, *gt_3d_, icp_max_distance_, initial_matrix_, PointToPoint, ICPConvergenceCriteria())
    // (map_eval.cpp:1369-1371): relative_fitness = relative_rmse = 1e-6, max_iteration = 30 [Open3D defaults, upstream]
    // Multi-GPU (comm_): both clouds are resident on every rank, the correspondence searches are sharded over the ranks
    // (me_set_shard: rank r searches the r-th share of the curve-sorted map), the step's additive sums are all-reduced, every rank
    // solves the same small system and moves its copy of the map: the iterates are those of the single-GPU loop up to the order
    // in which the sums are added.
    TicToc tic_toc;
    const bool root = param_.dist_rank == 0;
    if (comm_ && me_set_shard(ctx_, comm_->rank, comm_->world) != ME_OK) return fail(me_last_error(ctx_));
    for (int i = 0; i < 16; ++i) trans[i] = param_.initial_matrix_[i];
    if (param_.global_registration && !comm_) {  // ICP starts from T_c * initial_matrix (the map as loaded, moved by both)
        double Tc[16];
        if (globalRegistration(Tc) != 0) return -1;
        std::array<double, 16> M{};
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c)
                M[4 * r + c] = ((Tc[4 * r] * param_.initial_matrix_[c] + Tc[4 * r + 1] * param_.initial_matrix_[4 + c]) +
                                Tc[4 * r + 2] * param_.initial_matrix_[8 + c]) + Tc[4 * r + 3] * param_.initial_matrix_[12 + c];
        for (int i = 0; i < 16; ++i) trans[i] = M[i];
    }
    bool identity = true;
    for (int i = 0; i < 16; ++i) identity = identity && (trans[i] == ((i % 5 == 0) ? 1.0 : 0.0));
    const int method = param_.evaluation_method_;
    if (method == 2) {
        // RegistrationGeneralizedICP (:1378-1384): InitializePointCloudForGeneralizedICP(epsilon = 1e-3) on both clouds as
        // loaded (normals from the 20 nearest neighbours where a cloud has none); they rotate with the map from here on
        if (me_gicp_covariances(ctx_, ME_SLOT_EST, 1e-3, nullptr) != ME_OK || me_gicp_covariances(ctx_, ME_SLOT_GT, 1e-3, nullptr) != ME_OK)
            return fail(me_last_error(ctx_));
    }
    if (!identity && me_transform_cloud(ctx_, ME_SLOT_EST, trans.data()) != ME_OK) return fail(me_last_error(ctx_));
    me_icp_sums s;
    me_icp_lsq q;
    const int robust = method == 0 ? ME_ROBUST_L2 : param_.icp_robust_kernel;  // point-to-point takes no kernel (as upstream)
    auto evaluate = [&](me_ctx *c, double max_d, double &fit, double &rmse) -> bool {
        if (me_nn1(c, ME_SLOT_EST, ME_SLOT_GT, nullptr, nullptr) != ME_OK) return false;
        if (method == 0) {
            if (me_icp_p2p_sums(c, ME_SLOT_EST, max_d, &s) != ME_OK) return false;
        } else if (robust != ME_ROBUST_L2) {
            // TransformationEstimationPointToPlane(kernel) / ForGeneralizedICP(epsilon, kernel) [Open3D, upstream]
            me_icp_robust rq;
            if (me_icp_lsq_sums_robust(c, ME_SLOT_EST, method == 1 ? ME_ICP_POINT_TO_PLANE : ME_ICP_GENERALIZED, max_d, robust,
                                       param_.icp_robust_scale > 0 ? param_.icp_robust_scale : 1.0, &rq) != ME_OK)
                return false;
            for (int i = 0; i < 36; ++i) q.JTJ[i] = rq.JTJ[i];
            for (int i = 0; i < 6; ++i) q.JTr[i] = rq.JTr[i];
            q.n_corr = s.n_corr = rq.n_corr;
            q.n_source = s.n_source = rq.n_source;
            q.r2 = rq.r2;
            q.sum_d2 = s.sum_d2 = rq.sum_d2;
        } else {
            // TransformationEstimationPointToPlane (:1373-1377) needs normals on the target, as in Open3D
            if (me_icp_lsq_sums(c, ME_SLOT_EST, method == 1 ? ME_ICP_POINT_TO_PLANE : ME_ICP_GENERALIZED, max_d, &q) != ME_OK)
                return false;
            s.n_corr = q.n_corr;
            s.n_source = q.n_source;
            s.sum_d2 = q.sum_d2;
        }
        if (comm_ && reduceIcp(s, q, method) != 0) return false;
        fit = s.n_source ? (double) s.n_corr / (double) s.n_source : 0.0;
        rmse = s.n_corr ? std::sqrt(s.sum_d2 / (double) s.n_corr) : 0.0;
        return true;
    };
    double fit = 0, rmse = 0;
    // the loop of RegistrationICP on context c; `total` is multiplied by every update
    auto run_loop = [&](me_ctx *c, double max_d, int max_iteration, double *total) -> bool {
        if (!evaluate(c, max_d, fit, rmse)) return fail(me_last_error(c)), false;
        for (int it = 1; it <= max_iteration; ++it) {
            if (method == 0 ? s.n_corr < 3 : s.n_corr == 0) break;
            double upd[16];
            if (method == 0) kabsch_from_sums(s, upd);
            else lsq_update(q, upd);
            matmul4(upd, total, total);
            if (me_transform_cloud(c, ME_SLOT_EST, upd) != ME_OK) return fail(me_last_error(c)), false;
            const double pf = fit, pr = rmse;
            if (!evaluate(c, max_d, fit, rmse)) return fail(me_last_error(c)), false;
            if (std::fabs(pf - fit) < 1e-6 && std::fabs(pr - rmse) < 1e-6) break;
        }
        return true;
    };
    if (param_.icp_multi_scale_voxels.empty()) {
        if (!run_loop(ctx_, param_.icp_max_distance_, 30, trans.data())) return -1;
    } else {
        // icp_multi_scale_*: coarse to fine.  A level with a voxel > 0 runs on voxel down-samples of both resident clouds, as posed, in
        // a private context (the copies carry no attributes: method 1 estimates the target copy's normals from 20 neighbours, method 2
        // the covariances of both copies); its update then moves the resident map.  A level <= 0 runs on the resident clouds.
        for (size_t l = 0; l < param_.icp_multi_scale_voxels.size(); ++l) {
            const double v = param_.icp_multi_scale_voxels[l], max_d = param_.icp_multi_scale_distances[l];
            const int iters = param_.icp_multi_scale_iterations[l];
            if (!(v > 0)) {
                if (!run_loop(ctx_, max_d, iters, trans.data())) return -1;
                continue;
            }
            me_ctx *co = me_create(param_.gpu_device, 0);
            if (!co) return fail(std::string("icp_multi_scale_voxels: ") + me_last_error(nullptr));
            struct Destroy {
                me_ctx *c;
                ~Destroy() { me_destroy(c); }
            } d{co};
            int64_t n = 0;
            if (me_voxel_downsample_into(ctx_, ME_SLOT_EST, co, ME_SLOT_EST, v, &n) != ME_OK ||
                me_voxel_downsample_into(ctx_, ME_SLOT_GT, co, ME_SLOT_GT, v, &n) != ME_OK)
                return fail(std::string("icp_multi_scale_voxels: ") + me_last_error(co));
            if (method == 1 && me_estimate_normals(co, ME_SLOT_GT, 20, nullptr, nullptr, nullptr) != ME_OK)
                return fail(std::string("icp_multi_scale_voxels: ") + me_last_error(co));
            if (method == 2 && (me_gicp_covariances(co, ME_SLOT_EST, 1e-3, nullptr) != ME_OK ||
                                me_gicp_covariances(co, ME_SLOT_GT, 1e-3, nullptr) != ME_OK))
                return fail(std::string("icp_multi_scale_voxels: ") + me_last_error(co));
            double level[16];
            for (int i = 0; i < 16; ++i) level[i] = (i % 5 == 0) ? 1.0 : 0.0;
            if (!run_loop(co, max_d, iters, level)) return -1;
            matmul4(level, trans.data(), trans.data());
            if (me_transform_cloud(ctx_, ME_SLOT_EST, level) != ME_OK) return fail(me_last_error(ctx_));
        }
    }
    t3 = 0;  // no mesh stage
    t4 = tic_toc.toc();
    if (comm_ && me_set_shard(ctx_, 0, 1) != ME_OK) return fail(me_last_error(ctx_));
    if (me_download_cloud(ctx_, ME_SLOT_EST, map_3d_->points_.data()) != ME_OK)  // *map_3d_ = map_3d_->Transform(trans) (:1392)
        return fail(me_last_error(ctx_));
    if (root) {
        std::cout << "INFO: ICP registration time: " << t4 / 1000.0 << " [s]" << std::endl;
        std::cout << "INFO: Aligned transformation: \n";
        for (int r = 0; r < 4; ++r)
            std::cout << trans[4 * r] << " " << trans[4 * r + 1] << " " << trans[4 * r + 2] << " " << trans[4 * r + 3] << std::endl;
        std::cout << "INFO: ICP overlap ratio: " << fit << std::endl;
        std::cout << "INFO: ICP correspondences RMSE: " << rmse << std::endl;
        std::cout << "INFO: ICP correspondences size: " << s.n_corr << std::endl;
    }
    // "Aligned cloud:" / "Aligned results:" lines (map_eval.cpp:223-225)
    // (`file_result << matrix`: Eigen's default IOFormat pads every coefficient to the width of the widest one of the WHOLE
    //  matrix, one space between columns, one row per line)
    file_result << std::fixed << std::setprecision(5) << "Aligned cloud: " << eigen_matrix4(trans.data(), 5) << std::endl;
    file_result << std::fixed << std::setprecision(5) << "Aligned results: " << fit << " " << s.n_corr << std::endl;
    if (param_.icp_information_matrix && writeRegistrationInformation() != 0) return -1;
    if (metrics) calculateMetrics();
    t5 = tic_toc.toc();
    return last_error.empty() ? 0 : -1;
}

// registration_information.txt (icp_information_matrix: true; no reference counterpart): Open3D's GetInformationMatrixFromPointClouds
// [upstream] of the final alignment over the pairs inside icp_max_distance (me_icp_information).  Six rows of the matrix (%.17g), then
// "n_corr N", "eigenvalues e0 .. e5" ascending (the Jacobi decomposition of csrc/me_horn.hpp) and "ratio smallest/largest": a ratio
// near zero names a direction of the pose that the pair does not constrain (a corridor, a single plane).
int MapEval::writeRegistrationInformation() {
    double info[36], a[36], ev[6], V[36];
    int64_t n = 0;
    if (me_nn1(ctx_, ME_SLOT_EST, ME_SLOT_GT, nullptr, nullptr) != ME_OK ||
        me_icp_information(ctx_, ME_SLOT_EST, param_.icp_max_distance_, info, &n) != ME_OK)
        return fail(std::string("icp_information_matrix: ") + me_last_error(ctx_));
    for (int i = 0; i < 36; ++i) a[i] = info[i];
    me::jacobi_sym(6, a, ev, V);
    std::sort(ev, ev + 6);
    const double ratio = ev[5] != 0.0 ? ev[0] / ev[5] : 0.0;
    std::filesystem::create_directories(results_subfolder);
    const std::string path = results_subfolder + "registration_information.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail("cannot write " + path);
    for (int r = 0; r < 6; ++r)
        std::fprintf(f, "%.17g %.17g %.17g %.17g %.17g %.17g\n", info[6 * r], info[6 * r + 1], info[6 * r + 2], info[6 * r + 3],
                     info[6 * r + 4], info[6 * r + 5]);
    std::fprintf(f, "n_corr %lld\neigenvalues %.17g %.17g %.17g %.17g %.17g %.17g\nratio %.17g\n", (long long) n, ev[0], ev[1], ev[2], ev[3],
                 ev[4], ev[5], ratio);
    if (std::fclose(f) != 0) return fail("writing " + path + " failed");
    if (param_.dist_rank == 0)
        std::cout << "INFO: Information matrix eigenvalue ratio (smallest / largest): " << ratio << " over " << n << " correspondences"
                  << std::endl;
    return 0;
}

void MapEval::calculateMetrics() {
    // map_eval.cpp:1147-1202: statistics on ICP's final correspondence set (est -> gt, d2 < max^2), then
    // EvaluateRegistration(gt -> map, max) (:1168), cd_vec (:1171) and the full Chamfer distance (:1194).
    TicToc tt;
    me_nn_stats_out eg, ge;
    if (me_nn1(ctx_, ME_SLOT_EST, ME_SLOT_GT, nullptr, nullptr) != ME_OK ||
        me_nn_stats(ctx_, ME_SLOT_EST, param_.icp_max_distance_, ME_GATE_LT_SQUARED, param_.trunc_dist_.data(), &eg) != ME_OK) {
        fail(me_last_error(ctx_));
        return;
    }
    t_acc = tt.toc() / 1000.0;
    if (me_nn1(ctx_, ME_SLOT_GT, ME_SLOT_EST, nullptr, nullptr) != ME_OK ||
        me_nn_stats(ctx_, ME_SLOT_GT, param_.icp_max_distance_, ME_GATE_LT_SQUARED, param_.trunc_dist_.data(), &ge) != ME_OK) {
        fail(me_last_error(ctx_));
        return;
    }
    finishRegistrationMetrics(eg, ge, t_acc);
    t_fcd += tt.toc() / 1000.0 - t_acc;
}

// the tail of calculateMetrics (map_eval.cpp:1171-1201): result vectors, cd_vec, the full Chamfer distance
void MapEval::finishRegistrationMetrics(const me_nn_stats_out &eg, const me_nn_stats_out &ge, double t_acc_s) {
    t_acc = t_acc_s;
    push_results(est_gt_results, eg);
    push_results(gt_est_results, ge);
    for (int i = 0; i < 5; ++i) cd_vec[i] = est_gt_results[1][i] + gt_est_results[1][i];  // (:1171)
    TicToc t1_;
    full_chamfer_dist = eg.mean_nn_dist + ge.mean_nn_dist;  // computeChamferDistance (:1194, :1429): same two searches
    t_fcd = t1_.toc() / 1000.0;
    if (param_.evaluate_error_distribution && computeErrorDistribution(ME_GATE_LT_SQUARED) != 0) return;
    if (param_.dist_rank > 0) return;
    std::cout << "INFO: RMSE/AC: " << eigen_row(est_gt_results[1], 6) << std::endl;
    std::cout << "INFO: Fitness/Overlap: " << eigen_row(est_gt_results[2], 6) << std::endl;
    std::cout << "INFO: Full Chamfer distance: " << full_chamfer_dist << std::endl;
}

// open3d ColorToUint8 + the packed-float rgb column of open3d::io::WritePointCloud(.pcd)
static std::vector<float> pack_rgb(const std::vector<double> &rgb) {
    std::vector<float> out(rgb.size() / 3);
    for (size_t i = 0; i < out.size(); ++i) {
        uint32_t c[3];
        for (int k = 0; k < 3; ++k) c[k] = (uint32_t) std::round(std::min(1.0, std::max(0.0, rgb[3 * i + k])) * 255.0);
        const uint32_t packed = (c[0] << 16) | (c[1] << 8) | c[2];
        std::memcpy(&out[i], &packed, 4);
    }
    return out;
}

// ColorPointCloudByMME(cloud, entropies) (map_eval.cpp:686-735) from the entropies the last me_mme left on the device
bool MapEval::renderEntropy(int slot, std::vector<double> &xyz, std::vector<double> &rgb, bool want_points) {
    int64_t m = 0;
    if (me_render_entropy(ctx_, slot, nullptr, nullptr, 0, &m, &min_abs_entropy, &max_abs_entropy) != ME_OK) {
        fail(me_last_error(ctx_));
        return false;
    }
    xyz.clear();
    rgb.clear();
    if (m == 0) {
        // no point had enough neighbours (sparse cloud / small nn_radius): the entropy range is undefined (the reference
        // reads min/max of an empty set there).  Say so, and report NaN rather than the +-inf of an empty reduction.
        std::cerr << "WARNING: no valid entropy value (0 points with enough neighbours within nn_radius): MME range is undefined, "
                     "no entropy map is written" << std::endl;
        min_abs_entropy = max_abs_entropy = std::nan("");
        return true;
    }
    if (!want_points) return true;
    xyz.resize((size_t) m * 3);
    rgb.resize((size_t) m * 3);
    if (me_render_entropy(ctx_, slot, xyz.data(), rgb.data(), m, &m, &min_abs_entropy, &max_abs_entropy) != ME_OK) {
        fail(me_last_error(ctx_));
        return false;
    }
    return true;
}

// MapEval::process()'s metric phase (map_eval.cpp:52-85: computeMME :56, calculateMetricsWithInitialMatrix :76, calculateVMD :85)
// as ONE call into the library, made from this one thread (process() is single-threaded, :4): me_run_suite_from runs the stages
// on two lanes (its second lane is a thread inside the library, csrc/me_suite.hip).  The reference's member functions keep their
// roles below as CONSUMERS of what the call left on the device: entropies / colour maps, result vectors, the voxel files.
// (the clouds are std::vectors: pageable.  The library moves them through its own pinned staging buffers at the link's rate;
//  ME_SUITE_PIN_HOST_INPUT — page-locking the vectors in place for the call — is the alternative for callers short of host threads)
static const int kSuiteFlags = ME_SUITE_OVERLAP;
int MapEval::processOneCall(bool from_host, double t_loaded) {
    t1 = t_loaded;
    TicToc clock;
    me_suite_params sp{};
    sp.icp_max_distance = param_.icp_max_distance_;
    sp.gate_mode = ME_GATE_LE_UNSQUARED;  // d2 <= icp_max_distance (:1219, sic)
    for (int k = 0; k < 5; ++k) sp.trunc[k] = param_.trunc_dist_[k];
    sp.nn_radius = param_.nn_radius_;
    sp.vmd_voxel_size = param_.vmd_voxel_size_;
    sp.evaluate_mme = param_.evaluate_mme_ ? 1 : 0;
    sp.evaluate_gt_mme = param_.evaluate_gt_mme_ ? 1 : 0;
    sp.min_pts = 100;
    sp.scs_radius = 5;
    me_suite_out so;
    const double *T = param_.initial_matrix_.data();
    bool identity = true;
    for (int i = 0; i < 16; ++i) identity = identity && (T[i] == ((i % 5 == 0) ? 1.0 : 0.0));
    const int rc = from_host ? me_run_suite_from(ctx_, map_3d_->points_.data(), (int64_t) map_3d_->size(), gt_3d_->points_.data(),
                                                 (int64_t) gt_3d_->size(), T, &sp, kSuiteFlags, &so)
                             : me_run_suite_from(ctx_, nullptr, 0, nullptr, 0, T, &sp, ME_SUITE_OVERLAP, &so);
    if (rc != ME_OK) return fail(me_last_error(ctx_));
    const double suite_ms = clock.toc();
    std::cout << std::fixed << std::setprecision(3) << "INFO: metric phase, one me_run_suite_from call (two lanes): " << suite_ms
              << " ms for " << map_3d_->size() << " + " << gt_3d_->size() << " points [index " << so.stage_ms[0] << ", mme " << so.stage_ms[4]
              << " + " << so.stage_ms[5] << ", nn " << so.stage_ms[1] << " + " << so.stage_ms[2] << ", stats " << so.stage_ms[3]
              << ", awd/scs " << so.stage_ms[6] << "]" << std::endl;
    std::cout.unsetf(std::ios::floatfield);
    std::cout << std::setprecision(6);
    // ---- computeMME's members (:149-189) ----
    if (param_.evaluate_mme_) {
        mme_est = so.mme_est;
        mme_gt = so.mme_gt;
        if (param_.save_immediate_result_) {  // the per-point arrays are fetched only when something is written from them
            est_entropies.assign(map_3d_->size(), 0.0);
            valid_entropy_points.assign(map_3d_->size(), 0);
            if (me_mme_fetch(ctx_, ME_SLOT_EST, est_entropies.data(), valid_entropy_points.data()) != ME_OK) return fail(me_last_error(ctx_));
        }
        if (!renderEntropy(ME_SLOT_EST, map_entropy_xyz, map_entropy_rgb, param_.save_immediate_result_)) return -1;
        if (!identity && param_.save_immediate_result_) {
            // map_3d_entropy is built from the map AS LOADED (:179, before :1206): the colours above are those of the untransformed
            // map's entropies, the coordinates are taken from the host's copy, which is still untransformed here
            size_t k = 0;
            for (size_t i = 0; i < valid_entropy_points.size() && 3 * k + 2 < map_entropy_xyz.size(); ++i)
                if (valid_entropy_points[i]) {
                    for (int d = 0; d < 3; ++d) map_entropy_xyz[3 * k + d] = map_3d_->points_[3 * i + d];
                    ++k;
                }
        }
        const int64_t nv = so.mme_est_valid;
        if (param_.enable_debug)
            std::cout << "TBB MME Valid_points " << nv * 100.0 / (double) map_3d_->size() << "% " << nv << " " << map_3d_->size() << std::endl;
        if (nv * 100.0 / (double) map_3d_->size() < 0.6) std::cerr << "valid points is too small, please check the input point cloud" << std::endl;
        if (param_.evaluate_gt_mme_) {
            if (param_.save_immediate_result_) {
                gt_entropies.assign(gt_3d_->size(), 0.0);
                if (me_mme_fetch(ctx_, ME_SLOT_GT, gt_entropies.data(), nullptr) != ME_OK) return fail(me_last_error(ctx_));
            }
            if (!renderEntropy(ME_SLOT_GT, gt_entropy_xyz, gt_entropy_rgb, param_.save_immediate_result_)) return -1;
            std::cout << "MME EST-GT: " << mme_est << " " << mme_gt << std::endl;
        } else {
            std::cout << "MME EST: " << mme_est << std::endl;
        }
        if (param_.save_immediate_result_) saveMmeResults();
    }
    if (param_.evaluate_mpv && param_.save_immediate_result_) saveMpvResults();
    if (param_.segment_planes && param_.save_immediate_result_) savePlaneResults();
    if (param_.evaluate_mom && param_.save_immediate_result_) saveMomResults();
    t2 = t1 + so.stage_ms[0] + so.stage_ms[4] + so.stage_ms[5];
    // ---- calculateMetricsWithInitialMatrix's members (:1204-1260) ----
    if (param_.enable_debug) std::cout << "INFO: Using initial matrix without registration." << std::endl;
    if (!identity && me_download_cloud(ctx_, ME_SLOT_EST, map_3d_->points_.data()) != ME_OK)  // *map_3d_ = map_3d_->Transform(..) (:1206)
        return fail(me_last_error(ctx_));
    finishInitialMatrixMetrics(so.est_gt, so.gt_est, so.stage_ms[1] / 1000.0);
    t_fcd += so.stage_ms[2] / 1000.0;  // the gt -> est search is what the full Chamfer distance adds (:1194)
    t5 = t4 = t3 = t2 + so.stage_ms[1] + so.stage_ms[2] + so.stage_ms[3];
    // ---- calculateVMD (:240-390): the voxel tables are cached on the clouds, AWD / CDF / SCS are O(voxels) ----
    calculateVMD();
    if (!last_error.empty()) return -1;
    if (param_.evaluate_deformation && computeDeformation() != 0) return -1;
    if (param_.evaluate_voxel_distances && computeVoxelDistances() != 0) return -1;
    if (param_.evaluate_voxel_transport && computeVoxelTransport() != 0) return -1;
    if (param_.save_voxel_metrics) {
        saveVoxelMetrics(ME_GATE_LE_UNSQUARED);  // the gate of the statistics above (:1219)
        if (!last_error.empty()) return -1;
    }
    if (param_.enable_debug) std::cout << "INFO: VMD calculation completed." << std::endl;
    if (param_.save_immediate_result_) saveRegistrationResults();
    if (param_.enable_debug) std::cout << "INFO: Results saved successfully." << std::endl;
    return 0;
}

void MapEval::computeMME(PointCloud &cloud, PointCloud &gt) {
    // est: ComputeMeanMapEntropyUsingNormal[TBB] k >= 10 (map_eval.cpp:1675); gt: ComputeMeanMapEntropy k >= 5 (:1458)
    est_entropies.assign(cloud.size(), 0.0);
    valid_entropy_points.assign(cloud.size(), 0);
    double s = 0;
    int64_t nv = 0;
    if (me_mme(ctx_, ME_SLOT_EST, param_.nn_radius_, 10, est_entropies.data(), valid_entropy_points.data(), &s, &nv) != ME_OK) {
        fail(me_last_error(ctx_));
        return;
    }
    mme_est = nv > 0 ? s / (double) nv : 0.0;
    // map_3d_entropy = ColorPointCloudByMME(map_3d_, est_entropies) (:136, :179) — on the device, from the entropies it holds
    if (!renderEntropy(ME_SLOT_EST, map_entropy_xyz, map_entropy_rgb, param_.save_immediate_result_)) return;
    if (param_.enable_debug)
        std::cout << "TBB MME Valid_points " << nv * 100.0 / (double) cloud.size() << "% " << nv << " " << cloud.size() << std::endl;
    if (nv * 100.0 / (double) cloud.size() < 0.6) std::cerr << "valid points is too small, please check the input point cloud" << std::endl;
    if (param_.evaluate_gt_mme_) {
        gt_entropies.assign(gt.size(), 0.0);
        std::vector<uint8_t> &gv = gt_valid_entropy_points;
        gv.assign(gt.size(), 0);
        if (me_mme(ctx_, ME_SLOT_GT, param_.nn_radius_, 5, gt_entropies.data(), gv.data(), &s, &nv) != ME_OK) {
            fail(me_last_error(ctx_));
            return;
        }
        mme_gt = nv > 0 ? s / (double) nv : 0.0;
        // gt_3d_entropy = ColorPointCloudByMME(gt_3d_, gt_entropies) (:139, :181); like the reference, this call overwrites
        // min/max_abs_entropy with the GT range (they are members there, :698-699)
        if (!renderEntropy(ME_SLOT_GT, gt_entropy_xyz, gt_entropy_rgb, param_.save_immediate_result_)) return;
        std::cout << "MME EST-GT: " << mme_est << " " << mme_gt << std::endl;
    } else {
        std::cout << "MME EST: " << mme_est << std::endl;
    }
}

void MapEval::calculateMetricsWithInitialMatrix() {
    TicToc tt;
    me_nn_stats_out eg, ge;
    // est -> gt: keep (i, nn) iff d2 <= icp_max_distance (:1215-1223, squared vs un-squared, sic)
    if (me_nn1(ctx_, ME_SLOT_EST, ME_SLOT_GT, nullptr, nullptr) != ME_OK ||
        me_nn_stats(ctx_, ME_SLOT_EST, param_.icp_max_distance_, ME_GATE_LE_UNSQUARED, param_.trunc_dist_.data(), &eg) != ME_OK) {
        fail(me_last_error(ctx_));
        return;
    }
    t_acc = tt.toc() / 1000.0;
    // gt -> est (:1226-1236): the intended (gt_i, map_nn) pairing — the reference stores the pair swapped and then indexes
    // the wrong clouds (undefined behaviour when N_e != N_g); see DESIGN.md "deviations".
    if (me_nn1(ctx_, ME_SLOT_GT, ME_SLOT_EST, nullptr, nullptr) != ME_OK ||
        me_nn_stats(ctx_, ME_SLOT_GT, param_.icp_max_distance_, ME_GATE_LE_UNSQUARED, param_.trunc_dist_.data(), &ge) != ME_OK) {
        fail(me_last_error(ctx_));
        return;
    }
    const double t_both = tt.toc() / 1000.0;
    finishInitialMatrixMetrics(eg, ge, t_acc);
    t_fcd += t_both - t_acc;  // the gt -> est search is what the full Chamfer distance adds (:1194)
}

void MapEval::finishInitialMatrixMetrics(const me_nn_stats_out &eg, const me_nn_stats_out &ge, double t_acc_s) {
    TicToc tt;
    t_acc = t_acc_s;
    push_results(est_gt_results, eg);
    push_results(gt_est_results, ge);
    for (int i = 0; i < 5; ++i) {
        cd_vec[i] = est_gt_results[1][i] + gt_est_results[1][i];  // (:1245)
        const double overlap_ratio = est_gt_results[2][i], rmse = est_gt_results[1][i];
        f1_vec[i] = 2 * overlap_ratio * rmse / (overlap_ratio + rmse);  // (:1249, sic)
        const int num_intersection = (int) est_gt_results[4][i];
        const long long num_union = (long long) map_3d_->size() + (long long) gt_3d_->size() - num_intersection;
        iou_vec[i] = (double) num_intersection / (double) num_union;  // (:1250-1252)
    }
    // FULL CD: the reference never computes it on this path (stays 0.0); it is free here (same two searches).
    full_chamfer_dist = param_.strict_reference ? 0.0 : (eg.mean_nn_dist + ge.mean_nn_dist);  // (:1429)
    t_fcd = tt.toc() / 1000.0;
    if (param_.evaluate_error_distribution && computeErrorDistribution(ME_GATE_LE_UNSQUARED) != 0) return;
    if (param_.evaluate_surface_error && computeSurfaceError(ME_GATE_LE_UNSQUARED) != 0) return;
    if (param_.dist_rank > 0) return;
    std::cout << "INFO: Chamfer Distance: " << eigen_row(cd_vec, 6) << std::endl;
    std::cout << "INFO: F1 Score: " << eigen_row(f1_vec, 6) << std::endl;
    std::cout << "INFO: est-gt MME: " << mme_est << " " << mme_gt << std::endl;
    std::cout << "INFO: IoU: " << eigen_row(iou_vec, 6) << std::endl;
}

double MapEval::computeChamferDistance() {
    double cd = 0;
    if (me_chamfer(ctx_, &cd) != ME_OK) fail(me_last_error(ctx_));
    return cd;
}

void MapEval::calculateVMD(bool tables_ready, bool write_files) {
    TicToc ticToc;
    int64_t nv = 0;
    // buildVoxelMap(gt), buildVoxelMap(est), updateVoxelMap (:248-252); tables_ready: the merged tables of a multi-GPU run
    if (!tables_ready)
    if (me_voxel_gaussians(ctx_, ME_SLOT_GT, param_.vmd_voxel_size_, nullptr, nullptr, nullptr, nullptr, nullptr, &nv) != ME_OK ||
        me_voxel_gaussians(ctx_, ME_SLOT_EST, param_.vmd_voxel_size_, nullptr, nullptr, nullptr, nullptr, nullptr, &nv) != ME_OK) {
        fail(me_last_error(ctx_));
        return;
    }
    t_v = ticToc.toc();
    int64_t n_rows = 0, counts[3] = {0, 0, 0};
    if (me_awd_scs(ctx_, param_.vmd_voxel_size_, 100, 5, nullptr, nullptr, &n_rows, &vmd, &scs_overall, counts) != ME_OK) {
        fail(me_last_error(ctx_));
        return;
    }
    if (!write_files) return;  // (ranks > 0 of a multi-GPU run hold the same scalars and write nothing)
    std::cout << "Update active/old/new voxel num: " << counts[0] << " " << counts[1] << " " << counts[2] << std::endl;
    std::vector<double> rows((size_t) n_rows * 27), ws((size_t) n_rows);
    if (n_rows > 0) {
        int64_t cap = n_rows;
        if (me_awd_scs(ctx_, param_.vmd_voxel_size_, 100, 5, rows.data(), ws.data(), &cap, &vmd, &scs_overall, counts) != ME_OK) {
            fail(me_last_error(ctx_));
            return;
        }
    }
    t_vmd = ticToc.toc();
    // voxel_errors.txt: 27 columns, default ostream precision (:292-302); rows in ascending voxel-index order
    std::ofstream output_file(results_subfolder + "voxel_errors.txt");
    if (!output_file.is_open()) {
        std::cerr << "ERROR: Failed to open voxel error output file." << std::endl;
        return;
    }
    for (int64_t r = 0; r < n_rows; ++r) {
        const double *p = rows.data() + 27 * r;
        for (int c = 0; c < 27; ++c) {
            if (c == 10 || c == 11) output_file << (long long) p[c];
            else output_file << p[c];
            output_file << (c == 26 ? "" : " ");
        }
        output_file << std::endl;
    }
    output_file.close();
    std::cout << "INFO: Calculated VMD: " << vmd << std::endl;
    // voxel_wasserstein_cdf.txt (:330-341)
    std::ofstream cdf_file(results_subfolder + "voxel_wasserstein_cdf.txt");
    if (!cdf_file.is_open()) {
        std::cerr << "ERROR: Failed to open CDF output file." << std::endl;
        return;
    }
    for (size_t i = 0; i < ws.size(); ++i) cdf_file << ws[i] << " " << static_cast<double>(i + 1) / ws.size() << std::endl;
    cdf_file.close();
    t_cdf = ticToc.toc();
    t_scs = t_cdf;  // SCS ran inside me_awd_scs
    std::cout << "INFO: Spatial Consistency Score (SCS): " << scs_overall << std::endl;
}

// voxel_metrics.txt (save_voxel_metrics: true; no reference counterpart): the AC / COM / CD statistics of both search directions and
// the MME, broken down by the voxels of calculateVMD's lattice (getVoxelIndex, voxel_calculator.cpp:241-245) — me_voxel_metrics on
// both clouds, joined on the voxel key with the W of voxel_errors.txt.  One row per voxel of the union of both clouds' voxels,
// ascending (ix, iy, iz); 44 columns: ix iy iz n_est n_gt, the 17 sums of me_nn_partial est -> gt (n_corr n_inl[5] sum_d[5]
// sum_d2[5] sum_sqrt_all), the same gt -> est, n_H_est sum_H_est n_H_gt sum_H_gt w2 (nan where AWD defines no W).  A cloud with no
// point in a voxel has zeros there.  Doubles as %.17g: the file round-trips.
void MapEval::saveVoxelMetrics(int gate_mode) {
    const double vs = param_.vmd_voxel_size_;
    struct Side {
        std::vector<int32_t> keys;
        std::vector<me_nn_partial> nn;
        std::vector<double> sum_h;
        std::vector<int64_t> n_h;
    } side[2];
    for (int s = 0; s < 2; ++s) {
        int have = 0;
        int64_t v = 0;
        if (me_voxel_metrics(ctx_, s, vs, param_.icp_max_distance_, gate_mode, param_.trunc_dist_.data(), nullptr, nullptr, nullptr,
                             nullptr, &have, &v) != ME_OK) {
            fail(me_last_error(ctx_));
            return;
        }
        side[s].keys.resize((size_t) v * 3);
        side[s].nn.resize((size_t) v);
        side[s].sum_h.resize((size_t) v);
        side[s].n_h.resize((size_t) v);
        if (me_voxel_metrics(ctx_, s, vs, param_.icp_max_distance_, gate_mode, param_.trunc_dist_.data(), side[s].keys.data(),
                             side[s].nn.data(), side[s].sum_h.data(), side[s].n_h.data(), &have, &v) != ME_OK) {
            fail(me_last_error(ctx_));
            return;
        }
    }
    // W of the voxels AWD pairs (voxel_errors.txt: columns 0-2 = key * voxel size, column 9 = W), ascending key order
    int64_t n_rows = 0;
    double awd = 0, scs = 0;
    if (me_awd_scs(ctx_, vs, 100, 5, nullptr, nullptr, &n_rows, &awd, &scs, nullptr) != ME_OK) {
        fail(me_last_error(ctx_));
        return;
    }
    std::vector<double> rows((size_t) n_rows * 27);
    if (n_rows > 0 && me_awd_scs(ctx_, vs, 100, 5, rows.data(), nullptr, &n_rows, &awd, &scs, nullptr) != ME_OK) {
        fail(me_last_error(ctx_));
        return;
    }
    auto pack = [](long long x, long long y, long long z) {
        return ((x + (1LL << 20)) << 42) | ((y + (1LL << 20)) << 21) | (z + (1LL << 20));
    };
    std::vector<long long> wkey((size_t) n_rows);
    for (int64_t r = 0; r < n_rows; ++r) {
        const double *p = rows.data() + 27 * r;
        wkey[r] = pack(std::llrint(p[0] / vs), std::llrint(p[1] / vs), std::llrint(p[2] / vs));
    }
    std::ofstream out(results_subfolder + "voxel_metrics.txt");
    if (!out.is_open()) {
        fail("failed to open " + results_subfolder + "voxel_metrics.txt");
        return;
    }
    char buf[64];
    auto put_i = [&](long long v) { out << ' ' << v; };
    auto put_d = [&](double v) {
        std::snprintf(buf, sizeof buf, " %.17g", v);
        out << buf;
    };
    auto put_nn = [&](const me_nn_partial *q) {
        const me_nn_partial z{};
        if (!q) q = &z;
        put_i(q->n_corr);
        for (int k = 0; k < 5; ++k) put_i(q->n_inl[k]);
        for (int k = 0; k < 5; ++k) put_d(q->sum_d[k]);
        for (int k = 0; k < 5; ++k) put_d(q->sum_d2[k]);
        put_d(q->sum_sqrt_all);
    };
    size_t i[2] = {0, 0}, w = 0;
    const size_t n[2] = {side[0].nn.size(), side[1].nn.size()};
    while (i[0] < n[0] || i[1] < n[1]) {  // merge of the two ascending key lists
        long long k[2];
        for (int s = 0; s < 2; ++s)
            k[s] = i[s] < n[s] ? pack(side[s].keys[3 * i[s]], side[s].keys[3 * i[s] + 1], side[s].keys[3 * i[s] + 2]) : LLONG_MAX;
        const long long key = std::min(k[0], k[1]);
        const bool in[2] = {k[0] == key, k[1] == key};
        const int s0 = in[0] ? 0 : 1;
        out << side[s0].keys[3 * i[s0]] << ' ' << side[s0].keys[3 * i[s0] + 1] << ' ' << side[s0].keys[3 * i[s0] + 2];
        put_i(in[0] ? side[0].nn[i[0]].n_query : 0);
        put_i(in[1] ? side[1].nn[i[1]].n_query : 0);
        put_nn(in[0] ? &side[0].nn[i[0]] : nullptr);
        put_nn(in[1] ? &side[1].nn[i[1]] : nullptr);
        for (int s = 0; s < 2; ++s) {
            put_i(in[s] ? side[s].n_h[i[s]] : 0);
            put_d(in[s] ? side[s].sum_h[i[s]] : 0.0);
        }
        while (w < wkey.size() && wkey[w] < key) ++w;
        put_d(w < wkey.size() && wkey[w] == key ? rows[27 * w + 9] : std::nan(""));
        out << '\n';
        for (int s = 0; s < 2; ++s) i[s] += in[s] ? 1 : 0;
    }
    out.close();
    std::cout << "INFO: Saved per-voxel metrics to " << results_subfolder + "voxel_metrics.txt" << std::endl;
}

void MapEval::saveMmeResults() {
    if (!param_.evaluate_mme_) return;
    file_result << std::fixed << std::setprecision(5) << "MME: " << mme_est << " " << mme_gt << " " << min_abs_entropy << " "
                << max_abs_entropy << std::endl;  // (:395-396)
    // map_entropy.pcd / gt_entropy.pcd (:404, :412): valid points + Jet colour of the log-mapped entropy
    if (!map_entropy_xyz.empty()) {  // (nothing to draw when no point has a valid entropy; renderEntropy has said so)
        pcio::write_pcd(results_subfolder + "map_entropy.pcd", map_entropy_xyz.data(), map_entropy_xyz.size() / 3,
                        pack_rgb(map_entropy_rgb).data());
        std::cout << "INFO: Saved rendered entropy map to " << results_subfolder + "map_entropy.pcd" << std::endl;
    }
    if (param_.evaluate_gt_mme_ && !gt_entropy_xyz.empty()) {
        pcio::write_pcd(results_subfolder + "gt_entropy.pcd", gt_entropy_xyz.data(), gt_entropy_xyz.size() / 3,
                        pack_rgb(gt_entropy_rgb).data());
        std::cout << "INFO: Saved rendered entropy ground truth map to " << results_subfolder + "gt_entropy.pcd" << std::endl;
    }
    // (extra) the raw per-point entropies, so that nothing is lost to the colour map
    std::ofstream e(results_subfolder + "map_entropy.txt");
    for (size_t i = 0; i < est_entropies.size(); ++i) e << est_entropies[i] << " " << (int) valid_entropy_points[i] << "\n";
}

// the means of a me_local_geom_out: [0] MPV (mean l3), [1..4] linearity, planarity, sphericity, surface variation, [5] mean k; zeros
// when no point is valid (MME's convention)
static std::array<double, 6> local_geom_means(const me_local_geom_out &o) {
    std::array<double, 6> m{};
    if (o.n_valid > 0) {
        const double nv = (double) o.n_valid;
        m = {o.sum_l3 / nv, o.sum_linearity / nv, o.sum_planarity / nv, o.sum_sphericity / nv, o.sum_surface_variation / nv,
             (double) o.sum_k / nv};
    }
    return m;
}

int MapEval::computeMPV() {
    for (int s : {ME_SLOT_EST, ME_SLOT_GT}) {
        if (s == ME_SLOT_GT && !param_.evaluate_gt_mpv) break;
        if (me_local_geometry(ctx_, s, param_.mpv_radius, param_.mpv_min_points, &mpv_out[s]) != ME_OK)
            return fail(std::string("evaluate_mpv: ") + me_last_error(ctx_));
    }
    const auto e = local_geom_means(mpv_out[ME_SLOT_EST]), g = local_geom_means(mpv_out[ME_SLOT_GT]);
    if (param_.evaluate_gt_mpv) std::cout << "MPV EST-GT: " << e[0] << " " << g[0] << std::endl;
    else std::cout << "MPV EST: " << e[0] << std::endl;
    return 0;
}

void MapEval::saveMpvResults() {
    const bool gt = param_.evaluate_gt_mpv;
    const auto e = local_geom_means(mpv_out[ME_SLOT_EST]), g = local_geom_means(mpv_out[ME_SLOT_GT]);
    file_result << std::fixed << std::setprecision(5) << "MPV: " << e[0];
    if (gt) file_result << " " << g[0];
    file_result << std::endl;
    file_result << std::fixed << std::setprecision(5) << "LocalGeometry lin-plan-sph-sv: " << e[1] << " " << e[2] << " " << e[3] << " " << e[4];
    if (gt) file_result << " " << g[1] << " " << g[2] << " " << g[3] << " " << g[4];
    file_result << std::endl;
    // local_geometry.txt: radius and min_points, then per cloud n, n_valid, mean_k, MPV, linearity, planarity, sphericity, surface variation
    const std::string path = results_subfolder + "local_geometry.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    std::fprintf(f, "radius %.17g\nmin_points %d\n", param_.mpv_radius, param_.mpv_min_points);
    for (int s : {ME_SLOT_EST, ME_SLOT_GT}) {
        if (s == ME_SLOT_GT && !gt) break;
        const auto &m = s == ME_SLOT_EST ? e : g;
        std::fprintf(f, "%s %lld %lld %.17g %.17g %.17g %.17g %.17g %.17g\n", s == ME_SLOT_EST ? "est" : "gt", (long long) mpv_out[s].n,
                     (long long) mpv_out[s].n_valid, m[5], m[0], m[1], m[2], m[3], m[4]);
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

me_plane_params MapEval::planeParams(int max_planes) const {
    me_plane_params pp{};
    pp.distance_threshold = param_.plane_distance_threshold;
    pp.num_iterations = param_.plane_num_iterations;
    pp.max_planes = max_planes;
    pp.refit = param_.plane_refit ? 1 : 0;
    pp.min_inliers = param_.plane_min_inliers;
    pp.seed = param_.plane_seed;
    return pp;
}

// the count-weighted mean rms of a cloud's planes (0 without planes)
static double planes_mean_rms(const std::vector<me_plane_record> &r) {
    double num = 0.0, den = 0.0;
    for (const auto &p : r) {
        num += (double) p.count * p.rms;
        den += (double) p.count;
    }
    return den > 0 ? num / den : 0.0;
}

int MapEval::segmentPlanes() {
    const me_plane_params pp = planeParams(param_.plane_max_planes);
    for (int s : {ME_SLOT_EST, ME_SLOT_GT}) {
        if (s == ME_SLOT_GT && !param_.segment_gt_planes) break;
        plane_rec[s].assign((size_t) pp.max_planes, me_plane_record{});
        me_plane_info info{};
        if (me_segment_planes(ctx_, s, &pp, plane_rec[s].data(), nullptr, nullptr, &info) != ME_OK)
            return fail(std::string("segment_planes: ") + me_last_error(ctx_));
        plane_rec[s].resize((size_t) info.n_planes);
    }
    if (param_.segment_gt_planes)
        std::cout << "Planes EST-GT: " << plane_rec[ME_SLOT_EST].size() << " " << plane_rec[ME_SLOT_GT].size() << std::endl;
    else std::cout << "Planes EST: " << plane_rec[ME_SLOT_EST].size() << std::endl;
    return 0;
}

void MapEval::savePlaneResults() {
    const bool gt = param_.segment_gt_planes;
    // plane counts, then the count-weighted mean rms per cloud
    file_result << std::fixed << std::setprecision(5) << "Planes est-gt: " << plane_rec[ME_SLOT_EST].size();
    if (gt) file_result << " " << plane_rec[ME_SLOT_GT].size();
    file_result << " rms " << planes_mean_rms(plane_rec[ME_SLOT_EST]);
    if (gt) file_result << " " << planes_mean_rms(plane_rec[ME_SLOT_GT]);
    file_result << std::endl;
    // plane_segmentation.txt: the parameters ("name value"), then per cloud one row per plane:
    // cloud index count h a b c d rms mean_abs max_abs refit_degenerate
    const std::string path = results_subfolder + "plane_segmentation.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    std::fprintf(f, "distance_threshold %.17g\nnum_iterations %lld\nmax_planes %d\nmin_inliers %lld\nseed %llu\nrefit %s\n",
                 param_.plane_distance_threshold, (long long) param_.plane_num_iterations, param_.plane_max_planes,
                 (long long) param_.plane_min_inliers, (unsigned long long) param_.plane_seed, param_.plane_refit ? "true" : "false");
    for (int s : {ME_SLOT_EST, ME_SLOT_GT}) {
        if (s == ME_SLOT_GT && !gt) break;
        for (size_t i = 0; i < plane_rec[s].size(); ++i) {
            const me_plane_record &r = plane_rec[s][i];
            std::fprintf(f, "%s %zu %lld %lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d\n", s == ME_SLOT_EST ? "est" : "gt", i,
                         (long long) r.count, (long long) r.h, r.plane[0], r.plane[1], r.plane[2], r.plane[3], r.rms, r.mean_abs, r.max_abs,
                         (int) r.refit_degenerate);
        }
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

me_mom_params MapEval::momParams() const {
    me_mom_params mp{};
    mp.cos_parallel = std::cos(param_.mom_parallel_deg * (M_PI / 180.0));
    mp.cos_orthogonal = std::sin(param_.mom_orthogonal_deg * (M_PI / 180.0));  // cos(90 - deg)
    mp.min_axis_points = param_.mom_min_axis_points;
    return mp;
}

// me_mom per cloud; an input whose own stage (evaluate_mpv / segment_planes) did not run on that cloud is computed here, with the same
// keys, and leaves no line or file of its own
int MapEval::computeMOM() {
    const me_mom_params mp = momParams();
    for (int s : {ME_SLOT_EST, ME_SLOT_GT}) {
        if (s == ME_SLOT_GT && !param_.evaluate_gt_mom) break;
        const bool have_lg = param_.evaluate_mpv && (s == ME_SLOT_EST || param_.evaluate_gt_mpv);
        const bool have_planes = param_.segment_planes && (s == ME_SLOT_EST || param_.segment_gt_planes);
        if (!have_lg && me_local_geometry(ctx_, s, param_.mpv_radius, param_.mpv_min_points, nullptr) != ME_OK)
            return fail(std::string("evaluate_mom: ") + me_last_error(ctx_));
        if (!have_planes) {
            const me_plane_params pp = planeParams(param_.plane_max_planes);
            if (me_segment_planes(ctx_, s, &pp, nullptr, nullptr, nullptr, nullptr) != ME_OK)
                return fail(std::string("evaluate_mom: ") + me_last_error(ctx_));
        }
        if (me_mom(ctx_, s, &mp, &mom_out[s]) != ME_OK) return fail(std::string("evaluate_mom: ") + me_last_error(ctx_));
    }
    if (param_.evaluate_gt_mom) std::cout << "MOM EST-GT: " << mom_out[ME_SLOT_EST].mom_median << " " << mom_out[ME_SLOT_GT].mom_median << std::endl;
    else std::cout << "MOM EST: " << mom_out[ME_SLOT_EST].mom_median << std::endl;
    return 0;
}

void MapEval::saveMomResults() {
    const bool gt = param_.evaluate_gt_mom;
    // the sum of the axis medians per cloud, then the number of axes it was taken over
    file_result << std::fixed << std::setprecision(5) << "MOM est-gt: " << mom_out[ME_SLOT_EST].mom_median;
    if (gt) file_result << " " << mom_out[ME_SLOT_GT].mom_median;
    file_result << " n_axes " << mom_out[ME_SLOT_EST].n_axes;
    if (gt) file_result << " " << mom_out[ME_SLOT_GT].n_axes;
    file_result << std::endl;
    // mom.txt: the parameters ("name value"), then per cloud one row per axis:
    // cloud axis direction n_planes n_points n_valid rep_x rep_y rep_z sum_l3 min max lower upper median
    const std::string path = results_subfolder + "mom.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    std::fprintf(f, "parallel_deg %.17g\northogonal_deg %.17g\nmin_axis_points %lld\nradius %.17g\nmin_points %d\n", param_.mom_parallel_deg,
                 param_.mom_orthogonal_deg, (long long) param_.mom_min_axis_points, param_.mpv_radius, param_.mpv_min_points);
    for (int s : {ME_SLOT_EST, ME_SLOT_GT}) {
        if (s == ME_SLOT_GT && !gt) break;
        for (int k = 0; k < mom_out[s].n_axes; ++k) {
            const me_mom_axis &a = mom_out[s].axis[k];
            std::fprintf(f, "%s %d %d %d %lld %lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", s == ME_SLOT_EST ? "est" : "gt", k,
                         (int) a.direction, (int) a.n_planes, (long long) a.n_points, (long long) a.n_valid, a.rep[0], a.rep[1], a.rep[2], a.sum_l3,
                         a.min, a.max, a.lower, a.upper, a.median);
        }
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

// me_nn_error_distribution on the 1-NN results of both directions, which the metric path has just used for its statistics (the gate
// and gate mode are that path's when error_gated is set, none otherwise)
int MapEval::computeErrorDistribution(int gate_mode) {
    me_errdist_params &p = errdist_params;
    p = me_errdist_params{};
    p.gate = param_.error_gated ? param_.icp_max_distance_ : -1.0;
    p.gate_mode = gate_mode;
    p.n_quantiles = (int32_t) param_.error_quantiles.size();
    for (int j = 0; j < p.n_quantiles; ++j) p.prob[j] = param_.error_quantiles[(size_t) j];
    p.n_thresholds = (int32_t) param_.error_thresholds.size();
    for (int k = 0; k < p.n_thresholds; ++k) p.tau[k] = param_.error_thresholds[(size_t) k];
    p.n_bins = param_.error_cdf_bins;
    p.bin_width = p.n_bins > 0 ? param_.error_cdf_max / (double) p.n_bins : 0.0;
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s) {
        errdist_hist[s].assign((size_t) p.n_bins, 0);
        if (me_nn_error_distribution(ctx_, s, &p, &errdist_out[s], p.n_bins > 0 ? errdist_hist[s].data() : nullptr) != ME_OK)
            return fail(std::string("evaluate_error_distribution: ") + me_last_error(ctx_));
    }
    if (param_.dist_rank == 0)
        std::cout << "INFO: Hausdorff est-gt-sym: " << errdist_out[0].max_d << " " << errdist_out[1].max_d << " "
                  << std::max(errdist_out[0].max_d, errdist_out[1].max_d) << std::endl;
    return 0;
}

void MapEval::saveErrorDistribution() {
    const me_errdist_params &p = errdist_params;
    const me_errdist_out *o = errdist_out;
    file_result << std::fixed << std::setprecision(5) << "Hausdorff est-gt-sym: " << o[0].max_d << " " << o[1].max_d << " "
                << std::max(o[0].max_d, o[1].max_d) << std::endl;
    file_result << std::fixed << std::setprecision(5) << "Error quantiles est|gt:";
    for (int j = 0; j < p.n_quantiles; ++j) file_result << " " << p.prob[j];
    file_result << " |";
    for (int j = 0; j < p.n_quantiles; ++j) file_result << " " << o[0].quantile_d[j];
    file_result << " |";
    for (int j = 0; j < p.n_quantiles; ++j) file_result << " " << o[1].quantile_d[j];
    file_result << std::endl;
    file_result << std::fixed << std::setprecision(5) << "Fscore P-R-F @t:";
    for (int k = 0; k < p.n_thresholds; ++k) {
        double prf[3];
        me_fscore_finalize(o[0].n_within[k], o[0].n_used, o[1].n_within[k], o[1].n_used, prf);
        file_result << " " << p.tau[k] << " " << prf[0] << " " << prf[1] << " " << prf[2];
    }
    file_result << std::endl;
    // error_distribution.txt: the parameters ("name value ..."), then per direction the scalar row
    //   cloud n_query n_used sum_d sum_d2 min_d max_d argmax x y z
    // the quantile rows `cloud q prob rank quantile_d quantile_d2`, the threshold rows `cloud t tau n_within`, and the CDF rows
    // `cloud c edge count cumulative fraction`, closed by `cloud overflow n_overflow` (doubles as %.17g)
    const std::string path = results_subfolder + "error_distribution.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    std::fprintf(f, "gate %.17g\ngate_mode %d\nquantiles", p.gate, (int) p.gate_mode);
    for (int j = 0; j < p.n_quantiles; ++j) std::fprintf(f, " %.17g", p.prob[j]);
    std::fprintf(f, "\nthresholds");
    for (int k = 0; k < p.n_thresholds; ++k) std::fprintf(f, " %.17g", p.tau[k]);
    std::fprintf(f, "\ncdf_bins %d\ncdf_bin_width %.17g\n", (int) p.n_bins, p.bin_width);
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s) {
        const char *tag = s == ME_SLOT_EST ? "est" : "gt";
        const std::vector<double> &pts = (s == ME_SLOT_EST ? map_3d_ : gt_3d_)->points_;
        double xyz[3] = {0, 0, 0};
        if (o[s].argmax >= 0 && (size_t) o[s].argmax * 3 + 2 < pts.size())
            for (int d = 0; d < 3; ++d) xyz[d] = pts[(size_t) o[s].argmax * 3 + (size_t) d];
        std::fprintf(f, "%s %lld %lld %.17g %.17g %.17g %.17g %lld %.17g %.17g %.17g\n", tag, (long long) o[s].n_query, (long long) o[s].n_used,
                     o[s].sum_d, o[s].sum_d2, o[s].min_d, o[s].max_d, (long long) o[s].argmax, xyz[0], xyz[1], xyz[2]);
        for (int j = 0; j < p.n_quantiles; ++j)
            std::fprintf(f, "%s q %.17g %lld %.17g %.17g\n", tag, p.prob[j], (long long) o[s].rank[j], o[s].quantile_d[j], o[s].quantile_d2[j]);
        for (int k = 0; k < p.n_thresholds; ++k) std::fprintf(f, "%s t %.17g %lld\n", tag, p.tau[k], (long long) o[s].n_within[k]);
        long long cum = 0;
        for (int j = 0; j < p.n_bins; ++j) {
            cum += errdist_hist[s][(size_t) j];
            std::fprintf(f, "%s c %.17g %lld %lld %.17g\n", tag, (double) (j + 1) * p.bin_width, (long long) errdist_hist[s][(size_t) j], cum,
                         o[s].n_used > 0 ? (double) cum / (double) o[s].n_used : 0.0);
        }
        if (p.n_bins > 0) std::fprintf(f, "%s overflow %lld\n", tag, (long long) o[s].n_overflow);
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

// me_radius_normals on both clouds as loaded (the ground truth's file normals, if any, are replaced: this path's metrics use none)
int MapEval::computeSurfaceNormals() {
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s)
        if (me_radius_normals(ctx_, s, param_.normal_radius, param_.normal_min_points, nullptr, 0, &surface_normals[s]) != ME_OK)
            return fail(std::string("evaluate_surface_error: ") + me_last_error(ctx_));
    return 0;
}

// evaluate_m3c2: the map where initial_matrix puts it (me_transform_cloud; the host's copy stays as loaded), me_radius_normals on both
// clouds at m3c2_normal_radius (normal_min_points neighbours; the sign as Jacobi yields it), then me_m3c2 with each cloud as the query.
// Every m3c2_core_every-th point of a cloud, in the order of its slot, is a core point.
int MapEval::computeM3C2() {
    const double *T = param_.initial_matrix_.data();
    bool identity = true;
    for (int i = 0; i < 16; ++i) identity = identity && (T[i] == ((i % 5 == 0) ? 1.0 : 0.0));
    if (!identity && me_transform_cloud(ctx_, ME_SLOT_EST, T) != ME_OK) return fail(std::string("evaluate_m3c2: ") + me_last_error(ctx_));
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s)
        if (me_radius_normals(ctx_, s, param_.m3c2_normal_radius, param_.normal_min_points, nullptr, 0, &m3c2_normals[s]) != ME_OK)
            return fail(std::string("evaluate_m3c2: ") + me_last_error(ctx_));
    me_m3c2_params p{};
    p.projection_radius = param_.m3c2_projection_radius;
    p.max_depth = param_.m3c2_max_depth;
    p.reg_error = param_.m3c2_reg_error;
    p.min_points = param_.m3c2_min_points;
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s) {
        std::vector<uint8_t> mask;
        if (param_.m3c2_core_every > 1) {
            mask.assign((size_t) me_cloud_size(ctx_, s), 0);
            for (size_t i = 0; i < mask.size(); i += (size_t) param_.m3c2_core_every) mask[i] = 1;
        }
        if (me_m3c2(ctx_, s, &p, mask.empty() ? nullptr : mask.data(), &m3c2_out[s]) != ME_OK)
            return fail(std::string("evaluate_m3c2: ") + me_last_error(ctx_));
    }
    return 0;
}

void MapEval::saveM3C2() {
    const me_m3c2_out *o = m3c2_out;
    auto mean = [](double s, int64_t n) { return n > 0 ? s / (double) n : 0.0; };
    file_result << std::fixed << std::setprecision(5) << "M3C2 est-gt: " << mean(o[0].sum_dist, o[0].n_valid) << " "
                << mean(o[0].sum_abs_dist, o[0].n_valid) << " " << std::sqrt(mean(o[0].sum_dist2, o[0].n_valid)) << " "
                << mean((double) o[0].n_significant, o[0].n_valid) << std::endl;
    // m3c2.txt: the parameters ("name value"), then per direction (the query cloud's tag) the normals row `cloud normals n n_valid sum_k`,
    // the totals row
    //   cloud n_core n_no_normal n_valid n_significant sum_dist sum_abs_dist sum_dist2 sum_lod sum_n_own sum_n_other
    // and the worst point `cloud worst max_abs_dist argmax` (doubles as %.17g)
    const std::string path = results_subfolder + "m3c2.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    std::fprintf(f, "normal_radius %.17g\nnormal_min_points %d\nprojection_radius %.17g\nmax_depth %.17g\nmin_points %d\nreg_error %.17g\ncore_every %d\n",
                 param_.m3c2_normal_radius, param_.normal_min_points, param_.m3c2_projection_radius, param_.m3c2_max_depth, param_.m3c2_min_points,
                 param_.m3c2_reg_error, param_.m3c2_core_every);
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s) {
        const char *tag = s == ME_SLOT_EST ? "est" : "gt";
        const me_radius_normals_out &rn = m3c2_normals[s];
        std::fprintf(f, "%s normals %lld %lld %lld\n", tag, (long long) rn.n, (long long) rn.n_valid, (long long) rn.sum_k);
        std::fprintf(f, "%s %lld %lld %lld %lld %.17g %.17g %.17g %.17g %lld %lld\n", tag, (long long) o[s].n_core, (long long) o[s].n_no_normal,
                     (long long) o[s].n_valid, (long long) o[s].n_significant, o[s].sum_dist, o[s].sum_abs_dist, o[s].sum_dist2, o[s].sum_lod,
                     (long long) o[s].sum_n_own, (long long) o[s].sum_n_other);
        std::fprintf(f, "%s worst %.17g %lld\n", tag, o[s].max_abs_dist, (long long) o[s].argmax);
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

// evaluate_deformation: the per-voxel rigid deformation field of the map against the ground truth, from the resident 1-NN result with
// the map as the query (the one the statistics above were taken from), where the map stands now: me_voxel_deformation.
int MapEval::computeDeformation() {
    if (me_voxel_deformation(ctx_, ME_SLOT_EST, param_.deformation_voxel_size, param_.deformation_max_distance, param_.deformation_min_pairs,
                             param_.deformation_min_spread, &deform_out) != ME_OK)
        return fail(std::string("evaluate_deformation: ") + me_last_error(ctx_));
    return 0;
}

// The result line `Deformation mean-rms-max share_t-share_R:` (mean = sum n|t0| / sum n, rms = sqrt(sum n|t0|^2 / sum n), the largest |t0|
// of a fitted voxel, 1 - sum e_t / sum e0, 1 - sum e_R / sum e0_fit; nan on a zero denominator) and deformation_field.txt: the
// parameters ("name value"), then one row per voxel WITH pairs
//   ix iy iz n flags t0x t0y t0z ux uy uz angle e0 e_t e_R          (doubles as %.17g; angle = atan2(s, c) in radians,
// s = sqrt((R21 - R12)^2 + (R02 - R20)^2 + (R10 - R01)^2) / 2, c = (tr R - 1) / 2: Engine.deformation_field's formula)
void MapEval::saveDeformation() {
    const me_deform_summary &o = deform_out;
    const double nan = std::nan("");
    const double sn = (double) o.n_pairs;
    file_result << std::fixed << std::setprecision(15) << "Deformation mean-rms-max share_t-share_R: " << (o.n_pairs > 0 ? o.sum_n_t0 / sn : nan) << " "
                << (o.n_pairs > 0 ? std::sqrt(o.sum_n_t0sq / sn) : nan) << " " << o.max_t0 << " "
                << (o.sum_e0 != 0 ? 1.0 - o.sum_e_t / o.sum_e0 : nan) << " " << (o.sum_e0_fit != 0 ? 1.0 - o.sum_e_R / o.sum_e0_fit : nan) << std::endl;
    int64_t V = 0;
    if (me_voxel_deformation_fetch(ctx_, ME_SLOT_EST, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &V) != ME_OK) {
        fail(std::string("evaluate_deformation: ") + me_last_error(ctx_));
        return;
    }
    std::vector<int32_t> keys((size_t) V * 3);
    std::vector<int64_t> n((size_t) V);
    std::vector<uint8_t> flags((size_t) V);
    std::vector<double> t0((size_t) V * 3), u((size_t) V * 3), R((size_t) V * 9), e((size_t) V * 3);
    if (V > 0 && me_voxel_deformation_fetch(ctx_, ME_SLOT_EST, keys.data(), n.data(), flags.data(), nullptr, t0.data(), u.data(), R.data(), e.data(),
                                            &V) != ME_OK) {
        fail(std::string("evaluate_deformation: ") + me_last_error(ctx_));
        return;
    }
    const std::string path = results_subfolder + "deformation_field.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    std::fprintf(f, "voxel_size %.17g\nmax_distance %.17g\nmin_pairs %d\nmin_spread %.17g\n", param_.deformation_voxel_size,
                 param_.deformation_max_distance, param_.deformation_min_pairs, param_.deformation_min_spread);
    for (int64_t v = 0; v < V; ++v) {
        if (n[v] <= 0) continue;
        const double *r = &R[(size_t) v * 9];
        const double a = r[7] - r[5], b = r[2] - r[6], c = r[3] - r[1];
        const double angle = std::atan2(0.5 * std::sqrt(a * a + b * b + c * c), 0.5 * (r[0] + r[4] + r[8] - 1.0));
        std::fprintf(f, "%d %d %d %lld %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", keys[3 * v], keys[3 * v + 1], keys[3 * v + 2],
                     (long long) n[v], (int) flags[v], t0[3 * v], t0[3 * v + 1], t0[3 * v + 2], u[3 * v], u[3 * v + 1], u[3 * v + 2], angle,
                     e[3 * v], e[3 * v + 1], e[3 * v + 2]);
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

// evaluate_voxel_distances: per row of the AWD table (vmd_voxel_size, 100 points in both clouds, as calculateVMD) the point-set MMD at
// the bandwidths mmd_sigmas and the Gaussian closed forms, where both clouds stand now: me_voxel_distances.
int MapEval::computeVoxelDistances() {
    me_voxdist_params p;
    std::memset(&p, 0, sizeof(p));
    p.voxel_size = param_.vmd_voxel_size_;
    p.min_pts = 100;
    p.n_sigma = (int32_t) param_.mmd_sigmas.size();
    for (int b = 0; b < p.n_sigma; ++b) p.sigma[b] = param_.mmd_sigmas[(size_t) b];
    p.max_points = param_.mmd_max_points;
    p.eig_floor = param_.voxel_distance_eig_floor;
    int64_t V = 0;
    if (me_voxel_distances(ctx_, &p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &V, nullptr) != ME_OK)
        return fail(std::string("evaluate_voxel_distances: ") + me_last_error(ctx_));
    const size_t v = (size_t) V, ns = (size_t) p.n_sigma;
    voxdist_keys.assign(v * 3, 0);
    voxdist_pop.assign(v * 2, 0);
    voxdist_used.assign(v * 2, 0);
    voxdist_ksum.assign(v * ns * 3, 0.0);
    voxdist_mmd2.assign(v * ns * 2, 0.0);
    voxdist_gauss.assign(v * 4, 0.0);
    if (me_voxel_distances(ctx_, &p, voxdist_keys.data(), voxdist_pop.data(), voxdist_used.data(), voxdist_ksum.data(), voxdist_mmd2.data(),
                           voxdist_gauss.data(), &V, &voxdist_out) != ME_OK)
        return fail(std::string("evaluate_voxel_distances: ") + me_last_error(ctx_));
    return 0;
}

// The result lines `VoxelMMD @s1,s2,..:` (the bandwidths, then per bandwidth "mean_mmd mean_mmd2_u", the means over the rows) and `VoxelKL-BD-W2:` (the means of
// KL(est || gt), KL(gt || est), Bhattacharyya and W2), and voxel_distances.txt: the parameters ("name value"), then one row per voxel
//   ix iy iz n_est n_gt used_est used_gt kl_est_gt kl_gt_est bhattacharyya w2 { Sxx Syy Sxy mmd2_u mmd2_b } per bandwidth   (doubles as %.17g)
void MapEval::saveVoxelDistances() {
    const me_voxdist_out &o = voxdist_out;
    const size_t ns = param_.mmd_sigmas.size();
    file_result << std::fixed << std::setprecision(15) << "VoxelMMD @";
    for (size_t b = 0; b < ns; ++b) file_result << (b ? "," : "") << param_.mmd_sigmas[b];
    file_result << ":";
    for (size_t b = 0; b < ns; ++b) file_result << " " << o.mean_mmd[b] << " " << o.mean_mmd2_u[b];
    file_result << std::endl;
    file_result << std::fixed << std::setprecision(15) << "VoxelKL-BD-W2: " << o.mean_gauss[0] << " " << o.mean_gauss[1] << " " << o.mean_gauss[2] << " "
                << o.mean_gauss[3] << std::endl;
    const std::string path = results_subfolder + "voxel_distances.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    std::fprintf(f, "voxel_size %.17g\nmin_pts %d\nmax_points %lld\neig_floor %.17g\nn_sigma %d\n", param_.vmd_voxel_size_, 100, param_.mmd_max_points,
                 param_.voxel_distance_eig_floor, (int) ns);
    for (size_t b = 0; b < ns; ++b) std::fprintf(f, "sigma %.17g\n", param_.mmd_sigmas[b]);
    std::fprintf(f, "n_rows %lld\nn_rows_subsampled %lld\nn_pairs %lld\n", (long long) o.n_rows, (long long) o.n_rows_subsampled, (long long) o.n_pairs);
    for (size_t v = 0; v < (size_t) o.n_rows; ++v) {
        std::fprintf(f, "%d %d %d %d %d %d %d %.17g %.17g %.17g %.17g", voxdist_keys[3 * v], voxdist_keys[3 * v + 1], voxdist_keys[3 * v + 2],
                     voxdist_pop[2 * v], voxdist_pop[2 * v + 1], voxdist_used[2 * v], voxdist_used[2 * v + 1], voxdist_gauss[4 * v],
                     voxdist_gauss[4 * v + 1], voxdist_gauss[4 * v + 2], voxdist_gauss[4 * v + 3]);
        for (size_t b = 0; b < ns; ++b) {
            const double *k = &voxdist_ksum[(v * ns + b) * 3], *m = &voxdist_mmd2[(v * ns + b) * 2];
            std::fprintf(f, " %.17g %.17g %.17g %.17g %.17g", k[0], k[1], k[2], m[0], m[1]);
        }
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

// evaluate_voxel_transport: per row of the AWD table (vmd_voxel_size, 100 points in both clouds, as calculateVMD) the sliced 2-Wasserstein
// distance over transport_directions directions of a Fibonacci half sphere (z_k = (k + 0.5) / L, azimuth k times the golden angle,
// normalised twice) and the debiased Sinkhorn divergence on the schedule eps_0 = max(blur^2, 3 voxel_size^2), eps_{t+1} = max(blur^2,
// eps_t scaling^2) down to blur^2, then 128 further iterations at blur^2, where both clouds stand now: me_voxel_transport.
int MapEval::computeVoxelTransport() {
    const int L = param_.transport_directions;
    voxtrans_dirs.assign((size_t) L * 3, 0.0);
    for (int k = 0; k < L; ++k) {
        const double z = ((double) k + 0.5) / (double) L, rho = std::sqrt(1.0 - z * z), phi = (double) k * (M_PI * (3.0 - std::sqrt(5.0)));
        double d[3] = {rho * std::cos(phi), rho * std::sin(phi), z};
        for (int pass = 0; pass < 2; ++pass) {
            const double len = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            for (int c = 0; c < 3; ++c) d[c] /= len;
        }
        for (int c = 0; c < 3; ++c) voxtrans_dirs[(size_t) 3 * k + c] = d[c];
    }
    const double vs = param_.vmd_voxel_size_, b2 = param_.transport_blur * param_.transport_blur, s2 = param_.transport_scaling * param_.transport_scaling;
    voxtrans_eps.assign(1, std::max(b2, 3.0 * (vs * vs)));
    while (voxtrans_eps.back() > b2) voxtrans_eps.push_back(std::max(b2, voxtrans_eps.back() * s2));
    voxtrans_eps.insert(voxtrans_eps.end(), 128, b2);
    if (voxtrans_eps.size() > 512) return fail("evaluate_voxel_transport: the schedule has more than 512 iterations (raise transport_blur or lower transport_scaling)");
    me_voxtrans_params p;
    std::memset(&p, 0, sizeof(p));
    p.voxel_size = vs;
    p.min_pts = 100;
    p.n_dir = L;
    p.n_eps = (int32_t) voxtrans_eps.size();
    p.max_points = param_.transport_max_points;
    const double *dirs = L > 0 ? voxtrans_dirs.data() : nullptr;
    int64_t V = 0;
    if (me_voxel_transport(ctx_, &p, dirs, voxtrans_eps.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &V, nullptr) != ME_OK)
        return fail(std::string("evaluate_voxel_transport: ") + me_last_error(ctx_));
    const size_t v = (size_t) V;
    voxtrans_keys.assign(v * 3, 0);
    voxtrans_pop.assign(v * 2, 0);
    voxtrans_used.assign(v * 2, 0);
    voxtrans_sliced.assign(v * 4, std::nan(""));
    voxtrans_sinkhorn.assign(v * 6, 0.0);
    if (me_voxel_transport(ctx_, &p, dirs, voxtrans_eps.data(), voxtrans_keys.data(), voxtrans_pop.data(), voxtrans_used.data(), voxtrans_sliced.data(),
                           voxtrans_sinkhorn.data(), nullptr, nullptr, &V, &voxtrans_out) != ME_OK)
        return fail(std::string("evaluate_voxel_transport: ") + me_last_error(ctx_));
    return 0;
}

// The result lines `VoxelSW2 mean-max:` (the means over the rows of sw2 and of sqrt(max_sw2_sq)) and `VoxelSinkhorn @blur:` (the means of S,
// sqrt(max(0, S)) and marginal_err), and voxel_transport.txt: the parameters ("name value"), one "direction ux uy uz" line per direction, one
// "eps value" line per iteration, then one row per voxel
//   ix iy iz n_est n_gt used_est used_gt sw2_sq sw2 max_sw2_sq max_dir ot_xy ot_xx ot_yy S sinkhorn marginal_err   (doubles as %.17g)
void MapEval::saveVoxelTransport() {
    const me_voxtrans_out &o = voxtrans_out;
    file_result << std::fixed << std::setprecision(15) << "VoxelSW2 mean-max: " << o.mean_sw2 << " " << o.mean_max_sw2 << std::endl;
    file_result << std::fixed << std::setprecision(15) << "VoxelSinkhorn @" << param_.transport_blur << ": " << o.mean_s << " " << o.mean_sinkhorn << " "
                << o.mean_marginal_err << std::endl;
    const std::string path = results_subfolder + "voxel_transport.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    const size_t L = voxtrans_dirs.size() / 3;
    std::fprintf(f, "voxel_size %.17g\nmin_pts %d\nmax_points %lld\nblur %.17g\nscaling %.17g\nn_final %d\nn_dir %d\nn_eps %d\n", param_.vmd_voxel_size_, 100,
                 param_.transport_max_points, param_.transport_blur, param_.transport_scaling, 128, (int) L, (int) voxtrans_eps.size());
    for (size_t k = 0; k < L; ++k) std::fprintf(f, "direction %.17g %.17g %.17g\n", voxtrans_dirs[3 * k], voxtrans_dirs[3 * k + 1], voxtrans_dirs[3 * k + 2]);
    for (const double e : voxtrans_eps) std::fprintf(f, "eps %.17g\n", e);
    std::fprintf(f, "n_rows %lld\nn_rows_subsampled %lld\nn_pairs %lld\nmax_marginal_err %.17g\nmax_marginal_row %lld\n", (long long) o.n_rows,
                 (long long) o.n_rows_subsampled, (long long) o.n_pairs, o.max_marginal_err, (long long) o.max_marginal_row);
    for (size_t v = 0; v < (size_t) o.n_rows; ++v) {
        const double *s = &voxtrans_sliced[4 * v], *k = &voxtrans_sinkhorn[6 * v];
        std::fprintf(f, "%d %d %d %d %d %d %d %.17g %.17g %.17g %d %.17g %.17g %.17g %.17g %.17g %.17g\n", voxtrans_keys[3 * v], voxtrans_keys[3 * v + 1],
                     voxtrans_keys[3 * v + 2], voxtrans_pop[2 * v], voxtrans_pop[2 * v + 1], voxtrans_used[2 * v], voxtrans_used[2 * v + 1], s[0], s[1], s[2],
                     L > 0 ? (int) s[3] : -1, k[0], k[1], k[2], k[3], k[4], k[5]);
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

// evaluate_mesh_distance: the mesh of gt_mesh_path as it is in the file (like the ground-truth cloud it is not moved), the map where
// initial_matrix puts it (me_transform_cloud; the host's copy stays as loaded), me_mesh_distance with the map as the query, the exact
// nearest-rank quantiles of d over the matched points (error_quantiles; me_rank_select on the fetched values) and, with
// mesh_sample_points > 0, the mesh sampled into the ground-truth slot, me_nn1 both ways and their error distributions at the thresholds.
int MapEval::computeMeshDistance() {
    auto bad = [&](const std::string &m) { return fail("evaluate_mesh_distance: " + m); };
    std::vector<double> vx;
    std::vector<int32_t> tri;
    std::string err;
    if (param_.gt_mesh_path.empty() && param_.evaluate_mesh) {  // the ground truth's own reconstruction (computeReconstruction ran before)
        vx = recon_vertices[ME_SLOT_GT];
        tri = recon_triangles[ME_SLOT_GT];
        if (tri.empty()) return bad("the reconstruction of the ground truth has no triangle (mesh_voxel_size, mesh_min_points)");
    } else if (!pcio::read_ply_mesh(param_.gt_mesh_path, vx, tri, &err)) {
        return bad(err);
    }
    if (me_mesh_upload(ctx_, vx.data(), (int64_t) (vx.size() / 3), tri.data(), (int64_t) (tri.size() / 3), nullptr) != ME_OK ||
        me_mesh_info(ctx_, &mesh_info) != ME_OK)
        return bad(me_last_error(ctx_));
    const double *T = param_.initial_matrix_.data();
    bool identity = true;
    for (int i = 0; i < 16; ++i) identity = identity && (T[i] == ((i % 5 == 0) ? 1.0 : 0.0));
    if (!identity && me_transform_cloud(ctx_, ME_SLOT_EST, T) != ME_OK) return bad(me_last_error(ctx_));
    me_mesh_params p{};
    p.max_distance = param_.mesh_max_distance;
    p.n_thresholds = (int64_t) param_.mesh_thresholds.size();
    for (size_t k = 0; k < param_.mesh_thresholds.size(); ++k) p.thresholds[k] = param_.mesh_thresholds[k];
    if (me_mesh_distance(ctx_, ME_SLOT_EST, &p, &mesh_out) != ME_OK) return bad(me_last_error(ctx_));
    const size_t n = (size_t) mesh_out.n_query, nq = std::min<size_t>(param_.error_quantiles.size(), ME_RANK_MAX);
    mesh_rank.assign(nq, -1);
    mesh_quantile.assign(nq, 0.0);
    if (nq > 0 && mesh_out.n_matched > 0) {
        std::vector<double> d(n);
        std::vector<uint8_t> use(n);
        if (me_mesh_distance_fetch(ctx_, ME_SLOT_EST, d.data(), nullptr, nullptr, nullptr, nullptr) != ME_OK) return bad(me_last_error(ctx_));
        const double max2 = p.max_distance * p.max_distance;
        for (size_t i = 0; i < n; ++i) use[i] = d[i] <= max2, d[i] = std::sqrt(d[i]);
        const int64_t nm = mesh_out.n_matched;
        for (size_t j = 0; j < nq; ++j)  // nearest rank: ceil(q n) - 1, clamped
            mesh_rank[j] = std::min<int64_t>(nm - 1, std::max<int64_t>(0, (int64_t) std::ceil(param_.error_quantiles[j] * (double) nm) - 1));
        me_rank_stats rs{};
        if (me_rank_select(ctx_, d.data(), use.data(), (int64_t) n, mesh_rank.data(), (int32_t) nq, &rs) != ME_OK) return bad(me_last_error(ctx_));
        for (size_t j = 0; j < nq; ++j) mesh_quantile[j] = rs.value[j];
    }
    if (param_.mesh_signed) {  // the sign everywhere, over the result above and under the same gate
        me_mesh_sign_params sp{};
        sp.max_distance = param_.mesh_max_distance;
        if (me_mesh_topology(ctx_, &mesh_topo) != ME_OK || me_mesh_signed_distance(ctx_, ME_SLOT_EST, &sp, &mesh_sign) != ME_OK)
            return fail(std::string("mesh_signed: ") + me_last_error(ctx_));
    }
    if (param_.mesh_sample_points > 0) {
        if (me_mesh_sample(ctx_, ME_SLOT_GT, param_.mesh_sample_points, param_.mesh_seed) != ME_OK ||
            me_nn1(ctx_, ME_SLOT_EST, ME_SLOT_GT, nullptr, nullptr) != ME_OK || me_nn1(ctx_, ME_SLOT_GT, ME_SLOT_EST, nullptr, nullptr) != ME_OK)
            return bad(me_last_error(ctx_));
        me_errdist_params ep{};
        ep.gate = -1.0;
        ep.n_thresholds = (int32_t) param_.mesh_thresholds.size();
        for (int k = 0; k < ep.n_thresholds; ++k) ep.tau[k] = param_.mesh_thresholds[(size_t) k];
        for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s)
            if (me_nn_error_distribution(ctx_, s, &ep, &mesh_sampled[s], nullptr) != ME_OK) return bad(me_last_error(ctx_));
        for (int k = 0; k < ep.n_thresholds; ++k)
            me_fscore_finalize(mesh_sampled[0].n_within[k], mesh_sampled[0].n_used, mesh_sampled[1].n_within[k], mesh_sampled[1].n_used, mesh_prf[k]);
    }
    if (me_mesh_clear(ctx_) != ME_OK) return bad(me_last_error(ctx_));
    return 0;
}

// evaluate_observable: the ground-truth mesh (gt_mesh_path as it is in the file, or the ground truth's reconstruction), the positions of
// trajectory_path (every observable_pose_stride-th), the map where initial_matrix puts it; me_cloud_visibility of the ground truth
// (first_only), me_nn1 both ways and the ground truth's error distribution at the thresholds (all points); the visible points into a
// private context beside a copy of the moved map (me_outlier_select_into), the same there (observable points).
int MapEval::computeObservable() {
    auto bad = [&](const std::string &m) { return fail("evaluate_observable: " + m); };
    std::vector<double> vx, traj, org;
    std::vector<int32_t> tri;
    std::string err;
    if (param_.gt_mesh_path.empty()) {  // the ground truth's own reconstruction (computeReconstruction ran before)
        vx = recon_vertices[ME_SLOT_GT];
        tri = recon_triangles[ME_SLOT_GT];
        if (tri.empty()) return bad("the reconstruction of the ground truth has no triangle (mesh_voxel_size, mesh_min_points)");
    } else if (!pcio::read_ply_mesh(param_.gt_mesh_path, vx, tri, &err)) {
        return bad(err);
    }
    if (!tumio::read_tum_positions(param_.trajectory_path, traj, &err)) return bad(err);
    obs_poses_file = (int64_t) (traj.size() / 3);
    for (size_t i = 0; i < traj.size() / 3; i += (size_t) param_.observable_pose_stride) org.insert(org.end(), traj.begin() + 3 * i, traj.begin() + 3 * i + 3);
    obs_poses = (int64_t) (org.size() / 3);
    if (obs_poses > ME_VIS_MAX_ORIGINS)
        return bad("the trajectory holds " + std::to_string(obs_poses) + " poses after the stride, at most 65536 are cast (observable_pose_stride)");
    if (me_mesh_upload(ctx_, vx.data(), (int64_t) (vx.size() / 3), tri.data(), (int64_t) (tri.size() / 3), nullptr) != ME_OK)
        return bad(me_last_error(ctx_));
    const double *T = param_.initial_matrix_.data();
    bool identity = true;
    for (int i = 0; i < 16; ++i) identity = identity && (T[i] == ((i % 5 == 0) ? 1.0 : 0.0));
    if (!identity && me_transform_cloud(ctx_, ME_SLOT_EST, T) != ME_OK) return bad(me_last_error(ctx_));
    me_vis_params vp{};
    vp.min_range = 0.0, vp.max_range = param_.observable_max_range, vp.tolerance = param_.observable_tolerance, vp.first_only = 1;
    if (me_cloud_visibility(ctx_, ME_SLOT_GT, org.data(), obs_poses, &vp, &obs_vis) != ME_OK) return bad(me_last_error(ctx_));
    if (obs_vis.n_visible == 0) return bad("no ground-truth point is visible from the trajectory");
    me_errdist_params ep{};
    ep.gate = -1.0;
    ep.n_thresholds = (int32_t) param_.observable_thresholds.size();
    for (int k = 0; k < ep.n_thresholds; ++k) ep.tau[k] = param_.observable_thresholds[(size_t) k];
    if (me_nn1(ctx_, ME_SLOT_EST, ME_SLOT_GT, nullptr, nullptr) != ME_OK || me_nn1(ctx_, ME_SLOT_GT, ME_SLOT_EST, nullptr, nullptr) != ME_OK ||
        me_nn_error_distribution(ctx_, ME_SLOT_GT, &ep, &obs_gt[0], nullptr) != ME_OK)
        return bad(me_last_error(ctx_));
    std::vector<double> moved((size_t) me_cloud_size(ctx_, ME_SLOT_EST) * 3);
    if (me_download_cloud(ctx_, ME_SLOT_EST, moved.data()) != ME_OK) return bad(me_last_error(ctx_));
    me_ctx *priv = me_create(param_.gpu_device, 0);
    if (!priv) return bad(me_last_error(nullptr));
    int64_t kept = 0;
    const bool ok = me_outlier_select_into(ctx_, ME_SLOT_GT, priv, ME_SLOT_GT, &kept) == ME_OK &&
                    me_upload_cloud(priv, ME_SLOT_EST, moved.data(), (int64_t) (moved.size() / 3), nullptr, param_.nn_radius_) == ME_OK &&
                    me_nn1(priv, ME_SLOT_EST, ME_SLOT_GT, nullptr, nullptr) == ME_OK && me_nn1(priv, ME_SLOT_GT, ME_SLOT_EST, nullptr, nullptr) == ME_OK &&
                    me_nn_error_distribution(priv, ME_SLOT_GT, &ep, &obs_gt[1], nullptr) == ME_OK;
    const std::string perr = ok ? "" : me_last_error(priv);
    me_destroy(priv);
    if (!ok) return bad(perr);
    if (me_mesh_clear(ctx_) != ME_OK) return bad(me_last_error(ctx_));
    if (param_.dist_rank == 0)
        std::cout << "INFO: Observable ground truth: " << obs_vis.n_visible << " of " << obs_vis.n_points << " points from " << obs_poses << " poses"
                  << std::endl;
    return 0;
}

// `Observable visible-share COM@t: <share> then per threshold <t> <recall over all> <recall over the observable>`; observable.txt: the
// parameters and totals as "name value" lines, then one row per threshold: t, n_within and recall for all, the same for the observable
void MapEval::saveObservable() {
    const double share = obs_vis.n_points > 0 ? (double) obs_vis.n_visible / (double) obs_vis.n_points : 0.0;
    auto recall = [](const me_errdist_out &o, size_t k) { return o.n_used > 0 ? (double) o.n_within[k] / (double) o.n_used : 0.0; };
    file_result << std::fixed << std::setprecision(5) << "Observable visible-share COM@t: " << share;
    for (size_t k = 0; k < param_.observable_thresholds.size(); ++k)
        file_result << " " << param_.observable_thresholds[k] << " " << recall(obs_gt[0], k) << " " << recall(obs_gt[1], k);
    file_result << std::endl;
    const std::string path = results_subfolder + "observable.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    std::fprintf(f, "trajectory_path %s\nposes_in_file %lld\npose_stride %d\nposes_used %lld\n", param_.trajectory_path.c_str(),
                 (long long) obs_poses_file, param_.observable_pose_stride, (long long) obs_poses);
    std::fprintf(f, "max_range %.17g\ntolerance %.17g\n", param_.observable_max_range, param_.observable_tolerance);
    std::fprintf(f, "n_points %lld\nn_visible %lld\nn_in_range %lld\nn_tests %lld\nvisible_share %.17g\n", (long long) obs_vis.n_points,
                 (long long) obs_vis.n_visible, (long long) obs_vis.n_in_range, (long long) obs_vis.n_tests, share);
    std::fprintf(f, "n_used_all %lld\nn_used_observable %lld\n", (long long) obs_gt[0].n_used, (long long) obs_gt[1].n_used);
    std::fprintf(f, "# threshold n_within_all recall_all n_within_observable recall_observable\n");
    for (size_t k = 0; k < param_.observable_thresholds.size(); ++k)
        std::fprintf(f, "%.17g %lld %.17g %lld %.17g\n", param_.observable_thresholds[k], (long long) obs_gt[0].n_within[k], recall(obs_gt[0], k),
                     (long long) obs_gt[1].n_within[k], recall(obs_gt[1], k));
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

// evaluate_mesh: on each cloud as loaded, me_radius_normals at mesh_normal_radius (normal_min_points neighbours) turned towards
// mesh_viewpoint, or towards the centre of the cloud's bounding box, then me_reconstruct; the meshes are kept on the host for the writers
// and for computeMeshDistance.  With mesh_orient: propagate the radius normals are left unoriented (no viewpoint) and me_orient_normals
// (mesh_orient_k neighbours, direction +z, mesh_orient_inward) gives them one sign per component of the k-NN graph before me_reconstruct.
int MapEval::computeReconstruction() {
    auto bad = [&](const std::string &m) { return fail("evaluate_mesh: " + m); };
    me_recon_params rp{};
    rp.voxel = param_.mesh_voxel_size;
    rp.radius = param_.mesh_radius;
    rp.min_k = (int32_t) param_.mesh_min_points;
    rp.band = (int32_t) param_.mesh_band;
    const bool propagate = param_.mesh_orient == "propagate";
    me_orient_params op{};
    op.direction[2] = 1.0;
    op.k = (int32_t) param_.mesh_orient_k;
    op.inward = param_.mesh_orient_inward ? 1 : 0;
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s) {
        const std::vector<double> &pts = s == ME_SLOT_EST ? map_3d_->points_ : gt_3d_->points_;
        double *vp = recon_viewpoint[s];
        if (propagate) {  // unoriented radius normals, one sign carried over the k-NN graph from the top point of every component
            if (me_radius_normals(ctx_, s, param_.mesh_normal_radius, param_.normal_min_points, nullptr, 0, &recon_normals[s]) != ME_OK ||
                me_orient_normals(ctx_, s, &op, &recon_orient[s]) != ME_OK || me_reconstruct(ctx_, s, &rp, &recon_out[s]) != ME_OK)
                return bad(me_last_error(ctx_));
            recon_vertices[s].assign((size_t) recon_out[s].n_vertices * 3, 0.0);
            recon_triangles[s].assign((size_t) recon_out[s].n_triangles * 3, 0);
            if (me_reconstruct_fetch(ctx_, recon_vertices[s].data(), nullptr, recon_triangles[s].data()) != ME_OK) return bad(me_last_error(ctx_));
            continue;
        }
        if (param_.mesh_viewpoint.size() == 3) {
            for (int d = 0; d < 3; ++d) vp[d] = param_.mesh_viewpoint[(size_t) d];
        } else {
            double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (size_t i = 0; i + 2 < pts.size(); i += 3)
                for (int d = 0; d < 3; ++d) lo[d] = std::fmin(lo[d], pts[i + d]), hi[d] = std::fmax(hi[d], pts[i + d]);
            for (int d = 0; d < 3; ++d) vp[d] = pts.empty() ? 0.0 : 0.5 * (lo[d] + hi[d]);
        }
        if (me_radius_normals(ctx_, s, param_.mesh_normal_radius, param_.normal_min_points, vp, 0, &recon_normals[s]) != ME_OK ||
            me_reconstruct(ctx_, s, &rp, &recon_out[s]) != ME_OK)
            return bad(me_last_error(ctx_));
        recon_vertices[s].assign((size_t) recon_out[s].n_vertices * 3, 0.0);
        recon_triangles[s].assign((size_t) recon_out[s].n_triangles * 3, 0);
        if (me_reconstruct_fetch(ctx_, recon_vertices[s].data(), nullptr, recon_triangles[s].data()) != ME_OK) return bad(me_last_error(ctx_));
    }
    return 0;
}

// gt_mesh.ply / est_mesh.ply (the reference's names, map_eval.cpp:509-523) and reconstruction.txt: the parameters ("name value"), then per
// cloud ("<est|gt> name value ...") the viewpoint, the normals' counts and the counts of me_recon_out.  With mesh_orient: propagate the
// parameters gain three "orient..." lines and the viewpoint line of each cloud becomes "Orientation <est|gt>: " + the 8 integers of me_orient_out.
void MapEval::saveReconstruction() {
    std::string err;
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s) {
        const std::string path = results_subfolder + (s == ME_SLOT_EST ? "est_mesh.ply" : "gt_mesh.ply");
        if (!pcio::write_ply_mesh(path, recon_vertices[s], recon_triangles[s], &err)) fail("evaluate_mesh: " + err);
    }
    const std::string path = results_subfolder + "reconstruction.txt";
    std::FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot open " + path);
        return;
    }
    std::fprintf(f, "voxel %.17g\nradius %.17g\nmin_points %d\nband %d\nnormal_radius %.17g\nnormal_min_points %d\n", param_.mesh_voxel_size,
                 param_.mesh_radius, param_.mesh_min_points, param_.mesh_band, param_.mesh_normal_radius, param_.normal_min_points);
    if (param_.mesh_orient == "propagate") std::fprintf(f, "orient propagate\norient_k %d\norient_inward %d\n", param_.mesh_orient_k, param_.mesh_orient_inward ? 1 : 0);
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s) {
        const char *tag = s == ME_SLOT_EST ? "est" : "gt";
        const me_recon_out &o = recon_out[s];
        if (param_.mesh_orient == "propagate") {  // in place of the viewpoint: the integers of me_orient_out, in the struct's order
            const me_orient_out &r = recon_orient[s];
            std::fprintf(f, "Orientation %s: %lld %lld %lld %lld %lld %lld %lld %lld\n", tag, (long long) r.n, (long long) r.n_valid,
                         (long long) r.n_components, (long long) r.largest_component, (long long) r.n_tree_edges, (long long) r.n_graph_edges,
                         (long long) r.n_flipped, (long long) r.n_inconsistent_edges);
        } else
            std::fprintf(f, "%s viewpoint %.17g %.17g %.17g\n", tag, recon_viewpoint[s][0], recon_viewpoint[s][1], recon_viewpoint[s][2]);
        std::fprintf(f, "%s normals %lld %lld %lld\n", tag, (long long) recon_normals[s].n, (long long) recon_normals[s].n_valid,
                     (long long) recon_normals[s].sum_k);
        std::fprintf(f, "%s n_occupied_cells %lld\n%s n_active_cells %lld\n%s n_nodes %lld\n%s n_valid_nodes %lld\n%s n_cells_extracted %lld\n", tag,
                     (long long) o.n_occupied_cells, tag, (long long) o.n_active_cells, tag, (long long) o.n_nodes, tag, (long long) o.n_valid_nodes,
                     tag, (long long) o.n_cells_extracted);
        std::fprintf(f, "%s n_vertices %lld\n%s n_triangles %lld\n%s n_degenerate %lld\n%s sum_k %lld\n", tag, (long long) o.n_vertices, tag,
                     (long long) o.n_triangles, tag, (long long) o.n_degenerate, tag, (long long) o.sum_k);
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

void MapEval::saveMeshDistance() {
    const me_mesh_out &o = mesh_out;
    const double nm = (double) o.n_matched;
    file_result << std::fixed << std::setprecision(5) << "MeshError mean-rmse-max: " << (o.n_matched > 0 ? o.sum_d / nm : 0.0) << " "
                << (o.n_matched > 0 ? std::sqrt(o.sum_d2 / nm) : 0.0) << " " << o.max_d << std::endl;
    file_result << std::fixed << std::setprecision(5) << "MeshAC @t:";  // per threshold: the share of the matched points within it
    for (size_t k = 0; k < param_.mesh_thresholds.size(); ++k)
        file_result << " " << param_.mesh_thresholds[k] << " " << (o.n_matched > 0 ? (double) o.n_within[k] / nm : 0.0);
    file_result << std::endl;
    const me_mesh_sign_out &sg = mesh_sign;
    if (param_.mesh_signed) {  // over the signed points: mean, mean |.|, inside share; over the matched ones: the unreliable share
        const double ns = (double) sg.n_signed, nsm = (double) sg.n_matched;
        file_result << std::fixed << std::setprecision(5) << "MeshSigned mean-meanabs-inside-unreliable: "
                    << (sg.n_signed > 0 ? sg.sum_signed / ns : 0.0) << " " << (sg.n_signed > 0 ? sg.sum_abs_signed / ns : 0.0) << " "
                    << (sg.n_signed > 0 ? (double) sg.n_inside / ns : 0.0) << " " << (sg.n_matched > 0 ? (double) sg.n_unreliable / nsm : 0.0)
                    << std::endl;
    }
    // mesh_distance.txt: the info block ("name value ..."), the parameters, the totals row
    //   totals n_query n_matched n_face sum_d sum_d2 max_d argmax
    // the signed bias over the face region `signed sum_signed sum_abs_signed mean mean_abs`, the rows `t threshold n_within`,
    // `q prob rank d`, and with mesh_sample_points the rows `sampled <est|gt> n_query n_used sum_d sum_d2 max_d` and
    // `f threshold precision recall fscore` (doubles as %.17g)
    const std::string path = results_subfolder + "mesh_distance.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    const me_mesh_info_out &mi = mesh_info;
    std::fprintf(f, "vertices %lld\ntriangles %lld\ndegenerate %lld\ndepth %lld\narea %.17g\nbbox %.17g %.17g %.17g %.17g %.17g %.17g\n",
                 (long long) mi.n_vertices, (long long) mi.n_triangles, (long long) mi.n_degenerate, (long long) mi.depth, mi.area, mi.bbox_lo[0],
                 mi.bbox_lo[1], mi.bbox_lo[2], mi.bbox_hi[0], mi.bbox_hi[1], mi.bbox_hi[2]);
    std::fprintf(f, "max_distance %.17g\nsample_points %lld\nseed %llu\n", param_.mesh_max_distance, (long long) param_.mesh_sample_points,
                 (unsigned long long) param_.mesh_seed);
    std::fprintf(f, "totals %lld %lld %lld %.17g %.17g %.17g %lld\n", (long long) o.n_query, (long long) o.n_matched, (long long) o.n_face, o.sum_d,
                 o.sum_d2, o.max_d, (long long) o.argmax);
    std::fprintf(f, "signed %.17g %.17g %.17g %.17g\n", o.sum_signed, o.sum_abs_signed, o.n_face > 0 ? o.sum_signed / (double) o.n_face : 0.0,
                 o.n_face > 0 ? o.sum_abs_signed / (double) o.n_face : 0.0);
    for (size_t k = 0; k < param_.mesh_thresholds.size(); ++k)
        std::fprintf(f, "t %.17g %lld\n", param_.mesh_thresholds[k], (long long) o.n_within[k]);
    for (size_t j = 0; j < mesh_rank.size(); ++j)
        std::fprintf(f, "q %.17g %lld %.17g\n", param_.error_quantiles[j], (long long) mesh_rank[j], mesh_quantile[j]);
    if (param_.mesh_sample_points > 0) {
        for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s)
            std::fprintf(f, "sampled %s %lld %lld %.17g %.17g %.17g\n", s == ME_SLOT_EST ? "est" : "gt", (long long) mesh_sampled[s].n_query,
                         (long long) mesh_sampled[s].n_used, mesh_sampled[s].sum_d, mesh_sampled[s].sum_d2, mesh_sampled[s].max_d);
        for (size_t k = 0; k < param_.mesh_thresholds.size(); ++k)
            std::fprintf(f, "f %.17g %.17g %.17g %.17g\n", param_.mesh_thresholds[k], mesh_prf[k][0], mesh_prf[k][1], mesh_prf[k][2]);
    }
    if (param_.mesh_signed) {
        // with mesh_signed the topology block `topology <name> <count>` (me_mesh_topo_out's members in order) and the signed block:
        //   sign counts n_matched n_signed n_inside n_outside n_on n_unsigned n_unreliable
        //   sign regions n_face n_edge n_vertex
        //   sign sums sum_signed sum_abs_signed sum_signed2
        //   sign extremes min_signed argmin max_signed argmax
        const me_mesh_topo_out &tp = mesh_topo;
        std::fprintf(f, "topology n_edges %lld\ntopology n_boundary_edges %lld\ntopology n_nonmanifold_edges %lld\n"
                        "topology n_inconsistent_edges %lld\ntopology n_zero_edges %lld\ntopology n_zero_vertices %lld\n"
                        "topology n_tainted_vertices %lld\ntopology n_unreferenced_vertices %lld\ntopology closed %lld\n"
                        "topology oriented_manifold %lld\n",
                     (long long) tp.n_edges, (long long) tp.n_boundary_edges, (long long) tp.n_nonmanifold_edges,
                     (long long) tp.n_inconsistent_edges, (long long) tp.n_zero_edges, (long long) tp.n_zero_vertices,
                     (long long) tp.n_tainted_vertices, (long long) tp.n_unreferenced_vertices, (long long) tp.closed,
                     (long long) tp.oriented_manifold);
        std::fprintf(f, "sign counts %lld %lld %lld %lld %lld %lld %lld\n", (long long) sg.n_matched, (long long) sg.n_signed,
                     (long long) sg.n_inside, (long long) sg.n_outside, (long long) sg.n_on, (long long) sg.n_unsigned, (long long) sg.n_unreliable);
        std::fprintf(f, "sign regions %lld %lld %lld\n", (long long) sg.n_by_region[0], (long long) sg.n_by_region[1], (long long) sg.n_by_region[2]);
        std::fprintf(f, "sign sums %.17g %.17g %.17g\n", sg.sum_signed, sg.sum_abs_signed, sg.sum_signed2);
        std::fprintf(f, "sign extremes %.17g %lld %.17g %lld\n", sg.min_signed, (long long) sg.argmin, sg.max_signed, (long long) sg.argmax);
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

// me_nn_surface_error on the 1-NN results of both directions, after the metric path's statistics (the gate is that path's when
// surface_gated is set, none otherwise); the cosines of the angle thresholds are taken here, with the C library's cos
int MapEval::computeSurfaceError(int gate_mode) {
    me_surface_params &p = surface_params;
    p = me_surface_params{};
    p.gate = param_.surface_gated ? param_.icp_max_distance_ : -1.0;
    p.gate_mode = gate_mode;
    p.n_thresholds = (int32_t) param_.surface_thresholds.size();
    for (int k = 0; k < p.n_thresholds; ++k) p.tau[k] = param_.surface_thresholds[(size_t) k];
    p.n_angles = (int32_t) param_.surface_angles_deg.size();
    for (int k = 0; k < p.n_angles; ++k) p.cos_min[k] = std::cos(param_.surface_angles_deg[(size_t) k] * (M_PI / 180.0));
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s)
        if (me_nn_surface_error(ctx_, s, &p, &surface_out[s]) != ME_OK) return fail(std::string("evaluate_surface_error: ") + me_last_error(ctx_));
    return 0;
}

void MapEval::saveSurfaceError() {
    const me_surface_params &p = surface_params;
    const me_surface_out *o = surface_out;
    auto mean = [](double s, int64_t n) { return n > 0 ? s / (double) n : 0.0; };
    const double me[2] = {mean(o[0].sum_e, o[0].n_used), mean(o[1].sum_e, o[1].n_used)};
    file_result << std::fixed << std::setprecision(5) << "PlaneError est-gt-chamfer: " << me[0] << " " << me[1] << " " << me[0] + me[1] << std::endl;
    file_result << std::fixed << std::setprecision(5) << "PlaneAC @t:";
    for (int k = 0; k < p.n_thresholds; ++k)
        file_result << " " << p.tau[k] << " " << (o[0].n_within[k] > 0 ? std::sqrt(o[0].sum_e2_within[k] / (double) o[0].n_within[k]) : 0.0);
    file_result << std::endl;
    file_result << std::fixed << std::setprecision(5) << "NormalConsistency est-gt: " << mean(o[0].sum_c, o[0].n_normal_used) << " "
                << mean(o[1].sum_c, o[1].n_normal_used) << std::endl;
    // surface_error.txt: the parameters ("name value ..."), then per direction the normals row `cloud normals n n_valid sum_k` (of
    // that cloud's own me_radius_normals), the scalar row
    //   cloud n_query n_used n_normal_used sum_e sum_e2 sum_t2 sum_c max_e argmax
    // the rows `cloud t tau n_within sum_e2_within` and `cloud a angle_deg cos_min n_angle` (doubles as %.17g)
    const std::string path = results_subfolder + "surface_error.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) {
        fail("cannot write " + path);
        return;
    }
    std::fprintf(f, "normal_radius %.17g\nnormal_min_points %d\ngate %.17g\ngate_mode %d\nthresholds", param_.normal_radius,
                 param_.normal_min_points, p.gate, (int) p.gate_mode);
    for (int k = 0; k < p.n_thresholds; ++k) std::fprintf(f, " %.17g", p.tau[k]);
    std::fprintf(f, "\nangles_deg");
    for (int k = 0; k < p.n_angles; ++k) std::fprintf(f, " %.17g", param_.surface_angles_deg[(size_t) k]);
    std::fprintf(f, "\n");
    for (int s = ME_SLOT_EST; s <= ME_SLOT_GT; ++s) {
        const char *tag = s == ME_SLOT_EST ? "est" : "gt";
        const me_radius_normals_out &rn = surface_normals[s];
        std::fprintf(f, "%s normals %lld %lld %lld\n", tag, (long long) rn.n, (long long) rn.n_valid, (long long) rn.sum_k);
        std::fprintf(f, "%s %lld %lld %lld %.17g %.17g %.17g %.17g %.17g %lld\n", tag, (long long) o[s].n_query, (long long) o[s].n_used,
                     (long long) o[s].n_normal_used, o[s].sum_e, o[s].sum_e2, o[s].sum_t2, o[s].sum_c, o[s].max_e, (long long) o[s].argmax);
        for (int k = 0; k < p.n_thresholds; ++k)
            std::fprintf(f, "%s t %.17g %lld %.17g\n", tag, p.tau[k], (long long) o[s].n_within[k], o[s].sum_e2_within[k]);
        for (int k = 0; k < p.n_angles; ++k)
            std::fprintf(f, "%s a %.17g %.17g %lld\n", tag, param_.surface_angles_deg[(size_t) k], p.cos_min[k], (long long) o[s].n_angle[k]);
    }
    if (std::fclose(f) != 0) fail("writing " + path + " failed");
}

void MapEval::saveRegistrationResults() {
    // identical lines and precisions to map_eval.cpp:439-476
    file_result << std::fixed << std::setprecision(15) << "RMSE/AC: " << eigen_row(est_gt_results.at(1), 15) << std::endl;
    file_result << std::fixed << std::setprecision(15) << "Comp: " << eigen_row(est_gt_results.at(2), 15) << std::endl;
    file_result << std::fixed << std::setprecision(5) << "FULL CD: " << full_chamfer_dist << std::endl;
    if (param_.evaluate_error_distribution) saveErrorDistribution();
    if (param_.evaluate_surface_error) saveSurfaceError();
    if (param_.evaluate_m3c2) saveM3C2();
    if (param_.evaluate_mesh_distance) saveMeshDistance();
    if (param_.evaluate_mesh) saveReconstruction();
    if (param_.evaluate_observable) saveObservable();
    if (param_.evaluate_deformation) saveDeformation();
    if (param_.evaluate_voxel_distances) saveVoxelDistances();
    if (param_.evaluate_voxel_transport) saveVoxelTransport();
    file_result << std::fixed << std::setprecision(5) << "VMD: " << vmd << std::endl;
    file_result << std::fixed << std::setprecision(5) << "SCS: " << scs_overall << std::endl;
    if (param_.evaluate_using_initial_)
        file_result << "Time load-MME-mesh-ICP-Metric-AC-FCD: " << t1 / 1000.0 << " " << (t2 - t1) / 1000.0 << " " << 0.0 << " "
                    << 0.0 << " " << (t5 - t2) / 1000.0 << " " << t_acc << " " << t_fcd << std::endl;
    else  // t3..t5 come from performRegistration's own clock (map_eval.cpp:192, :465-467)
        file_result << "Time load-MME-mesh-ICP-Metric-AC-FCD: " << t1 / 1000.0 << " " << (t2 - t1) / 1000.0 << " " << t3 / 1000.0
                    << " " << (t4 - t3) / 1000.0 << " " << (t5 - t4) / 1000.0 << " " << t_acc << " " << t_fcd << std::endl;
    file_result << "VMD Time voxelization-WD-CDF-SCS: " << t_v / 1000.0 << " " << (t_vmd - t_v) / 1000.0 << " "
                << (t_cdf - t_vmd) / 1000.0 << " " << (t_scs - t_cdf) / 1000.0 << std::endl;
    file_result << "AC+MME Time: " << t_acc + (t2 - t1) / 1000.0 << std::endl;
    file_result << "CD+MME Time: " << t_fcd + (t2 - t1) / 1000.0 << std::endl;
    file_result << "AWD+SCS Time: " << t_v / 1000.0 + (t_vmd - t_v) / 1000.0 + (t_scs - t_cdf) / 1000.0 << std::endl;
    file_result.close();
    if (param_.enable_debug) std::cout << "INFO: Results saved to " << results_subfolder + "map_results.txt" << std::endl;
    // raw_rendered_dis_map.pcd / inlier_rendered_dis_map.pcd (:485-495): the map coloured by min(d2, trunc[0]) / trunc[0]
    // (renderDistanceOnPointCloud, :586-607).  The reference runs a serial KD-tree pass for it; the squared distances of
    // the est -> gt search are still on the device.  Inlier cloud = corresponding_cloud_est, the gated rows (:1086-1087).
    {
        const size_t n = map_3d_->size();
        std::vector<double> rgb(n * 3);
        std::vector<uint8_t> inl(n);
        const int mode = param_.evaluate_using_initial_ ? ME_GATE_LE_UNSQUARED : ME_GATE_LT_SQUARED;
        if (me_render_distance(ctx_, ME_SLOT_EST, param_.trunc_dist_[0], param_.icp_max_distance_, mode, rgb.data(), inl.data()) !=
            ME_OK) {
            fail(me_last_error(ctx_));
            return;
        }
        pcio::write_pcd(results_subfolder + "raw_rendered_dis_map.pcd", map_3d_->points_.data(), n, pack_rgb(rgb).data());
        std::vector<double> ixyz, irgb;
        for (size_t i = 0; i < n; ++i)
            if (inl[i])
                for (int k = 0; k < 3; ++k) {
                    ixyz.push_back(map_3d_->points_[3 * i + k]);
                    irgb.push_back(rgb[3 * i + k]);
                }
        pcio::write_pcd(results_subfolder + "inlier_rendered_dis_map.pcd", ixyz.data(), ixyz.size() / 3, pack_rgb(irgb).data());
        if (param_.enable_debug)
            std::cout << "INFO: Saved raw / inlier distance error maps to " << results_subfolder << "{raw,inlier}_rendered_dis_map.pcd"
                      << std::endl;
    }
    // the noised ground truth as evaluated, i.e. after the transform (:502-505)
    if (param_.evaluate_noised_gt_) {
        pcio::write_pcd(results_subfolder + "noise_gt_map.pcd", map_3d_->points_.data(), map_3d_->size());
        if (param_.enable_debug) std::cout << "INFO: Saved noisy ground truth map to " << results_subfolder + "noise_gt_map.pcd" << std::endl;
    }
}

me_perturb_params MapEval::perturbParams(double noise_std) const {
    me_perturb_params pp{};
    pp.noise_std = noise_std;
    pp.sparse_ratio = param_.noise_sparse_ratio;
    pp.dense_ratio = param_.noise_dense_ratio;
    pp.region_size = param_.noise_region_size;
    pp.outlier_ratio = param_.noise_outlier_ratio;
    pp.outlier_range = param_.noise_outlier_range;
    pp.deform_radius = param_.noise_deform_radius;
    pp.deform_strength = param_.noise_deform_strength;
    for (int a = 0; a < 3; ++a) pp.deform_center[a] = param_.noise_deform_center[a];
    pp.seed = param_.noise_seed;
    return pp;
}

// outlier_removal.txt (remove_outliers: statistical | radius; no reference counterpart): the map, and with outlier_filter_gt the ground
// truth, filtered in place on the device (me_statistical_outlier / me_radius_outlier + me_outlier_select_into); the host copies take the
// kept points, so every writer sees the filtered clouds.  The file: the method, its parameters ("name value"), then per filtered cloud
// "<est|gt> n_in n_kept mean std_dev threshold" (radius: mean = std_dev = 0, threshold = nb_points).
// remove_outliers: cluster (me_cluster_dbscan + me_cluster_keep): "eps", "min_points", "min_cluster_size", "keep_largest", then per
// filtered cloud "<est|gt> n_in n_clusters n_core n_border n_noise largest kept".
int MapEval::removeOutliers() {
    if (param_.remove_outliers == "cluster") return removeSmallClusters();
    if (param_.remove_outliers == "plane") return removeLargestPlane();
    const bool sor = param_.remove_outliers == "statistical";
    std::filesystem::create_directories(results_subfolder);
    const std::string path = results_subfolder + "outlier_removal.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail("cannot write " + path);
    std::fprintf(f, "method %s\n", param_.remove_outliers.c_str());
    if (sor) std::fprintf(f, "nb_neighbors %d\nstd_ratio %.17g\n", param_.outlier_nb_neighbors, param_.outlier_std_ratio);
    else std::fprintf(f, "nb_points %d\nradius %.17g\n", param_.outlier_nb_points, param_.outlier_radius);
    std::fprintf(f, "filter_gt %s\n", param_.outlier_filter_gt ? "true" : "false");
    for (int s : {ME_SLOT_EST, ME_SLOT_GT}) {
        if (s == ME_SLOT_GT && !param_.outlier_filter_gt) break;
        me_outlier_info info{};
        const int rc = sor ? me_statistical_outlier(ctx_, s, param_.outlier_nb_neighbors, param_.outlier_std_ratio, nullptr, nullptr, &info)
                           : me_radius_outlier(ctx_, s, param_.outlier_nb_points, param_.outlier_radius, nullptr, nullptr, &info);
        int64_t n = 0;
        if (rc != ME_OK || me_outlier_select_into(ctx_, s, ctx_, s, &n) != ME_OK) {
            std::fclose(f);
            return fail(std::string("remove_outliers: ") + me_last_error(ctx_));
        }
        PointCloud &pc = s == ME_SLOT_EST ? *map_3d_ : *gt_3d_;
        pc.points_.resize((size_t) n * 3);
        if (me_download_cloud(ctx_, s, pc.points_.data()) != ME_OK) {
            std::fclose(f);
            return fail(me_last_error(ctx_));
        }
        std::fprintf(f, "%s %lld %lld %.17g %.17g %.17g\n", s == ME_SLOT_EST ? "est" : "gt", (long long) info.n_in, (long long) info.n_kept,
                     info.mean, info.std_dev, info.threshold);
    }
    if (std::fclose(f) != 0) return fail("writing " + path + " failed");
    return 0;
}

// remove_outliers: plane (me_segment_planes with one plane + me_plane_keep(0, inverted)): the plane_* parameters, then per filtered
// cloud "<est|gt> n_in n_kept count h a b c d rms"; a cloud without a plane of plane_min_inliers points stays as it is (count 0).
int MapEval::removeLargestPlane() {
    std::filesystem::create_directories(results_subfolder);
    const std::string path = results_subfolder + "outlier_removal.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail("cannot write " + path);
    std::fprintf(f, "method plane\ndistance_threshold %.17g\nnum_iterations %lld\nmin_inliers %lld\nseed %llu\nrefit %s\n",
                 param_.plane_distance_threshold, (long long) param_.plane_num_iterations, (long long) param_.plane_min_inliers,
                 (unsigned long long) param_.plane_seed, param_.plane_refit ? "true" : "false");
    std::fprintf(f, "filter_gt %s\n", param_.outlier_filter_gt ? "true" : "false");
    const me_plane_params pp = planeParams(1);
    for (int s : {ME_SLOT_EST, ME_SLOT_GT}) {
        if (s == ME_SLOT_GT && !param_.outlier_filter_gt) break;
        me_plane_record rec{};
        me_plane_info pi{};
        me_outlier_info info{};
        int64_t n = 0;
        bool ok = me_segment_planes(ctx_, s, &pp, &rec, nullptr, nullptr, &pi) == ME_OK;
        n = pi.n_in;
        if (ok && pi.n_planes > 0)
            ok = me_plane_keep(ctx_, s, 0, 1, nullptr, &info) == ME_OK && me_outlier_select_into(ctx_, s, ctx_, s, &n) == ME_OK;
        if (!ok) {
            std::fclose(f);
            return fail(std::string("remove_outliers: ") + me_last_error(ctx_));
        }
        PointCloud &pc = s == ME_SLOT_EST ? *map_3d_ : *gt_3d_;
        pc.points_.resize((size_t) n * 3);
        if (me_download_cloud(ctx_, s, pc.points_.data()) != ME_OK) {
            std::fclose(f);
            return fail(me_last_error(ctx_));
        }
        std::fprintf(f, "%s %lld %lld %lld %lld %.17g %.17g %.17g %.17g %.17g\n", s == ME_SLOT_EST ? "est" : "gt", (long long) pi.n_in,
                     (long long) n, (long long) rec.count, (long long) (pi.n_planes > 0 ? rec.h : -1), rec.plane[0], rec.plane[1], rec.plane[2],
                     rec.plane[3], rec.rms);
    }
    if (std::fclose(f) != 0) return fail("writing " + path + " failed");
    return 0;
}

int MapEval::removeSmallClusters() {
    std::filesystem::create_directories(results_subfolder);
    const std::string path = results_subfolder + "outlier_removal.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail("cannot write " + path);
    std::fprintf(f, "method cluster\neps %.17g\nmin_points %d\nmin_cluster_size %d\nkeep_largest %d\n", param_.outlier_eps,
                 param_.outlier_min_points, param_.outlier_min_cluster_size, param_.outlier_keep_largest);
    std::fprintf(f, "filter_gt %s\n", param_.outlier_filter_gt ? "true" : "false");
    for (int s : {ME_SLOT_EST, ME_SLOT_GT}) {
        if (s == ME_SLOT_GT && !param_.outlier_filter_gt) break;
        me_cluster_info ci{};
        me_outlier_info info{};
        int64_t n = 0;
        if (me_cluster_dbscan(ctx_, s, param_.outlier_eps, param_.outlier_min_points, nullptr, nullptr, &ci) != ME_OK ||
            me_cluster_keep(ctx_, s, param_.outlier_min_cluster_size, param_.outlier_keep_largest, nullptr, &info) != ME_OK ||
            me_outlier_select_into(ctx_, s, ctx_, s, &n) != ME_OK) {
            std::fclose(f);
            return fail(std::string("remove_outliers: ") + me_last_error(ctx_));
        }
        PointCloud &pc = s == ME_SLOT_EST ? *map_3d_ : *gt_3d_;
        pc.points_.resize((size_t) n * 3);
        if (me_download_cloud(ctx_, s, pc.points_.data()) != ME_OK) {
            std::fclose(f);
            return fail(me_last_error(ctx_));
        }
        std::fprintf(f, "%s %lld %lld %lld %lld %lld %lld %lld\n", s == ME_SLOT_EST ? "est" : "gt", (long long) ci.n_in, (long long) ci.n_clusters,
                     (long long) ci.n_core, (long long) ci.n_border, (long long) ci.n_noise, (long long) ci.largest, (long long) info.n_kept);
    }
    if (std::fclose(f) != 0) return fail("writing " + path + " failed");
    return 0;
}

// global_registration.txt (global_registration: true; no reference counterpart): the initial pose found on the device.  Coarse copies of
// the map as loaded and of the ground truth are made in a second context (me_voxel_downsample_into), the coarse map is moved by
// initial_matrix, and me_global_register gives T_c (coarse map -> ground truth).  The file holds T_c (four rows, %.17g), then fitness,
// inlier RMSE, the correspondence count, the valid hypothesis count and the seed, one "name value" per line.
int MapEval::globalRegistration(double T_c[16]) {
    me_ctx *co = me_create(param_.gpu_device, 0);
    if (!co) return fail(std::string("global_registration: ") + me_last_error(nullptr));
    struct Destroy {
        me_ctx *c;
        ~Destroy() { me_destroy(c); }
    } d{co};
    int64_t n = 0;
    me_outlier_info oinfo[2]{};
    const int k_out = param_.global_outlier_nb_neighbors;
    if (k_out > 0) {  // SOR on the full-resolution clouds; the kept points go to the second context, which down-samples them in place
        for (int s : {ME_SLOT_EST, ME_SLOT_GT}) {
            if (me_statistical_outlier(ctx_, s, k_out, param_.global_outlier_std_ratio, nullptr, nullptr, &oinfo[s]) != ME_OK)
                return fail(std::string("global_registration: ") + me_last_error(ctx_));
            if (me_outlier_select_into(ctx_, s, co, s, &n) != ME_OK || me_voxel_downsample(co, s, param_.global_voxel_size, &n) != ME_OK)
                return fail(std::string("global_registration: ") + me_last_error(co));
        }
    } else if (me_voxel_downsample_into(ctx_, ME_SLOT_EST, co, ME_SLOT_EST, param_.global_voxel_size, &n) != ME_OK ||
               me_voxel_downsample_into(ctx_, ME_SLOT_GT, co, ME_SLOT_GT, param_.global_voxel_size, &n) != ME_OK) {
        return fail(std::string("global_registration: ") + me_last_error(co));
    }
    bool identity = true;
    for (int i = 0; i < 16; ++i) identity = identity && (param_.initial_matrix_[i] == ((i % 5 == 0) ? 1.0 : 0.0));
    if (!identity && me_transform_cloud(co, ME_SLOT_EST, param_.initial_matrix_.data()) != ME_OK)
        return fail(std::string("global_registration: ") + me_last_error(co));
    me_globreg_params gp{};
    gp.fpfh.radius = param_.global_feature_radius > 0 ? param_.global_feature_radius : 5.0 * param_.global_voxel_size;
    gp.fpfh.max_nn = param_.global_max_nn;
    gp.fpfh.normal_knn = param_.global_normal_knn;
    gp.max_corr_dist = param_.global_max_corr_dist > 0 ? param_.global_max_corr_dist : 1.5 * param_.global_voxel_size;
    gp.edge_ratio = param_.global_edge_ratio;
    gp.max_iterations = param_.global_max_iterations;
    gp.validate_top = 64;
    gp.mutual = param_.global_mutual_filter ? 1 : 0;
    gp.seed = param_.global_seed;
    me_globreg_info info{};
    if (me_global_register(co, ME_SLOT_EST, ME_SLOT_GT, &gp, T_c, &info, nullptr) != ME_OK)
        return fail(std::string("global_registration: ") + me_last_error(co));
    std::filesystem::create_directories(results_subfolder);
    const std::string path = results_subfolder + "global_registration.txt";
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return fail("cannot write " + path);
    for (int r = 0; r < 4; ++r)
        std::fprintf(f, "%.17g %.17g %.17g %.17g\n", T_c[4 * r], T_c[4 * r + 1], T_c[4 * r + 2], T_c[4 * r + 3]);
    std::fprintf(f, "fitness %.17g\ninlier_rmse %.17g\ncorrespondences %lld\nvalid_hypotheses %lld\nseed %llu\n", info.fitness,
                 info.inlier_rmse, (long long) info.n_corr, (long long) info.n_valid_hypotheses, (unsigned long long) param_.global_seed);
    if (k_out > 0) {  // the filter's lines: only when it ran
        std::fprintf(f, "outlier_nb_neighbors %d\noutlier_std_ratio %.17g\n", k_out, param_.global_outlier_std_ratio);
        const char *name[2] = {"outlier_est", "outlier_gt"};
        for (int s = 0; s < 2; ++s)
            std::fprintf(f, "%s %lld %lld %.17g %.17g %.17g\n", name[s], (long long) oinfo[s].n_in, (long long) oinfo[s].n_kept,
                         oinfo[s].mean, oinfo[s].std_dev, oinfo[s].threshold);
    }
    if (std::fclose(f) != 0) return fail("writing " + path + " failed");
    if (info.fitness < param_.global_min_fitness) {
        std::ostringstream m;
        m << "global_registration: fitness " << info.fitness << " of the coarse alignment is below global_min_fitness "
          << param_.global_min_fitness << "; not evaluating a map that may be misaligned";
        return fail(m.str());
    }
    return 0;
}

// noise_sweep.txt (noise_sweep: [..]; no reference counterpart): the robustness sweep of the paper's noise-sensitivity experiment on
// the resident ground truth — it was read, down-sampled and indexed once; each level regenerates the map from it (same seed and
// stages, noise_std_dev = the level) and runs the whole suite on the two resident clouds.  One row per level:
// noise_std_dev n_est ac[5] com[5] full_cd mme_est mme_gt awd scs  (ac = est -> gt rmse "RMSE/AC", com = fitness "Comp")
int MapEval::runNoiseSweep() {
    me_suite_params sp{};
    sp.icp_max_distance = param_.icp_max_distance_;
    sp.gate_mode = ME_GATE_LE_UNSQUARED;  // (:1219, as processOneCall)
    for (int k = 0; k < 5; ++k) sp.trunc[k] = param_.trunc_dist_[k];
    sp.nn_radius = param_.nn_radius_;
    sp.vmd_voxel_size = param_.vmd_voxel_size_;
    sp.evaluate_mme = param_.evaluate_mme_ ? 1 : 0;
    sp.evaluate_gt_mme = param_.evaluate_gt_mme_ ? 1 : 0;
    sp.min_pts = 100;
    sp.scs_radius = 5;
    std::ofstream f(results_subfolder + "noise_sweep.txt");
    if (!f.is_open()) return fail("cannot write " + results_subfolder + "noise_sweep.txt");
    f << "# noise_std_dev n_est ac0 ac1 ac2 ac3 ac4 com0 com1 com2 com3 com4 full_cd mme_est mme_gt awd scs\n";
    f << std::setprecision(17);
    for (const double sigma : param_.noise_sweep) {
        TicToc clock;
        const me_perturb_params pp = perturbParams(sigma);
        int64_t ne = 0;
        me_suite_out so;
        if (me_perturb_cloud(ctx_, ME_SLOT_EST, ME_SLOT_GT, &pp, &ne) != ME_OK ||
            me_run_suite_from(ctx_, nullptr, 0, nullptr, 0, param_.initial_matrix_.data(), &sp, ME_SUITE_OVERLAP, &so) != ME_OK)
            return fail(me_last_error(ctx_));
        const double cd = param_.strict_reference ? 0.0 : so.est_gt.mean_nn_dist + so.gt_est.mean_nn_dist;  // (as finishInitialMatrixMetrics)
        f << sigma << " " << ne;
        for (int k = 0; k < 5; ++k) f << " " << so.est_gt.rmse[k];
        for (int k = 0; k < 5; ++k) f << " " << so.est_gt.fitness[k];
        f << " " << cd << " " << (param_.evaluate_mme_ ? so.mme_est : 0.0) << " " << (param_.evaluate_mme_ ? so.mme_gt : 0.0) << " " << so.awd
          << " " << so.scs << "\n";
        std::cout << std::setprecision(6) << "INFO: noise sweep, noise_std_dev " << sigma << ": " << ne << " points, AC " << so.est_gt.rmse[0]
                  << ", " << clock.toc() << " ms" << std::endl;
    }
    if (!f.good()) return fail("writing " + results_subfolder + "noise_sweep.txt failed");
    return 0;
}
