"""ICP registration on the device-side correspondence / reduction step.

Restates the loop of Open3D's pipelines::registration::RegistrationICP [upstream] with the default ICPConvergenceCriteria
(relative_fitness = relative_rmse = 1e-6, max_iteration = 30), which the reference calls at map_eval.cpp:1366-1394:
  registration_methods 0  TransformationEstimationPointToPoint   -> icp_point_to_point  (me_icp_p2p_sums + Kabsch)
  registration_methods 1  TransformationEstimationPointToPlane   -> icp_point_to_plane  (me_icp_lsq_sums, 6x6 solve)
  registration_methods 2  RegistrationGeneralizedICP             -> icp_generalized     (me_estimate_normals(20) +
                                                                    me_gicp_covariances(1e-3) + me_icp_lsq_sums)
Per iteration the GPU does the 1-NN search with the `d2 < max^2` gate (me_nn1) and the sums; the small solve below runs
on the host; me_transform_cloud applies the update (points, normals and covariances).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .engine import ME_SLOT_EST, ME_SLOT_GT


def kabsch_update(n: int, sum_p, sum_q, sum_pq) -> np.ndarray:
    """Rigid update minimising sum |R p + t - q|^2 from the raw sums (Eigen::umeyama without scaling)."""
    sum_p, sum_q = np.asarray(sum_p, float), np.asarray(sum_q, float)
    pbar, qbar = sum_p / n, sum_q / n
    H = (np.asarray(sum_pq, float).reshape(3, 3) - n * np.outer(pbar, qbar)) / n  # cov(p, q) = E[(p-pbar)(q-qbar)^T]
    U, _, Vt = np.linalg.svd(H.T)  # sigma = E[(q-qbar)(p-pbar)^T] = H^T
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = qbar - R @ pbar
    return T


def _shift(T: np.ndarray, origin) -> np.ndarray:
    """The sums are relative to `origin`; express the update in absolute coordinates: x -> o + R (x - o) + t."""
    o = np.asarray(origin, float)
    A = np.eye(4)
    A[:3, :3] = T[:3, :3]
    A[:3, 3] = o + T[:3, 3] - T[:3, :3] @ o
    return A


def icp_point_to_point(eng, max_distance: float, max_iteration: int = 30, relative_fitness: float = 1e-6,
                       relative_rmse: float = 1e-6):
    """RegistrationICP(source = slot EST as uploaded (already moved by the initial matrix), target = slot GT).

    Returns dict(transformation (4x4 update accumulated on top of the uploaded state), fitness, inlier_rmse, n_corr,
    iterations).  On return slot EST holds the registered map (as `*map_3d_ = map_3d_->Transform(trans)`, :1392).
    """
    def evaluate():
        eng.nn1(ME_SLOT_EST, ME_SLOT_GT, fetch=False)
        s = eng.icp_p2p_sums(ME_SLOT_EST, max_distance)
        fit = s.n_corr / s.n_source if s.n_source else 0.0
        rmse = float(np.sqrt(s.sum_d2 / s.n_corr)) if s.n_corr else 0.0
        return s, fit, rmse

    total = np.eye(4)
    s, fit, rmse = evaluate()
    it = 0
    for it in range(1, max_iteration + 1):
        if s.n_corr < 3:
            break
        upd = _shift(kabsch_update(s.n_corr, list(s.sum_p), list(s.sum_q), list(s.sum_pq)), list(s.origin))
        total = upd @ total
        eng.transform_cloud(ME_SLOT_EST, upd)
        prev_fit, prev_rmse = fit, rmse
        s, fit, rmse = evaluate()
        if abs(prev_fit - fit) < relative_fitness and abs(prev_rmse - rmse) < relative_rmse:
            break
    return dict(transformation=total, fitness=fit, inlier_rmse=rmse, n_corr=int(s.n_corr), iterations=it)


def vector6_to_matrix(x) -> np.ndarray:
    """open3d utility::TransformVector6dToMatrix4d: R = Rz(x[2]) Ry(x[1]) Rx(x[0]), t = x[3:6]."""
    a, b, g = float(x[0]), float(x[1]), float(x[2])
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = np.asarray(x[3:6], float)
    return T


def lsq_update(JTJ, JTr) -> np.ndarray:
    """utility::SolveJacobianSystemAndObtainExtrinsicMatrix: x = solve(JTJ, -JTr) -> 4x4; identity when singular."""
    A = np.asarray(JTJ, float).reshape(6, 6)
    b = -np.asarray(JTr, float).reshape(6)
    try:
        x = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return np.eye(4)
    return vector6_to_matrix(x) if np.all(np.isfinite(x)) else np.eye(4)


def _kernel_scale(kernel, kernel_scale) -> float:
    """The scale handed to the library: L2 and L1 read none; the others need one from the caller (no default is invented)."""
    kid = _lib.ROBUST_KERNELS.get(kernel.lower()) if isinstance(kernel, str) else int(kernel)
    if kid in (_lib.ME_ROBUST_L2, _lib.ME_ROBUST_L1):
        return 1.0 if kernel_scale is None else float(kernel_scale)
    if kernel_scale is None:
        raise ValueError(f"robust kernel {kernel!r} needs kernel_scale")
    return float(kernel_scale)


def _icp_lsq(eng, mode: int, max_distance: float, max_iteration: int, relative_fitness: float, relative_rmse: float, kernel=None,
             kernel_scale=None):
    if kernel is not None:
        kernel_scale = _kernel_scale(kernel, kernel_scale)

    def evaluate():
        eng.nn1(ME_SLOT_EST, ME_SLOT_GT, fetch=False)
        if kernel is None:
            s = eng.icp_lsq_sums(ME_SLOT_EST, mode, max_distance)
        else:
            s = eng.icp_lsq_sums_robust(ME_SLOT_EST, mode, max_distance, kernel, kernel_scale)
        fit = s.n_corr / s.n_source if s.n_source else 0.0
        rmse = float(np.sqrt(s.sum_d2 / s.n_corr)) if s.n_corr else 0.0
        return s, fit, rmse

    total = np.eye(4)
    s, fit, rmse = evaluate()
    it = 0
    for it in range(1, max_iteration + 1):
        if s.n_corr == 0:  # ComputeTransformation returns the identity on an empty correspondence set
            break
        upd = lsq_update(list(s.JTJ), list(s.JTr))
        total = upd @ total
        eng.transform_cloud(ME_SLOT_EST, upd)
        prev_fit, prev_rmse = fit, rmse
        s, fit, rmse = evaluate()
        if abs(prev_fit - fit) < relative_fitness and abs(prev_rmse - rmse) < relative_rmse:
            break
    return dict(transformation=total, fitness=fit, inlier_rmse=rmse, n_corr=int(s.n_corr), iterations=it)


def icp_point_to_plane(eng, max_distance: float, max_iteration: int = 30, relative_fitness: float = 1e-6,
                       relative_rmse: float = 1e-6, kernel=None, kernel_scale=None):
    """RegistrationICP(.., TransformationEstimationPointToPlane(kernel)) (registration_methods 1, map_eval.cpp:1373-1377).
    The target (slot GT) must carry normals (Engine.set_normals; Open3D refuses a target without them as well).
    kernel: None (the plain step, me_icp_lsq_sums) or a robust loss by id or name with its kernel_scale (me_icp_lsq_sums_robust)."""
    return _icp_lsq(eng, 1, max_distance, max_iteration, relative_fitness, relative_rmse, kernel, kernel_scale)


def icp_generalized(eng, max_distance: float, epsilon: float = 1e-3, max_iteration: int = 30,
                    relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, kernel=None, kernel_scale=None):
    """RegistrationGeneralizedICP (registration_methods 2, map_eval.cpp:1378-1384): covariances of both clouds from
    their normals (estimated from the 20 nearest neighbours where the cloud has none), then the ICP loop.
    kernel / kernel_scale: TransformationEstimationForGeneralizedICP(epsilon, kernel), one weight per row of M^(-1/2) d."""
    eng.gicp_covariances(ME_SLOT_EST, epsilon)
    eng.gicp_covariances(ME_SLOT_GT, epsilon)
    return _icp_lsq(eng, 2, max_distance, max_iteration, relative_fitness, relative_rmse, kernel, kernel_scale)


def icp_multi_scale(eng, voxel_sizes, max_distances, max_iterations, method: int, kernel=None, kernel_scale=None,
                    epsilon: float = 1e-3):
    """Coarse-to-fine registration (Open3D's multi-scale ICP [upstream]): level l runs the loop of `method` (0, 1 or 2) with
    max_distances[l] for at most max_iterations[l] iterations.
      voxel_sizes[l] > 0   both resident slots, as they are posed now, are voxel down-sampled into a private Engine on the same device
                           (Engine.downsample_into); the copies carry no attributes, so method 1 estimates the target copy's normals
                           from 20 neighbours and method 2 calls gicp_covariances(epsilon) on both copies; the loop runs there and the
                           level's update is applied to the resident map with transform_cloud
      voxel_sizes[l] <= 0  the loop runs on the resident clouds themselves (their own normals / covariances)
    The resident ground truth is never changed.  -> dict(transformation: the accumulated 4x4, levels: per level fitness, inlier_rmse,
    n_corr, iterations and the level's own transformation)."""
    from .engine import Engine

    if not (len(voxel_sizes) == len(max_distances) == len(max_iterations)):
        raise ValueError("icp_multi_scale: voxel_sizes, max_distances and max_iterations must have the same length")
    if method not in (0, 1, 2):
        raise ValueError("icp_multi_scale: method must be 0, 1 or 2")

    def run(e, max_d, iters):
        kw = {} if kernel is None else dict(kernel=kernel, kernel_scale=kernel_scale)
        if method == 2:
            return e.performICPRegistration(max_d, 2, epsilon=epsilon, max_iteration=iters, **kw)
        return e.performICPRegistration(max_d, method, max_iteration=iters, **kw)

    total = np.eye(4)
    levels = []
    for v, max_d, iters in zip(voxel_sizes, max_distances, max_iterations):
        if v > 0:
            with Engine(eng.device) as co:
                eng.downsample_into(ME_SLOT_EST, co, ME_SLOT_EST, v)
                eng.downsample_into(ME_SLOT_GT, co, ME_SLOT_GT, v)
                if method == 1:
                    co.estimate_normals(ME_SLOT_GT, 20, fetch=False)
                r = run(co, float(max_d), int(iters))
            eng.transform_cloud(ME_SLOT_EST, r["transformation"])
        else:
            r = run(eng, float(max_d), int(iters))
        total = r["transformation"] @ total
        levels.append(dict(voxel_size=float(v), fitness=r["fitness"], inlier_rmse=r["inlier_rmse"], n_corr=r["n_corr"],
                           iterations=r["iterations"], transformation=r["transformation"]))
    return dict(transformation=total, levels=levels)
