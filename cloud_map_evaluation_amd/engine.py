"""Python face of the C ABI: numpy / torch-tensor in, numpy / dataclasses out.

`Engine` owns one me_ctx (one GPU).  Method names follow the reference's MapEval members they stand in for
(map_eval/src/map_eval.h:196-312): computeMME, calculateMetricsWithInitialMatrix, computeChamferDistance,
calculateVMD.  The C++ host (cloud_map_evaluation_amd/host/) is the drop-in for the reference executable; this
module is what tests/ and bench.py drive.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib
from ._lib import ME_GATE_LE_UNSQUARED, ME_GATE_LT_SQUARED, ME_SLOT_EST, ME_SLOT_GT  # noqa: F401


class MapEvalError(RuntimeError):
    pass


@dataclass
class Param:
    """Hot-path fields of the reference's Param (map_eval.h:60-116), same names and defaults."""
    icp_max_distance_: float = 2.5
    nn_radius_: float = 0.2
    trunc_dist_: tuple = (0.2, 0.1, 0.08, 0.05, 0.01)  # accuracy_level (config.yaml)
    initial_matrix_: np.ndarray = field(default_factory=lambda: np.eye(4))
    vmd_voxel_size_: float = 3.0
    evaluate_mme_: bool = True
    evaluate_gt_mme_: bool = True
    evaluate_using_initial_: bool = True
    use_tbb_mme: bool = True  # accepted for compatibility; the GPU path has one implementation


@dataclass
class RegStats:
    """One getDiffRegResultWithCorrespondence result block (map_eval.cpp:1140-1144)."""
    n_src: int
    n_corr: int
    mean: np.ndarray
    rmse: np.ndarray
    fitness: np.ndarray
    sigma: np.ndarray
    number: np.ndarray
    mean_nn_dist: float

    @staticmethod
    def from_c(o: _lib.NNStatsOut) -> "RegStats":
        f = lambda x: np.array(list(x), dtype=np.float64)
        return RegStats(o.n_src, o.n_corr, f(o.mean), f(o.rmse), f(o.fitness), f(o.sigma), f(o.number), o.mean_nn_dist)


def rotation_angle(R) -> np.ndarray:
    """The angle of rotation matrices (.., 9) or (.., 3, 3), radians in [0, pi]: atan2(s, c) with
    s = sqrt((R21 - R12)^2 + (R02 - R20)^2 + (R10 - R01)^2) / 2 and c = (tr R - 1) / 2 (deformation_field; the C++ host's formula)."""
    R = np.asarray(R, np.float64)
    R = R.reshape(R.shape[:-2] + (9,)) if R.shape[-2:] == (3, 3) else R
    a, b, c = R[..., 7] - R[..., 5], R[..., 2] - R[..., 6], R[..., 3] - R[..., 1]
    s = 0.5 * np.sqrt(a * a + b * b + c * c)
    return np.arctan2(s, 0.5 * (R[..., 0] + R[..., 4] + R[..., 8] - 1.0))


TRANSPORT_N_FINAL = 128  # iterations at blur^2 after the descent: chosen on the numpy model's marginal_err


def transport_schedule(voxel_size: float, blur: float, scaling: float = 0.5, n_final: int = TRANSPORT_N_FINAL) -> np.ndarray:
    """The default eps schedule of Engine.voxel_transport, host arithmetic in float64: eps_0 = 3 voxel_size^2 (the squared diameter of a
    voxel), eps_{t+1} = max(blur^2, eps_t scaling^2) down to blur^2 (once), then n_final further iterations at blur^2."""
    vs, b, sc = float(voxel_size), float(blur), float(scaling)
    if not (vs > 0 and b > 0 and 0 < sc < 1 and n_final >= 0):
        raise ValueError("transport_schedule: voxel_size > 0, blur > 0, 0 < scaling < 1 and n_final >= 0")
    b2, s2 = b * b, sc * sc
    eps = [max(b2, 3.0 * (vs * vs))]
    while eps[-1] > b2:
        eps.append(max(b2, eps[-1] * s2))
    eps.extend([b2] * int(n_final))
    if len(eps) > 512:
        raise ValueError("transport_schedule: more than 512 iterations")
    return np.array(eps, np.float64)


def _addr(a) -> int:
    """Raw address of a numpy array (host) or a torch tensor (host or device)."""
    if a is None:
        return 0
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()  # torch.Tensor


# the 44 columns of voxel_metrics.txt (Engine.voxel_metrics_table)
_NN_COLUMNS = ["n_corr"] + [f"n_inl{k}" for k in range(5)] + [f"sum_d{k}" for k in range(5)] + [f"sum_d2_{k}" for k in range(5)] + ["sum_sqrt_all"]
VOXEL_METRICS_COLUMNS = (["ix", "iy", "iz", "n_est", "n_gt"] + [c + "_est" for c in _NN_COLUMNS] + [c + "_gt" for c in _NN_COLUMNS]
                         + ["n_H_est", "sum_H_est", "n_H_gt", "sum_H_gt", "w2"])


def _pack_keys(k) -> np.ndarray:
    """(V, 3) voxel indices -> int64 keys whose order is the ascending (ix, iy, iz) order of the library's tables."""
    k = np.asarray(k, dtype=np.int64) + (1 << 20)
    return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]


class Engine:
    def __init__(self, device: int = 0, borrow_device_input: bool = False, morton_order: bool = False):
        """borrow_device_input: ME_FLAG_BORROW_DEVICE_INPUT — cuda tensors uploaded without a transform are read where they lie
        (no copy); the Engine keeps a reference to them until the slot's next upload, the caller must not modify them meanwhile.
        morton_order: ME_FLAG_MORTON_ORDER — Z curve instead of the Hilbert curve (tests / measurements)."""
        self._L = _lib.load()
        self._ctx = self._L.me_create(int(device), (1 if borrow_device_input else 0) | (2 if morton_order else 0))
        self._held = {}  # slot -> the array / tensor of its last upload (borrowed device inputs must outlive their use)
        self._shared = {}  # what the Python side remembers about the CONTEXT's results: one dict for the engine and its twin
        if not self._ctx:
            raise MapEvalError(self._L.me_last_error(None).decode())
        self.device = device

    def twin(self) -> "Engine":
        """A second lane on the same clouds (me_twin): its own stream and scratch, so that a second host thread can run
        independent work concurrently (ctypes calls release the GIL).  Owned by this engine."""
        if getattr(self, "_twin", None) is None:
            t = Engine.__new__(Engine)
            t._L = self._L
            t._ctx = self._L.me_twin(self._ctx)
            if not t._ctx:
                raise MapEvalError(self._L.me_last_error(self._ctx).decode())
            t.device = self.device
            t._held = self._held
            t._shared = self._shared  # (the reconstruction lives in the primary context: a twin's call changes what both fetch)
            t._owned = False
            t._twin = None
            self._twin = t
        return self._twin

    def close(self):
        if getattr(self, "_ctx", None):
            if getattr(self, "_owned", True):
                self._L.me_destroy(self._ctx)
                if getattr(self, "_twin", None) is not None:
                    self._twin._ctx = None  # freed with the primary context
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc: int):
        if rc != 0:
            raise MapEvalError(f"[{rc}] " + self._L.me_last_error(self._ctx).decode())

    # ---- clouds ----
    def set_shard(self, rank: int, world: int):
        self._ck(self._L.me_set_shard(self._ctx, rank, world))

    def upload(self, slot: int, xyz, T=None, cell_size: float = 0.0):
        """xyz: (N,3) float64 numpy array (host) or torch tensor (CPU or cuda, contiguous)."""
        Tm = None if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        on_device = False
        if isinstance(xyz, np.ndarray):
            xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        else:  # torch tensor
            import torch

            if xyz.dtype != torch.float64 or not xyz.is_contiguous():
                xyz = xyz.to(torch.float64).contiguous()
            on_device = xyz.is_cuda
            if on_device:
                torch.cuda.current_stream(xyz.device).synchronize()  # producer stream -> library stream hand-over
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError("expected an (N,3) array")
        fn = self._L.me_upload_cloud_device if on_device else self._L.me_upload_cloud
        self._ck(fn(self._ctx, slot, _addr(xyz), int(xyz.shape[0]), _addr(Tm), float(cell_size)))
        self._held[slot] = xyz

    def upload_slab(self, slot: int, xyz, cell_size: float = 0.0):
        """upload() for a cuda tensor that already IS this rank's slab + halo (what the halo exchange delivered): no filter."""
        import torch

        if not xyz.is_cuda:
            return self.upload(slot, xyz, cell_size=cell_size)  # (host tensor: the general path, with its filter)
        if xyz.dtype != torch.float64 or not xyz.is_contiguous():
            xyz = xyz.to(torch.float64).contiguous()
        torch.cuda.current_stream(xyz.device).synchronize()
        self._ck(self._L.me_upload_slab_device(self._ctx, slot, xyz.data_ptr(), int(xyz.shape[0]), float(cell_size)))
        self._held[slot] = xyz

    def voxel_downsample(self, slot: int, voxel_size: float) -> int:
        """open3d VoxelDownSample (map_eval.cpp:38-39) on the uploaded cloud, in place; returns the new point count."""
        n = C.c_int64(0)
        self._ck(self._L.me_voxel_downsample(self._ctx, slot, float(voxel_size), C.byref(n)))
        return n.value

    def transform_cloud(self, slot: int, T):
        """*cloud = cloud->Transform(T) (map_eval.cpp:1206) on the device."""
        Tm = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        self._ck(self._L.me_transform_cloud(self._ctx, slot, _addr(Tm)))

    def perturb(self, dst: int, src: int, *, noise_std: float = 0.0, sparse_ratio: float = 1.0, dense_ratio: float = 1.0,
                region_size: float = 0.0, outlier_ratio: float = 0.0, outlier_range: float = 0.0, deform_radius: float = 0.0,
                deform_strength: float = 0.0, deform_center=(0.0, 0.0, 0.0), seed: int = 0) -> int:
        """me_perturb_cloud: slot dst = the reference's simulation-mode copy of slot src (addLocalDeformation, addNonUniformDensity,
        addGaussianNoise, addSparseOutliers, map_eval.cpp:1745-1829, in that order; the defaults switch every stage off) with
        Philox4x64-10 randomness keyed by seed.  dst == src works in place.  Returns dst's new point count."""
        pp = _lib.PerturbParams()
        pp.noise_std = float(noise_std)
        pp.sparse_ratio = float(sparse_ratio)
        pp.dense_ratio = float(dense_ratio)
        pp.region_size = float(region_size)
        pp.outlier_ratio = float(outlier_ratio)
        pp.outlier_range = float(outlier_range)
        pp.deform_radius = float(deform_radius)
        pp.deform_strength = float(deform_strength)
        for a in range(3):
            pp.deform_center[a] = float(deform_center[a])
        pp.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        n = C.c_int64(0)
        self._ck(self._L.me_perturb_cloud(self._ctx, int(dst), int(src), C.byref(pp), C.byref(n)))
        return n.value

    # ---- coarse global registration (FPFH + RANSAC, me_globreg.hip) ----
    def downsample_into(self, src_slot: int, dst: "Engine", dst_slot: int, voxel_size: float) -> int:
        """me_voxel_downsample_into: dst's slot = the voxel down-sample of this engine's src_slot (src untouched; dst may be self, another
        slot).  Returns the point count."""
        n = C.c_int64(0)
        rc = self._L.me_voxel_downsample_into(self._ctx, int(src_slot), dst._ctx, int(dst_slot), float(voxel_size), C.byref(n))
        dst._ck(rc)  # (the library reports on dst_ctx)
        dst._held.pop(int(dst_slot), None)
        return n.value

    @staticmethod
    def _fpfh_params(radius: float, max_nn: int, normal_knn: int) -> _lib.FpfhParams:
        fp = _lib.FpfhParams()
        fp.radius, fp.max_nn, fp.normal_knn = float(radius), int(max_nn), int(normal_knn)
        return fp

    def fpfh(self, slot: int, radius: float, max_nn: int = 40, normal_knn: int = 30, fetch: bool = True):
        """me_fpfh: Open3D ComputeFPFHFeature with KDTreeSearchParamHybrid(radius, max_nn <= 40) on the resident cloud (normals estimated
        with normal_knn when the slot has none).  Returns the (N, 33) features (fetch) or None; they also stay on the device."""
        fp = self._fpfh_params(radius, max_nn, normal_knn)
        out = np.empty((self.size(slot), 33), np.float64) if fetch else None
        self._ck(self._L.me_fpfh(self._ctx, int(slot), C.byref(fp), _addr(out)))
        return out

    def fpfh_match(self, src_slot: int, ref_slot: int, mutual: bool = True):
        """me_fpfh_match: exact 1-NN in feature space.  Returns (corr, n_corr): corr[i] = matched ref point of src point i, or -1."""
        corr = np.empty(self.size(src_slot), np.int32)
        n = C.c_int64(0)
        self._ck(self._L.me_fpfh_match(self._ctx, int(src_slot), int(ref_slot), int(bool(mutual)), _addr(corr), C.byref(n)))
        return corr, n.value

    def global_register(self, src_slot: int, ref_slot: int, *, max_corr_dist: float, radius: float = 0.0, max_nn: int = 40,
                        normal_knn: int = 30, edge_ratio: float = 0.9, max_iterations: int = 1_000_000, validate_top: int = 64,
                        mutual: bool = True, seed: int = 0, scores: bool = False):
        """me_global_register: FPFH feature matching + RANSAC on the device.  Returns (T, info) — T (4x4) maps src's current
        coordinates to ref's frame, info a dict of me_globreg_info — and, with scores=True, the per-hypothesis correspondence inliers
        (-1 = invalid) as a third item."""
        gp = _lib.GlobRegParams()
        gp.fpfh = self._fpfh_params(radius, max_nn, normal_knn)
        gp.max_corr_dist = float(max_corr_dist)
        gp.edge_ratio = float(edge_ratio)
        gp.max_iterations = int(max_iterations)
        gp.validate_top = int(validate_top)
        gp.mutual = int(bool(mutual))
        gp.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        T = np.zeros(16, np.float64)
        info = _lib.GlobRegInfo()
        sc = np.empty(int(max_iterations), np.int64) if scores else None
        self._ck(self._L.me_global_register(self._ctx, int(src_slot), int(ref_slot), C.byref(gp), _addr(T), C.byref(info), _addr(sc)))
        d = {k: getattr(info, k) for k, _ in _lib.GlobRegInfo._fields_}
        return (T.reshape(4, 4), d, sc) if scores else (T.reshape(4, 4), d)

    def coarse_align(self, voxel_size: float, *, src_slot: int = 0, ref_slot: int = 1, radius: float | None = None,
                     max_corr_dist: float | None = None, outlier_nb_neighbors: int = 0, outlier_std_ratio: float = 2.0,
                     cluster_eps: float = 0.0, cluster_min_points: int = 10, cluster_min_size: int = 1, **params):
        """The initial pose: voxel_size down-samples of both resident slots in a private second context on the same device, FPFH
        (radius 5 voxel_size by default), matching and RANSAC (max_corr_dist 1.5 voxel_size by default); returns T (4x4, src -> ref).
        outlier_nb_neighbors > 0: statistical outlier removal (that k, outlier_std_ratio) on the full-resolution clouds first — the
        kept points are copied into the private context and down-sampled there in place (self.last_coarse_outliers: both infos; None
        when the filter is off).  The resident POINTS are not changed: apply T with transform_cloud and run performICPRegistration as
        usual.  With the filter on, the filter's mask replaces any outlier mask the two slots held, and their octrees are built if
        they were not yet.
        cluster_eps > 0: the DBSCAN cluster filter (cluster_eps, cluster_min_points; clusters below cluster_min_size and noise dropped)
        on the full-resolution copies as well, after the statistical filter when both are on (self.last_coarse_clusters: per cloud the
        cluster info with n_kept; None when off).  With the cluster filter alone the slots' radius grids are rebuilt at cluster_eps
        when their cell differs."""
        radius = 5.0 * voxel_size if radius is None else radius
        max_corr_dist = 1.5 * voxel_size if max_corr_dist is None else max_corr_dist
        self.last_coarse_outliers = None
        self.last_coarse_clusters = None
        with Engine(self.device) as co:
            if outlier_nb_neighbors > 0 or cluster_eps > 0:
                outl, clus = [], []
                for s, d in ((src_slot, 0), (ref_slot, 1)):
                    if outlier_nb_neighbors > 0:
                        outl.append(self.statistical_outlier(s, outlier_nb_neighbors, outlier_std_ratio))
                        self.select_kept_into(s, co, d)
                        if cluster_eps > 0:  # (on the private copy: the statistical filter's survivors)
                            ci = co.cluster_dbscan(d, cluster_eps, cluster_min_points)
                            ci["n_kept"] = co.cluster_keep(d, cluster_min_size)["n_kept"]
                            co.select_kept_into(d)
                            clus.append(ci)
                    else:
                        ci = self.cluster_dbscan(s, cluster_eps, cluster_min_points)
                        ci["n_kept"] = self.cluster_keep(s, cluster_min_size)["n_kept"]
                        self.select_kept_into(s, co, d)
                        clus.append(ci)
                    co.voxel_downsample(d, voxel_size)
                self.last_coarse_outliers = outl or None
                self.last_coarse_clusters = clus or None
            else:
                self.downsample_into(src_slot, co, 0, voxel_size)
                self.downsample_into(ref_slot, co, 1, voxel_size)
            T, info = co.global_register(0, 1, radius=radius, max_corr_dist=max_corr_dist, **params)[:2]
        self.last_coarse_info = info
        return T

    # ---- outlier removal (Open3D remove_statistical_outlier / remove_radius_outlier) ----
    @staticmethod
    def _outlier_dict(o: _lib.OutlierInfo) -> dict:
        return {f: getattr(o, f) for f, _ in o._fields_}

    def statistical_outlier(self, slot: int, nb_neighbors: int = 20, std_ratio: float = 2.0, fetch: bool = False):
        """The statistical filter's mask on the slot (kept until the cloud changes); returns the info dict, and with fetch=True also
        (avg_dist, keep) in cloud order."""
        o = _lib.OutlierInfo()
        if not fetch:
            self._ck(self._L.me_statistical_outlier(self._ctx, slot, int(nb_neighbors), float(std_ratio), 0, 0, C.byref(o)))
            return self._outlier_dict(o)
        n = self.size(slot)
        avg = np.empty(n, np.float64)
        keep = np.empty(n, np.uint8)
        self._ck(self._L.me_statistical_outlier(self._ctx, slot, int(nb_neighbors), float(std_ratio), _addr(avg), _addr(keep), C.byref(o)))
        return self._outlier_dict(o), avg, keep

    def radius_outlier(self, slot: int, nb_points: int, radius: float, fetch: bool = False):
        """The radius filter's mask on the slot; returns the info dict, and with fetch=True also (counts, keep) in cloud order."""
        o = _lib.OutlierInfo()
        if not fetch:
            self._ck(self._L.me_radius_outlier(self._ctx, slot, int(nb_points), float(radius), 0, 0, C.byref(o)))
            return self._outlier_dict(o)
        n = self.size(slot)
        counts = np.empty(n, np.int32)
        keep = np.empty(n, np.uint8)
        self._ck(self._L.me_radius_outlier(self._ctx, slot, int(nb_points), float(radius), _addr(counts), _addr(keep), C.byref(o)))
        return self._outlier_dict(o), counts, keep

    def select_kept_into(self, src_slot: int, dst: "Engine | None" = None, dst_slot: int | None = None) -> int:
        """The kept points of the slot's last mask into dst's dst_slot (default: this engine, the same slot — in place)."""
        dst = self if dst is None else dst
        dst_slot = src_slot if dst_slot is None else dst_slot
        n = C.c_int64(0)
        rc = self._L.me_outlier_select_into(self._ctx, int(src_slot), dst._ctx, int(dst_slot), C.byref(n))
        dst._ck(rc)  # (the library reports on dst_ctx)
        dst._held.pop(int(dst_slot), None)
        return int(n.value)

    def remove_statistical_outlier(self, slot: int, nb_neighbors: int = 20, std_ratio: float = 2.0):
        """Open3D's remove_statistical_outlier, in place: returns (n_kept, info)."""
        info = self.statistical_outlier(slot, nb_neighbors, std_ratio)
        return self.select_kept_into(slot), info

    def remove_radius_outlier(self, slot: int, nb_points: int, radius: float):
        """Open3D's remove_radius_outlier, in place: returns (n_kept, info)."""
        info = self.radius_outlier(slot, nb_points, radius)
        return self.select_kept_into(slot), info

    # ---- clustering (Open3D cluster_dbscan) and the cluster-size filter (me_cluster.hip) ----
    def cluster_dbscan(self, slot: int, eps: float, min_points: int, fetch: bool = False):
        """me_cluster_dbscan: labels and cluster sizes stay on the slot until the cloud changes; returns the info dict, and with
        fetch=True also (labels, counts) in cloud order (-1 = noise; counts include the point itself)."""
        o = _lib.ClusterInfo()
        if not fetch:
            self._ck(self._L.me_cluster_dbscan(self._ctx, int(slot), float(eps), int(min_points), 0, 0, C.byref(o)))
            return {f: getattr(o, f) for f, _ in o._fields_}
        n = self.size(slot)
        labels = np.empty(n, np.int32)
        counts = np.empty(n, np.int32)
        self._ck(self._L.me_cluster_dbscan(self._ctx, int(slot), float(eps), int(min_points), _addr(labels), _addr(counts), C.byref(o)))
        return {f: getattr(o, f) for f, _ in o._fields_}, labels, counts

    def cluster_sizes(self, slot: int) -> np.ndarray:
        """me_cluster_sizes: points per cluster id (core and border) of the slot's last cluster_dbscan, int64."""
        m = C.c_int64(0)
        self._ck(self._L.me_cluster_sizes(self._ctx, int(slot), 0, 0, C.byref(m)))
        sizes = np.empty(m.value, np.int64)
        if m.value:
            self._ck(self._L.me_cluster_sizes(self._ctx, int(slot), _addr(sizes), int(m.value), C.byref(m)))
        return sizes

    def cluster_keep(self, slot: int, min_cluster_size: int = 1, keep_largest: int = 0, fetch: bool = False):
        """me_cluster_keep: the slot's keep-mask = the points of clusters with at least min_cluster_size points (and, keep_largest > 0,
        among the keep_largest largest); noise is dropped.  Returns the info dict, and with fetch=True also the mask (cloud order)."""
        o = _lib.OutlierInfo()
        keep = np.empty(self.size(slot), np.uint8) if fetch else None
        self._ck(self._L.me_cluster_keep(self._ctx, int(slot), int(min_cluster_size), int(keep_largest), _addr(keep), C.byref(o)))
        return (self._outlier_dict(o), keep) if fetch else self._outlier_dict(o)

    def remove_small_clusters(self, slot: int, eps: float, min_points: int, min_cluster_size: int = 1, keep_largest: int = 0):
        """DBSCAN + the cluster-size filter, in place: returns (n_kept, info) — info = the cluster info with the filter's n_kept."""
        info = self.cluster_dbscan(slot, eps, min_points)
        info["n_kept"] = self.cluster_keep(slot, min_cluster_size, keep_largest)["n_kept"]
        return self.select_kept_into(slot), info

    # ---- plane segmentation (Open3D segment_plane) and multi-plane extraction (me_plane.hip) ----
    @staticmethod
    def _plane_dict(r: _lib.PlaneRecord) -> dict:
        return {"count": int(r.count), "h": int(r.h), "score": int(r.score), "plane": np.array(list(r.plane), np.float64), "rms": r.rms,
                "mean_abs": r.mean_abs, "max_abs": r.max_abs, "refit_degenerate": int(r.refit_degenerate)}

    def segment_planes(self, slot: int, distance_threshold: float, num_iterations: int = 1000, max_planes: int = 1, min_inliers: int = 3,
                       refit: bool = True, seed: int = 0, fetch: bool = False):
        """me_segment_planes: up to max_planes RANSAC planes, each on what the earlier ones left; labels and records stay on the slot
        until the cloud changes.  Returns (info, planes) — planes = one dict per plane (count, h, score, plane = (a, b, c, d), rms,
        mean_abs, max_abs, refit_degenerate) — and with fetch=True also (labels [N] int32 in cloud order, -1 = no plane; scores
        [max_planes, num_iterations] int64, -1 = invalid hypothesis or round not reached)."""
        prm = _lib.PlaneParams(float(distance_threshold), int(num_iterations), int(max_planes), int(bool(refit)), int(min_inliers),
                               int(seed) & 0xFFFFFFFFFFFFFFFF)
        o = _lib.PlaneInfo()
        cap = max(1, min(int(max_planes), 64))
        recs = (_lib.PlaneRecord * cap)()
        labels = scores = None
        if fetch:
            labels = np.empty(self.size(slot), np.int32)
            if 1 <= int(max_planes) <= 64 and 1 <= int(num_iterations) <= 1 << 24:
                scores = np.empty((int(max_planes), int(num_iterations)), np.int64)
        self._ck(self._L.me_segment_planes(self._ctx, int(slot), C.byref(prm), C.addressof(recs), _addr(labels), _addr(scores), C.byref(o)))
        info = {f: getattr(o, f) for f, _ in o._fields_}
        planes = [self._plane_dict(recs[k]) for k in range(int(o.n_planes))]
        return (info, planes, labels, scores) if fetch else (info, planes)

    def segment_plane(self, slot: int, distance_threshold: float, num_iterations: int = 1000, min_inliers: int = 3, refit: bool = True,
                      seed: int = 0):
        """Open3D's segment_plane(distance_threshold, 3, num_iterations): (plane (a, b, c, d), inlier indices in cloud order); without a
        plane (None, an empty index array)."""
        _, planes, labels, _ = self.segment_planes(slot, distance_threshold, num_iterations, 1, min_inliers, refit, seed, fetch=True)
        if not planes:
            return None, np.empty(0, np.int64)
        return planes[0]["plane"], np.flatnonzero(labels == 0)

    def plane_fetch(self, slot: int):
        """me_plane_fetch: (planes, labels) of the slot's last segment_planes."""
        m = C.c_int64(0)
        self._ck(self._L.me_plane_fetch(self._ctx, int(slot), 0, 0, C.byref(m), 0))
        recs = (_lib.PlaneRecord * max(1, m.value))()
        labels = np.empty(self.size(slot), np.int32)
        self._ck(self._L.me_plane_fetch(self._ctx, int(slot), C.addressof(recs), int(m.value), C.byref(m), _addr(labels)))
        return [self._plane_dict(recs[k]) for k in range(m.value)], labels

    def plane_keep(self, slot: int, plane: int = -1, invert: bool = False, fetch: bool = False):
        """me_plane_keep: the slot's keep-mask = the points of that plane (plane = -1: of any plane), or with invert the others.
        Returns the info dict, and with fetch=True also the mask (cloud order)."""
        o = _lib.OutlierInfo()
        keep = np.empty(self.size(slot), np.uint8) if fetch else None
        self._ck(self._L.me_plane_keep(self._ctx, int(slot), int(plane), int(bool(invert)), _addr(keep), C.byref(o)))
        return (self._outlier_dict(o), keep) if fetch else self._outlier_dict(o)

    def remove_plane(self, slot: int, distance_threshold: float, num_iterations: int = 1000, min_inliers: int = 3, refit: bool = True,
                     seed: int = 0):
        """Segment the largest plane and remove its points, in place (ground removal): returns (n_kept, info, planes); without a plane
        the cloud stays as it is."""
        info, planes = self.segment_planes(slot, distance_threshold, num_iterations, 1, min_inliers, refit, seed)
        if not planes:
            return self.size(slot), info, planes
        info["n_kept"] = self.plane_keep(slot, 0, invert=True)["n_kept"]
        return self.select_kept_into(slot), info, planes

    def size(self, slot: int) -> int:
        return int(self._L.me_cloud_size(self._ctx, slot))

    def download(self, slot: int) -> np.ndarray:
        out = np.empty((self.size(slot), 3), np.float64)
        self._ck(self._L.me_download_cloud(self._ctx, slot, _addr(out)))
        return out

    # ---- 1-NN + AC/COM/CD ----
    def nn1(self, query_slot: int, ref_slot: int, fetch: bool = True):
        n = self.size(query_slot)
        if not fetch:
            self._ck(self._L.me_nn1(self._ctx, query_slot, ref_slot, 0, 0))
            return None, None
        idx = np.empty(n, np.int32)
        d2 = np.empty(n, np.float64)
        self._ck(self._L.me_nn1(self._ctx, query_slot, ref_slot, _addr(idx), _addr(d2)))
        return idx, d2

    def nn_stats(self, query_slot: int, gate: float, gate_mode: int, trunc) -> RegStats:
        tr = np.ascontiguousarray(trunc, dtype=np.float64)
        out = _lib.NNStatsOut()
        self._ck(self._L.me_nn_stats(self._ctx, query_slot, float(gate), int(gate_mode), _addr(tr), C.byref(out)))
        return RegStats.from_c(out)

    def nn_partial_sums(self, query_slot: int, gate: float, gate_mode: int, trunc) -> _lib.NNPartial:
        tr = np.ascontiguousarray(trunc, dtype=np.float64)
        out = _lib.NNPartial()
        self._ck(self._L.me_nn_partial_sums(self._ctx, query_slot, float(gate), int(gate_mode), _addr(tr), C.byref(out)))
        return out

    def nn_sigma_sums(self, query_slot: int, gate: float, gate_mode: int, mean) -> np.ndarray:
        m = np.ascontiguousarray(mean, dtype=np.float64)
        out = np.zeros(5, np.float64)
        self._ck(self._L.me_nn_sigma_sums(self._ctx, query_slot, float(gate), int(gate_mode), _addr(m), _addr(out)))
        return out

    def nn_finalize(self, total: _lib.NNPartial, sigma_num, n_src_total: int) -> RegStats:
        s = np.ascontiguousarray(sigma_num, dtype=np.float64)
        out = _lib.NNStatsOut()
        self._L.me_nn_finalize(C.byref(total), _addr(s), int(n_src_total), C.byref(out))
        return RegStats.from_c(out)

    def icp_p2p_sums(self, query_slot: int, max_distance: float) -> _lib.IcpSums:
        """Sums of the point-to-point ICP step over the correspondences (d2 < max^2) of the last nn1(query_slot, ...)."""
        out = _lib.IcpSums()
        self._ck(self._L.me_icp_p2p_sums(self._ctx, query_slot, float(max_distance), C.byref(out)))
        return out

    def renderDistanceOnPointCloud(self, query_slot: int, dis: float, gate: float = -1.0, gate_mode: int = 0):
        """map_eval.cpp:586-607 for the last nn1(query_slot, ...) -> (rgb (N,3), inlier (N,) bool)."""
        n = self.size(query_slot)
        rgb = np.empty((n, 3), np.float64)
        inl = np.empty(n, np.uint8)
        self._ck(self._L.me_render_distance(self._ctx, query_slot, float(dis), float(gate), int(gate_mode), _addr(rgb), _addr(inl)))
        return rgb, inl.astype(bool)

    def ColorPointCloudByMME(self, slot: int):
        """map_eval.cpp:686-735 for the last mme(slot) -> (xyz_valid (M,3), rgb (M,3), min_abs, max_abs)."""
        m, mn, mx = C.c_int64(0), C.c_double(), C.c_double()
        self._ck(self._L.me_render_entropy(self._ctx, slot, 0, 0, 0, C.byref(m), C.byref(mn), C.byref(mx)))
        xyz = np.empty((m.value, 3), np.float64)
        rgb = np.empty((m.value, 3), np.float64)
        if m.value:
            self._ck(self._L.me_render_entropy(self._ctx, slot, _addr(xyz), _addr(rgb), m.value, C.byref(m), C.byref(mn), C.byref(mx)))
        return xyz, rgb, mn.value, mx.value

    def set_normals(self, slot: int, normals) -> None:
        """Normals that came with the cloud (N,3), caller's point order."""
        nrm = np.ascontiguousarray(normals, dtype=np.float64)
        if nrm.shape != (self.size(slot), 3):
            raise ValueError("normals must be (N,3) for the N points of the slot")
        self._ck(self._L.me_set_normals(self._ctx, slot, _addr(nrm)))

    def get_normals(self, slot: int) -> np.ndarray:
        out = np.empty((self.size(slot), 3), np.float64)
        self._ck(self._L.me_get_normals(self._ctx, slot, _addr(out)))
        return out

    def estimate_normals(self, slot: int, knn: int = 20, fetch: bool = True, with_neighbours: bool = False):
        """open3d EstimateNormals(KDTreeSearchParamKNN(knn)) -> normals (N,3) [, knn_idx (N,knn), knn_d2 (N,knn)]."""
        n = self.size(slot)
        nrm = np.empty((n, 3), np.float64) if fetch else None
        idx = np.empty((n, knn), np.int32) if with_neighbours else None
        d2 = np.empty((n, knn), np.float64) if with_neighbours else None
        self._ck(self._L.me_estimate_normals(self._ctx, slot, int(knn), _addr(nrm) if fetch else 0,
                                             _addr(idx) if with_neighbours else 0, _addr(d2) if with_neighbours else 0))
        return (nrm, idx, d2) if with_neighbours else nrm

    def gicp_covariances(self, slot: int, epsilon: float = 1e-3, fetch: bool = False):
        """open3d InitializePointCloudForGeneralizedICP -> (N,3,3) when fetch."""
        out = np.empty((self.size(slot), 9), np.float64) if fetch else None
        self._ck(self._L.me_gicp_covariances(self._ctx, slot, float(epsilon), _addr(out) if fetch else 0))
        return out.reshape(-1, 3, 3) if fetch else None

    def get_covariances(self, slot: int) -> np.ndarray:
        out = np.empty((self.size(slot), 9), np.float64)
        self._ck(self._L.me_get_covariances(self._ctx, slot, _addr(out)))
        return out.reshape(-1, 3, 3)

    def icp_lsq_sums(self, query_slot: int, mode: int, max_distance: float) -> _lib.IcpLsq:
        """J^T J, J^T r of one point-to-plane (mode 1) / generalized (mode 2) step over the last nn1(query_slot, ...)."""
        out = _lib.IcpLsq()
        self._ck(self._L.me_icp_lsq_sums(self._ctx, query_slot, int(mode), float(max_distance), C.byref(out)))
        return out

    def icp_lsq_sums_robust(self, query_slot: int, mode: int, max_distance: float, kernel, k: float = 1.0) -> _lib.IcpRobust:
        """me_icp_lsq_sums_robust: the step of icp_lsq_sums under a robust loss (Open3D RobustKernel [upstream]).  kernel: an ME_ROBUST_*
        id or one of "l2", "l1", "huber", "cauchy", "gm", "tukey"; k: the scale of Huber, Cauchy, GM and Tukey."""
        if isinstance(kernel, str):
            if kernel.lower() not in _lib.ROBUST_KERNELS:
                raise ValueError(f"unknown robust kernel {kernel!r}")
            kernel = _lib.ROBUST_KERNELS[kernel.lower()]
        out = _lib.IcpRobust()
        self._ck(self._L.me_icp_lsq_sums_robust(self._ctx, query_slot, int(mode), float(max_distance), int(kernel), float(k), C.byref(out)))
        return out

    def icp_information(self, query_slot: int, max_distance: float):
        """me_icp_information: Open3D GetInformationMatrixFromPointClouds over the last nn1(query_slot, ...) -> ((6,6), n_corr)."""
        info = np.zeros(36, np.float64)
        n = C.c_int64(0)
        self._ck(self._L.me_icp_information(self._ctx, query_slot, float(max_distance), _addr(info), C.byref(n)))
        return info.reshape(6, 6), n.value

    def performICPRegistration(self, max_distance: float, method: int = 0, kernel=None, kernel_scale=None, **criteria):
        """map_eval.cpp:1366-1394: registration_methods 0 point-to-point, 1 point-to-plane, 2 generalized ICP (see icp.py).
        kernel / kernel_scale: a robust loss for methods 1 and 2 (icp_lsq_sums_robust); point-to-point takes none, as upstream."""
        from . import icp
        if method == 0:
            if kernel is not None:
                raise ValueError("point-to-point ICP takes no robust kernel")
            return icp.icp_point_to_point(self, max_distance, **criteria)
        if kernel is not None:
            criteria = dict(criteria, kernel=kernel, kernel_scale=kernel_scale)
        if method == 1:
            return icp.icp_point_to_plane(self, max_distance, **criteria)
        if method == 2:
            return icp.icp_generalized(self, max_distance, **criteria)
        raise MapEvalError("Invalid registration type specified")  # (:1385-1387)

    def computeChamferDistance(self) -> float:
        """map_eval.cpp:1398-1431 on the uploaded pair."""
        cd = C.c_double()
        self._ck(self._L.me_chamfer(self._ctx, C.byref(cd)))
        return cd.value

    def calculateMetricsWithInitialMatrix(self, p: Param):
        """map_eval.cpp:1204-1260 (clouds already uploaded, est with initial_matrix_) -> (est_gt, gt_est, cd_vec)."""
        self.nn1(ME_SLOT_EST, ME_SLOT_GT, fetch=False)
        est_gt = self.nn_stats(ME_SLOT_EST, p.icp_max_distance_, ME_GATE_LE_UNSQUARED, p.trunc_dist_)
        self.nn1(ME_SLOT_GT, ME_SLOT_EST, fetch=False)
        gt_est = self.nn_stats(ME_SLOT_GT, p.icp_max_distance_, ME_GATE_LE_UNSQUARED, p.trunc_dist_)
        return est_gt, gt_est, est_gt.rmse + gt_est.rmse  # cd_vec (:1245)

    # ---- MME ----
    def mme(self, slot: int, radius: float, min_k: int, per_point: bool = True):
        """-> (mean, entropies[N] | None, valid[N] | None, n_valid, sum_H)."""
        n = self.size(slot)
        ent = np.zeros(n, np.float64) if per_point else None
        val = np.zeros(n, np.uint8) if per_point else None
        s = C.c_double()
        nv = C.c_int64()
        self._ck(self._L.me_mme(self._ctx, slot, float(radius), int(min_k), _addr(ent), _addr(val), C.byref(s), C.byref(nv)))
        mean = s.value / nv.value if nv.value > 0 else 0.0
        return mean, ent, val, nv.value, s.value

    def computeMME(self, p: Param):
        """map_eval.cpp:149-189 -> (mme_est, mme_gt)."""
        mme_est = self.mme(ME_SLOT_EST, p.nn_radius_, 10, per_point=False)[0]
        mme_gt = self.mme(ME_SLOT_GT, p.nn_radius_, 5, per_point=False)[0] if p.evaluate_gt_mme_ else 0.0
        return mme_est, mme_gt

    # ---- MPV and the eigenvalue shape features (me_localgeom.hip) ----
    def local_geometry(self, slot: int, radius: float, min_k: int = 5, fetch: bool = False):
        """me_local_geometry: the eigenvalues l1 >= l2 >= l3 of every point's radius-neighbourhood covariance.  Returns the info dict
        (n, n_valid, sum_k and the means over the valid points: mpv = mean l3, linearity, planarity, sphericity, surface_variation,
        mean_k; 0.0 when no point is valid, as MME's mean), and with fetch=True also (eig[N, 3], k[N], valid[N]) in cloud order."""
        o = _lib.LocalGeomOut()
        self._ck(self._L.me_local_geometry(self._ctx, int(slot), float(radius), int(min_k), C.byref(o)))
        nv = o.n_valid

        def mean(s):
            return s / nv if nv > 0 else 0.0

        info = {"n": o.n, "n_valid": nv, "sum_k": o.sum_k, "mpv": mean(o.sum_l3), "linearity": mean(o.sum_linearity),
                "planarity": mean(o.sum_planarity), "sphericity": mean(o.sum_sphericity),
                "surface_variation": mean(o.sum_surface_variation), "mean_k": mean(o.sum_k)}
        if not fetch:
            return info
        return (info, *self.local_geometry_fetch(slot))

    def local_geometry_fetch(self, slot: int):
        """me_local_geometry_fetch -> (eig[N, 3], k[N], valid[N]) of the slot's last local_geometry / radius_normals, cloud order."""
        self._ck(self._L.me_local_geometry_fetch(self._ctx, int(slot), 0, 0, 0))  # (raises without a current result, before the size is asked)
        n = self.size(slot)
        eig = np.empty((n, 3), np.float64)
        k = np.empty(n, np.int32)
        valid = np.empty(n, np.uint8)
        self._ck(self._L.me_local_geometry_fetch(self._ctx, int(slot), _addr(eig), _addr(k), _addr(valid)))
        return eig, k, valid

    def mpv(self, slot: int, radius: float, min_k: int = 5) -> float:
        """Mean plane variance: the mean smallest covariance eigenvalue over the valid points (0.0 without one)."""
        return self.local_geometry(slot, radius, min_k)["mpv"]

    # ---- MOM: plane variance on mutually orthogonal planes, exact medians (me_mom.hip) ----
    def group_order_stats(self, values, groups, n_groups: int) -> dict:
        """me_group_order_stats: per group g in [0, n_groups) of the entries with groups[i] == g (-1 = ignored): count, sum, min, max
        and the two middle elements lower = sorted[(count - 1) // 2], upper = sorted[count // 2], all but the sum exact; median =
        (lower + upper) / 2.  Returns a dict of arrays of n_groups entries."""
        values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        groups = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        if values.shape != groups.shape:
            raise ValueError("values and groups differ in length")
        out = (_lib.GroupStats * max(1, min(int(n_groups), 64)))()
        self._ck(self._L.me_group_order_stats(self._ctx, _addr(values), _addr(groups), int(values.shape[0]), int(n_groups), C.addressof(out)))
        res = {f: np.array([getattr(out[g], f) for g in range(int(n_groups))], np.int64 if f == "count" else np.float64)
               for f, _ in _lib.GroupStats._fields_}
        res["median"] = (res["lower"] + res["upper"]) / 2
        return res

    @staticmethod
    def _mom_params(parallel_deg: float, orthogonal_deg: float, min_axis_points: int) -> _lib.MomParams:
        # planes within parallel_deg of each other share a direction; directions within orthogonal_deg of a right angle are orthogonal
        # (math, not numpy: the C library's cos / sin, which the C++ host calls too)
        return _lib.MomParams(math.cos(float(parallel_deg) * (math.pi / 180.0)), math.sin(float(orthogonal_deg) * (math.pi / 180.0)),
                              int(min_axis_points))

    @staticmethod
    def mom_select_axes(planes, parallel_deg: float = 10.0, orthogonal_deg: float = 10.0, min_axis_points: int = 1000, *,
                        cos_parallel: float | None = None, cos_orthogonal: float | None = None):
        """me_mom_select_axes (host arithmetic, no device): planes = the dicts of segment_planes (their "plane" and "count").  The
        thresholds are given in degrees, or directly as the cosines the library takes.  Returns (dir_of_plane [n_planes] int32, axes) —
        axes = {"n_axes", "n_directions", "axes": [{"direction", "n_planes", "weight", "rep"}, ...]}."""
        L = _lib.load()
        prm = Engine._mom_params(parallel_deg, orthogonal_deg, min_axis_points)
        if cos_parallel is not None:
            prm.cos_parallel = float(cos_parallel)
        if cos_orthogonal is not None:
            prm.cos_orthogonal = float(cos_orthogonal)
        n = len(planes)
        recs = (_lib.PlaneRecord * max(1, n))()
        for r, pl in enumerate(planes[:len(recs)]):
            recs[r].count = int(pl["count"])
            for e in range(4):
                recs[r].plane[e] = float(pl["plane"][e]) if e < len(pl["plane"]) else 0.0
        dirs = np.full(max(1, n), -1, np.int32)
        ax = _lib.MomAxes()
        rc = L.me_mom_select_axes(C.addressof(recs), n, C.byref(prm), _addr(dirs), C.byref(ax))
        if rc != 0:
            raise MapEvalError(f"[{rc}] me_mom_select_axes: needs 0 <= cos_orthogonal < cos_parallel <= 1, min_axis_points >= 1 and at most 64 planes")
        axes = [{"direction": int(a.direction), "n_planes": int(a.n_planes), "weight": int(a.weight), "rep": np.array(list(a.rep))}
                for a in list(ax.axis)[:ax.n_axes]]
        return dirs[:n], {"n_axes": int(ax.n_axes), "n_directions": int(ax.n_directions), "axes": axes}

    def _has_result(self, rc: int) -> bool:
        if rc == _lib.ME_ERR_STATE:
            return False
        self._ck(rc)
        return True

    def mom(self, slot: int, radius: float | None = None, min_k: int = 5, parallel_deg: float = 10.0, orthogonal_deg: float = 10.0,
            min_axis_points: int = 1000, plane_kwargs: dict | None = None, fetch: bool = False):
        """me_mom: the mutually orthogonal metric of a resident cloud, from the slot's local_geometry eigenvalues and segment_planes
        labels.  A stage whose result the slot lacks is run first when its arguments are given (radius and min_k; plane_kwargs = the
        keyword arguments of segment_planes); a current result is never recomputed.  Returns a dict: n_axes, n_directions, mom_median
        (the sum of the axis medians), mom_mean, axes = one dict per axis (direction, n_planes, rep, n_points, n_valid, sum_l3, min,
        max, lower, upper, median); with fetch=True also the axis byte per point ([N] int8 in cloud order, -1 = not used)."""
        if radius is not None and not self._has_result(self._L.me_local_geometry_fetch(self._ctx, int(slot), 0, 0, 0)):
            self.local_geometry(slot, radius, min_k)
        if plane_kwargs is not None:
            m = C.c_int64(0)
            if not self._has_result(self._L.me_plane_fetch(self._ctx, int(slot), 0, 0, C.byref(m), 0)):
                self.segment_planes(slot, **plane_kwargs)
        prm = self._mom_params(parallel_deg, orthogonal_deg, min_axis_points)
        o = _lib.MomOut()
        self._ck(self._L.me_mom(self._ctx, int(slot), C.byref(prm), C.byref(o)))
        axes = []
        for a in list(o.axis)[:o.n_axes]:
            d = {f: getattr(a, f) for f, _ in a._fields_ if f != "rep"}
            d["rep"] = np.array(list(a.rep))
            axes.append(d)
        res = {"n_axes": int(o.n_axes), "n_directions": int(o.n_directions), "mom_median": o.mom_median, "mom_mean": o.mom_mean, "axes": axes}
        return (res, self.mom_fetch(slot)) if fetch else res

    def mom_fetch(self, slot: int) -> np.ndarray:
        """me_mom_fetch -> the axis byte per point ([N] int8, cloud order, -1 = not used) of the slot's last mom."""
        self._ck(self._L.me_mom_fetch(self._ctx, int(slot), 0))  # (raises without a current result, before the size is asked)
        axis = np.empty(self.size(slot), np.int8)
        self._ck(self._L.me_mom_fetch(self._ctx, int(slot), _addr(axis)))
        return axis

    # ---- error distribution: exact quantiles, Hausdorff distance, F-score, error CDF (me_errdist.hip) ----
    def rank_select(self, values, ranks, use=None) -> dict:
        """me_rank_select: of the entries with use[i] != 0 (None: all): count, sum, min, max and value[j] = sorted_used[ranks[j]] (0-based
        ranks, unsorted and repeated ones allowed, at most 16), all but the sum exact.  Returns a dict; "value" has len(ranks) entries."""
        values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        if use is not None:
            use = np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8).reshape(-1)
            if use.shape != values.shape:
                raise ValueError("values and use differ in length")
        o = _lib.RankStats()
        self._ck(self._L.me_rank_select(self._ctx, _addr(values), _addr(use), int(values.shape[0]), _addr(ranks), int(ranks.shape[0]), C.byref(o)))
        return {"count": int(o.count), "sum": o.sum, "min": o.min, "max": o.max,
                "value": np.array(list(o.value)[:min(int(ranks.shape[0]), _lib.ME_RANK_MAX)], np.float64)}

    @staticmethod
    def sqrt_threshold(t: float) -> float:
        """me_sqrt_threshold: the largest double whose correctly rounded sqrt is <= t (host arithmetic)."""
        return float(_lib.load().me_sqrt_threshold(float(t)))

    @staticmethod
    def fscore(n_within_est: int, n_est: int, n_within_gt: int, n_gt: int):
        """me_fscore_finalize (host arithmetic): (precision, recall, fscore)."""
        prf = (C.c_double * 3)()
        _lib.load().me_fscore_finalize(int(n_within_est), int(n_est), int(n_within_gt), int(n_gt), C.byref(prf))
        return prf[0], prf[1], prf[2]

    def nn_error_distribution(self, query_slot: int, quantiles=(0.5, 0.9, 0.95, 0.99), thresholds=(), bins: int = 0, bin_width: float = 0.0,
                              gate: float = -1.0, gate_mode: int = ME_GATE_LE_UNSQUARED) -> dict:
        """me_nn_error_distribution on the current 1-NN result of query_slot: n_query, n_used, sum_d, sum_d2, min_d, max_d (the
        one-sided Hausdorff distance), argmax (original index of the worst query), per quantile rank / quantile_d / quantile_d2
        (nearest rank, exact), per threshold n_within, and with bins > 0 hist[bins] (counts between the edges j * bin_width) and
        n_overflow.  gate < 0: every query."""
        quantiles = [float(x) for x in quantiles]
        thresholds = [float(x) for x in thresholds]
        if len(quantiles) > _lib.ME_RANK_MAX or len(thresholds) > _lib.ME_ERRDIST_MAX_THRESHOLDS:
            raise MapEvalError("[-1] nn_error_distribution: at most 16 quantiles and 8 thresholds")
        p = _lib.ErrDistParams()
        p.gate, p.gate_mode = float(gate), int(gate_mode)
        p.n_quantiles, p.n_thresholds = len(quantiles), len(thresholds)
        for j, x in enumerate(quantiles):
            p.prob[j] = x
        for k, x in enumerate(thresholds):
            p.tau[k] = x
        p.n_bins, p.bin_width = int(bins), float(bin_width)
        hist = np.zeros(max(0, min(int(bins), _lib.ME_ERRDIST_MAX_BINS)), np.int64)
        o = _lib.ErrDistOut()
        self._ck(self._L.me_nn_error_distribution(self._ctx, int(query_slot), C.byref(p), C.byref(o), _addr(hist) if hist.size else 0))
        nq, nt = len(quantiles), len(thresholds)
        return {"n_query": int(o.n_query), "n_used": int(o.n_used), "sum_d": o.sum_d, "sum_d2": o.sum_d2, "min_d": o.min_d, "max_d": o.max_d,
                "argmax": int(o.argmax), "prob": np.array(quantiles, np.float64), "rank": np.array(list(o.rank)[:nq], np.int64),
                "quantile_d": np.array(list(o.quantile_d)[:nq], np.float64), "quantile_d2": np.array(list(o.quantile_d2)[:nq], np.float64),
                "tau": np.array(thresholds, np.float64), "n_within": np.array(list(o.n_within)[:nt], np.int64), "hist": hist,
                "n_overflow": int(o.n_overflow), "bin_width": float(bin_width)}

    def error_report(self, thresholds, quantiles=(0.5, 0.9, 0.95, 0.99), bins: int = 0, bin_width: float = 0.0, gate: float = -1.0,
                     gate_mode: int = ME_GATE_LE_UNSQUARED) -> dict:
        """Both directions from the resident 1-NN results of slots 0 and 1: "est" / "gt" = nn_error_distribution of each, hausdorff =
        max(max_d_est, max_d_gt), and per threshold precision (est points within tau of the ground truth / used est points), recall
        (the same from the ground truth's side) and fscore through me_fscore_finalize."""
        est = self.nn_error_distribution(ME_SLOT_EST, quantiles, thresholds, bins, bin_width, gate, gate_mode)
        gt = self.nn_error_distribution(ME_SLOT_GT, quantiles, thresholds, bins, bin_width, gate, gate_mode)
        prf = np.array([self.fscore(est["n_within"][k], est["n_used"], gt["n_within"][k], gt["n_used"]) for k in range(len(est["tau"]))],
                       np.float64).reshape(-1, 3)
        return {"est": est, "gt": gt, "hausdorff": max(est["max_d"], gt["max_d"]), "tau": est["tau"], "precision": prf[:, 0],
                "recall": prf[:, 1], "fscore": prf[:, 2]}

    # ---- radius-search normals and the normal-aware map error (me_localgeom.hip, me_surface.hip) ----
    def radius_normals(self, slot: int, radius: float, min_k: int = 5, viewpoint=None, invalid_z: bool = False, fetch: bool = False):
        """me_radius_normals: the unit eigenvector of the smallest eigenvalue of every point's radius-neighbourhood covariance (the
        neighbourhood and arithmetic of local_geometry, whose per-point result the call stores too) as the slot's normals; turned
        towards `viewpoint` (3 values) when given; (0, 0, 0), or (0, 0, 1) with invalid_z, where the point is invalid.  Returns the
        info dict (n, n_valid, sum_k, mean_k), and with fetch=True also the normals (N,3) in cloud order.  The call may rebuild the
        slot's index and so discard the 1-NN results: normals first, then nn1."""
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(-1)
        if vp is not None and vp.shape != (3,):
            raise ValueError("viewpoint must hold 3 values")
        o = _lib.RadiusNormalsOut()
        self._ck(self._L.me_radius_normals(self._ctx, int(slot), float(radius), int(min_k), _addr(vp), 1 if invalid_z else 0, C.byref(o)))
        info = {"n": int(o.n), "n_valid": int(o.n_valid), "sum_k": int(o.sum_k), "mean_k": o.sum_k / o.n_valid if o.n_valid > 0 else 0.0}
        return (info, self.get_normals(slot)) if fetch else info

    def nn_surface_error(self, query_slot: int, plane_thresholds=(), angle_thresholds_deg=(), gate: float = -1.0,
                         gate_mode: int = ME_GATE_LE_UNSQUARED, fetch: bool = False):
        """me_nn_surface_error on the current 1-NN result of query_slot, with the reference slot's normals (and the query's, when it
        has them): n_query, n_used, n_normal_used, sum_e, sum_e2, sum_t2, sum_c, max_e, argmax, per plane threshold n_within /
        sum_e2_within (e <= tau), per angle threshold n_angle (c >= cos_min; the cosine of the angle is taken here with math.cos).
        With fetch=True also (plane_d[N], cos_n[N]) in cloud order, -1 where the pair was not used."""
        taus = [float(x) for x in plane_thresholds]
        angs = [float(x) for x in angle_thresholds_deg]
        if len(taus) > _lib.ME_ERRDIST_MAX_THRESHOLDS or len(angs) > _lib.ME_SURFACE_MAX_ANGLES:
            raise MapEvalError("[-1] nn_surface_error: at most 8 plane thresholds and 8 angle thresholds")
        p = _lib.SurfaceParams()
        p.gate, p.gate_mode = float(gate), int(gate_mode)
        p.n_thresholds, p.n_angles = len(taus), len(angs)
        cos_min = [math.cos(a * (math.pi / 180.0)) for a in angs]
        for k, x in enumerate(taus):
            p.tau[k] = x
        for k, x in enumerate(cos_min):
            p.cos_min[k] = x
        o = _lib.SurfaceOut()
        self._ck(self._L.me_nn_surface_error(self._ctx, int(query_slot), C.byref(p), C.byref(o)))
        nt, na = len(taus), len(angs)
        res = {"n_query": int(o.n_query), "n_used": int(o.n_used), "n_normal_used": int(o.n_normal_used), "sum_e": o.sum_e,
               "sum_e2": o.sum_e2, "sum_t2": o.sum_t2, "sum_c": o.sum_c, "max_e": o.max_e, "argmax": int(o.argmax),
               "tau": np.array(taus, np.float64), "n_within": np.array(list(o.n_within)[:nt], np.int64),
               "sum_e2_within": np.array(list(o.sum_e2_within)[:nt], np.float64), "angle_deg": np.array(angs, np.float64),
               "cos_min": np.array(cos_min, np.float64), "n_angle": np.array(list(o.n_angle)[:na], np.int64)}
        return (res, *self.nn_surface_fetch(query_slot)) if fetch else res

    def nn_surface_fetch(self, query_slot: int):
        """me_nn_surface_fetch -> (plane_d[N], cos_n[N]) of the slot's last nn_surface_error, cloud order, -1 = pair not used."""
        n = self.size(query_slot)
        e = np.empty(n, np.float64)
        c = np.empty(n, np.float64)
        self._ck(self._L.me_nn_surface_fetch(self._ctx, int(query_slot), _addr(e), _addr(c)))
        return e, c

    def surface_report(self, plane_thresholds=(), angle_thresholds_deg=(5.0, 10.0, 20.0), quantiles=(), gate: float = -1.0,
                       gate_mode: int = ME_GATE_LE_UNSQUARED) -> dict:
        """Both directions from the resident 1-NN results of slots 0 and 1 (each slot needs the other's normals): "est" / "gt" =
        nn_surface_error of each plus mean_e, rms_e, mean_c, plane_rmse per threshold (sqrt(sum_e2_within / n_within), 0 without an
        inlier) and, for the quantiles given, rank / quantile_e (nearest rank, exact: rank_select on the fetched e with use = e >= 0);
        plane_chamfer = mean_e(est) + mean_e(gt)."""
        probs = [float(x) for x in quantiles]
        rep = {}
        for name, slot in (("est", ME_SLOT_EST), ("gt", ME_SLOT_GT)):
            d, e, _ = self.nn_surface_error(slot, plane_thresholds, angle_thresholds_deg, gate, gate_mode, fetch=True)
            nu, nn = d["n_used"], d["n_normal_used"]
            d["mean_e"] = d["sum_e"] / nu if nu > 0 else 0.0
            d["rms_e"] = math.sqrt(d["sum_e2"] / nu) if nu > 0 else 0.0
            d["mean_c"] = d["sum_c"] / nn if nn > 0 else 0.0
            d["plane_rmse"] = np.array([math.sqrt(s / m) if m > 0 else 0.0 for s, m in zip(d["sum_e2_within"], d["n_within"])], np.float64)
            d["prob"] = np.array(probs, np.float64)
            ranks = [min(nu - 1, max(0, int(math.ceil(pr * float(nu))) - 1)) if nu > 0 else -1 for pr in probs]
            d["rank"] = np.array(ranks, np.int64)
            if probs and nu > 0:
                d["quantile_e"] = self.rank_select(e, ranks, use=e >= 0)["value"]
            else:
                d["quantile_e"] = np.zeros(len(probs), np.float64)
            rep[name] = d
        rep["plane_chamfer"] = rep["est"]["mean_e"] + rep["gt"]["mean_e"]
        return rep

    # ---- M3C2: the signed distance between the two clouds along the query's normals (me_m3c2.hip) ----
    def m3c2(self, query_slot: int, projection_radius: float, max_depth: float, min_points: int = 5, reg_error: float = 0.0,
             core_mask=None, fetch: bool = False):
        """me_m3c2 with the points of query_slot (thinned by core_mask, (N,) of zero / non-zero, cloud order) as the core points, the
        slot's resident normals and the other slot as the compared cloud: per core point both clouds are averaged inside the cylinder
        of radius projection_radius and half-length max_depth along the normal; dist = mean_other - mean_own, lod = 1.96 *
        (sqrt(var_own / n_own + var_other / n_other) + reg_error).  Returns the totals (n_core, n_no_normal, n_valid, n_significant,
        sum_dist, sum_abs_dist, sum_dist2, sum_lod, sum_n_own, sum_n_other, max_abs_dist, argmax) with mean_dist, mean_abs_dist,
        rms_dist, mean_lod, mean_n_own, mean_n_other and significant_share over the valid points (0 without one); with fetch=True
        also the per-point dict of m3c2_fetch.  The call may re-index both slots and so discard the 1-NN and local-geometry results:
        normals first, then m3c2, then nn1."""
        n = self.size(query_slot)
        mask = None
        if core_mask is not None:
            mask = np.ascontiguousarray(np.asarray(core_mask) != 0, dtype=np.uint8).reshape(-1)
            if mask.shape != (n,):
                raise ValueError("core_mask must hold one entry per point of the query slot")
        p = _lib.M3c2Params()
        p.projection_radius, p.max_depth, p.reg_error, p.min_points = float(projection_radius), float(max_depth), float(reg_error), int(min_points)
        o = _lib.M3c2Out()
        self._ck(self._L.me_m3c2(self._ctx, int(query_slot), C.byref(p), _addr(mask), C.byref(o)))
        nv = int(o.n_valid)
        res = {"n_core": int(o.n_core), "n_no_normal": int(o.n_no_normal), "n_valid": nv, "n_significant": int(o.n_significant),
               "sum_dist": o.sum_dist, "sum_abs_dist": o.sum_abs_dist, "sum_dist2": o.sum_dist2, "sum_lod": o.sum_lod,
               "sum_n_own": int(o.sum_n_own), "sum_n_other": int(o.sum_n_other), "max_abs_dist": o.max_abs_dist, "argmax": int(o.argmax)}
        mean = (lambda v: v / nv) if nv > 0 else (lambda v: 0.0)
        res.update(mean_dist=mean(o.sum_dist), mean_abs_dist=mean(o.sum_abs_dist), rms_dist=math.sqrt(mean(o.sum_dist2)),
                   mean_lod=mean(o.sum_lod), mean_n_own=mean(o.sum_n_own), mean_n_other=mean(o.sum_n_other),
                   significant_share=mean(o.n_significant))
        return (res, self.m3c2_fetch(query_slot)) if fetch else res

    def m3c2_fetch(self, query_slot: int) -> dict:
        """me_m3c2_fetch -> dict of the slot's last m3c2 in cloud order: dist, lod, var_own, var_other (float64), n_own, n_other
        (int32), valid, significant (bool)."""
        n = self.size(query_slot)
        d = {k: np.empty(n, np.float64) for k in ("dist", "lod", "var_own", "var_other")}
        d["n_own"] = np.empty(n, np.int32)
        d["n_other"] = np.empty(n, np.int32)
        fl = np.empty(n, np.uint8)
        self._ck(self._L.me_m3c2_fetch(self._ctx, int(query_slot), _addr(d["dist"]), _addr(d["lod"]), _addr(d["var_own"]),
                                       _addr(d["var_other"]), _addr(d["n_own"]), _addr(d["n_other"]), _addr(fl)))
        d["valid"] = (fl & 1) != 0
        d["significant"] = (fl & 2) != 0
        return d

    # ---- consistent normal orientation: one sign propagated over the k-NN graph (me_orient.hip) ----
    def orient_normals(self, slot: int, k: int = 12, direction=(0.0, 0.0, 1.0), inward: bool = False, fetch: bool = False) -> dict:
        """me_orient_normals: the resident normals of the slot made consistent by carrying one sign along the minimum spanning forest
        of the k-NN graph weighted by 1 - |n_i . n_j| (Hoppe et al. 1992; Open3D's orient_normals_consistent_tangent_plane without its
        Delaunay edges: every component of the k-NN graph has a root of its own).  Per component the root is the extreme point along
        `direction` and is turned towards it (inward=True: against it).  The normals are replaced in place (get_normals); returns n,
        n_valid, n_components, largest_component, n_tree_edges, n_graph_edges, n_flipped, n_inconsistent_edges and, with fetch=True,
        component (int32[N], -1 for a point whose normal is the zero vector) and flipped (bool[N])."""
        d = np.asarray(direction, dtype=np.float64).reshape(-1)
        if d.shape[0] != 3:
            raise ValueError("direction must have 3 components")
        p = _lib.OrientParams()
        p.direction[0], p.direction[1], p.direction[2] = float(d[0]), float(d[1]), float(d[2])
        p.k, p.inward = int(k), 1 if inward else 0
        o = _lib.OrientOut()
        self._ck(self._L.me_orient_normals(self._ctx, int(slot), C.byref(p), C.byref(o)))
        res = {name: int(getattr(o, name)) for name, _ in _lib.OrientOut._fields_}
        if fetch:
            res.update(self.orient_fetch(slot))
        return res

    def orient_fetch(self, slot: int) -> dict:
        """me_orient_fetch: component (int32[N]) and flipped (bool[N]) of the slot's last orient_normals, in cloud order."""
        self._ck(self._L.me_orient_fetch(self._ctx, int(slot), None, None))  # (raises without a current result, before the size is asked)
        n = self.size(slot)
        comp = np.empty(n, np.int32)
        fl = np.empty(n, np.uint8)
        self._ck(self._L.me_orient_fetch(self._ctx, int(slot), _addr(comp), _addr(fl)))
        return {"component": comp, "flipped": fl != 0}

    # ---- surface reconstruction: IMLS field on a sparse voxel lattice + marching tetrahedra (me_recon.hip) ----
    @staticmethod
    def _recon_counts(o) -> dict:
        return {k: int(getattr(o, k)) for k, _ in _lib.ReconOut._fields_}

    def _recon_fetch(self, counts: dict) -> dict:
        nv, nt = counts["n_vertices"], counts["n_triangles"]
        d = {"vertices": np.empty((nv, 3), np.float64), "vertex_edge": np.empty((nv, 4), np.int32), "triangles": np.empty((nt, 3), np.int32)}
        self._ck(self._L.me_reconstruct_fetch(self._ctx, _addr(d["vertices"]), _addr(d["vertex_edge"]), _addr(d["triangles"])))
        return d

    def reconstruct(self, slot: int, voxel: float, radius=None, min_k: int = 8, band: int = 1, fetch: bool = True, install: bool = False,
                    orient_k=None):
        """me_reconstruct: the IMLS signed-distance field of the slot's points and resident normals (outward; orienting them is the
        caller's job: a viewpoint for radius_normals on a star-shaped scene, else orient_normals, which orient_k=<k> runs first with
        its defaults) on the nodes of the voxel lattice within `band` cells of the points, radius defaulting to 3 * voxel, and its
        zero set by marching tetrahedra.  Returns the counts (n_occupied_cells, n_active_cells, n_nodes, n_valid_nodes,
        n_cells_extracted, n_vertices, n_triangles, n_degenerate, sum_k) and, with fetch=True, vertices (V,3), vertex_edge (V,4) =
        (i, j, k, dir) and triangles (T,3) in the same dict; install=True makes the result the resident mesh (mesh_distance).  The call
        may re-index the slot and so discard the 1-NN, local-geometry, M3C2 and mesh-distance results: normals first, then
        reconstruct, then nn1."""
        if orient_k is not None:
            self.orient_normals(slot, int(orient_k))
        p = _lib.ReconParams()
        p.voxel, p.radius = float(voxel), float(3.0 * voxel if radius is None else radius)
        p.min_k, p.band = int(min_k), int(band)
        o = _lib.ReconOut()
        self._ck(self._L.me_reconstruct(self._ctx, int(slot), C.byref(p), C.byref(o)))
        res = self._recon_counts(o)
        self._shared["recon_n_nodes"] = res["n_nodes"]
        if fetch:
            res.update(self._recon_fetch(res))
        if install:
            self.reconstruct_install()
        return res

    def reconstruct_nodes(self) -> dict:
        """me_reconstruct_nodes_fetch: node_ijk (n,3) int32 in the Morton order of the lattice frame, f, k (int32), valid (bool) of the
        last reconstruct."""
        self._ck(self._L.me_reconstruct_nodes_fetch(self._ctx, None, None, None, None))  # (raises without a node field)
        n = int(self._shared["recon_n_nodes"])  # (of the context's last reconstruct, whichever lane ran it)
        d = {"node_ijk": np.empty((n, 3), np.int32), "f": np.empty(n, np.float64), "k": np.empty(n, np.int32)}
        v = np.empty(n, np.uint8)
        self._ck(self._L.me_reconstruct_nodes_fetch(self._ctx, _addr(d["node_ijk"]), _addr(d["f"]), _addr(d["k"]), _addr(v)))
        d["valid"] = v != 0
        return d

    def isosurface(self, node_ijk, f, valid, voxel: float) -> dict:
        """me_isosurface: marching tetrahedra of a sparse lattice field the caller supplies: node_ijk (n,3) int32, f (n,), valid (n,)
        of zero / non-zero; a cell is extracted iff all 8 corners are present and valid.  Returns the counts and the three arrays."""
        ijk = np.ascontiguousarray(node_ijk, dtype=np.int32).reshape(-1, 3)
        fv = np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
        ok = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8).reshape(-1)
        if fv.shape[0] != ijk.shape[0] or ok.shape[0] != ijk.shape[0]:
            raise ValueError("node_ijk, f and valid must have one entry per node")
        o = _lib.ReconOut()
        self._ck(self._L.me_isosurface(self._ctx, _addr(ijk), _addr(fv), _addr(ok), int(ijk.shape[0]), float(voxel), C.byref(o)))
        res = self._recon_counts(o)
        res.update(self._recon_fetch(res))
        return res

    def reconstruct_install(self):
        """me_reconstruct_install: the last reconstruction becomes the resident mesh, as mesh_upload of the fetched arrays would."""
        self._ck(self._L.me_reconstruct_install(self._ctx))

    # ---- cloud-to-mesh distance against a resident triangle mesh, and its area-uniform sample (me_mesh.hip) ----
    def mesh_upload(self, vertices, triangles, T=None):
        """me_mesh_upload: vertices (V,3) float64, triangles (F,3) int32 indices into them, T an optional 4x4 applied as upload() applies
        it.  The mesh stays resident beside the two clouds until the next mesh_upload or mesh_clear."""
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        t = np.ascontiguousarray(triangles, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("expected (V,3) vertices and (F,3) triangles")
        Tm = None if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        self._ck(self._L.me_mesh_upload(self._ctx, _addr(v), int(v.shape[0]), _addr(t), int(t.shape[0]), _addr(Tm)))

    def mesh_clear(self):
        self._ck(self._L.me_mesh_clear(self._ctx))

    def mesh_info(self) -> dict:
        """me_mesh_info: vertices, triangles, degenerate, depth (tree levels), bbox_lo / bbox_hi of the referenced vertices, area."""
        o = _lib.MeshInfoOut()
        self._ck(self._L.me_mesh_info(self._ctx, C.byref(o)))
        return {"vertices": int(o.n_vertices), "triangles": int(o.n_triangles), "degenerate": int(o.n_degenerate), "depth": int(o.depth),
                "bbox_lo": np.array(list(o.bbox_lo), np.float64), "bbox_hi": np.array(list(o.bbox_hi), np.float64), "area": o.area}

    def mesh_distance(self, query_slot: int, max_distance: float = math.inf, thresholds=(), fetch: bool = False):
        """me_mesh_distance: the exact distance from every point of query_slot to the resident mesh.  A point is matched iff
        d2 <= max_distance^2 (inf: every point).  Returns the totals (n_query, n_matched, n_face, sum_d, sum_d2, sum_signed,
        sum_abs_signed) with mean, rmse, max, worst_index, n_within per threshold, face_share and, over the matched points whose closest
        point lies inside a face, signed_mean and signed_mean_abs (the sign is not defined at edges and vertices); zeros without a
        matched point.  With fetch=True also the per-point dict of mesh_distance_fetch."""
        ths = [float(x) for x in thresholds]
        if len(ths) > _lib.ME_MESH_MAX_THRESHOLDS:
            raise MapEvalError("[-1] mesh_distance: at most 8 thresholds")
        p = _lib.MeshParams()
        p.max_distance, p.n_thresholds = float(max_distance), len(ths)
        for k, x in enumerate(ths):
            p.thresholds[k] = x
        o = _lib.MeshOut()
        self._ck(self._L.me_mesh_distance(self._ctx, int(query_slot), C.byref(p), C.byref(o)))
        nm, nf = int(o.n_matched), int(o.n_face)
        res = {"n_query": int(o.n_query), "n_matched": nm, "n_face": nf, "sum_d": o.sum_d, "sum_d2": o.sum_d2, "sum_signed": o.sum_signed,
               "sum_abs_signed": o.sum_abs_signed, "mean": o.sum_d / nm if nm > 0 else 0.0, "rmse": math.sqrt(o.sum_d2 / nm) if nm > 0 else 0.0,
               "max": o.max_d, "worst_index": int(o.argmax), "thresholds": np.array(ths, np.float64),
               "n_within": np.array(list(o.n_within)[:len(ths)], np.int64), "face_share": nf / nm if nm > 0 else 0.0,
               "signed_mean": o.sum_signed / nf if nf > 0 else 0.0, "signed_mean_abs": o.sum_abs_signed / nf if nf > 0 else 0.0}
        return (res, self.mesh_distance_fetch(query_slot)) if fetch else res

    def mesh_distance_fetch(self, query_slot: int) -> dict:
        """me_mesh_distance_fetch -> dict of the slot's last mesh_distance in cloud order: d2 (float64), tri (int32, the caller's triangle
        index), region (uint8: 0 face, 1-3 edges AB BC CA, 4-6 vertices A B C), closest (N,3), signed_d (NaN outside the face region)."""
        n = self.size(query_slot)
        d = {"d2": np.empty(n, np.float64), "tri": np.empty(n, np.int32), "region": np.empty(n, np.uint8),
             "closest": np.empty((n, 3), np.float64), "signed_d": np.empty(n, np.float64)}
        self._ck(self._L.me_mesh_distance_fetch(self._ctx, int(query_slot), _addr(d["d2"]), _addr(d["tri"]), _addr(d["region"]),
                                                _addr(d["closest"]), _addr(d["signed_d"])))
        return d

    def mesh_sample(self, dst_slot: int, n_points: int, seed: int = 0) -> int:
        """me_mesh_sample: n_points area-uniform, seeded samples of the resident mesh become the cloud of dst_slot."""
        self._ck(self._L.me_mesh_sample(self._ctx, int(dst_slot), int(n_points), int(seed) & ((1 << 64) - 1)))
        self._held.pop(dst_slot, None)
        return self.size(dst_slot)

    # ---- the sign of that distance at edges and vertices: connectivity, pseudo-normals, the sign pass (me_meshsign.hip) ----
    @staticmethod
    def mesh_weld(vertices, triangles):
        """Merge vertices of equal value (-0.0 == 0.0), keeping the first occurrence and the order of the kept ones -> (vertices,
        triangles, map) with map[i] the new index of old vertex i.  Plain numpy, for STL-style triangle soup: the topology identifies
        a vertex by its index, so unwelded soup is all boundary edges."""
        v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        if v.shape[0] == 0:
            return v.copy(), t.copy(), np.zeros(0, np.int64)
        _, first, inv = np.unique(v + 0.0, axis=0, return_index=True, return_inverse=True)  # (+ 0.0 turns -0.0 into +0.0)
        inv = np.asarray(inv).reshape(-1)
        keep = np.sort(first)  # first occurrences, in the caller's order
        new_of_group = np.empty(first.shape[0], np.int64)
        new_of_group[np.argsort(first, kind="stable")] = np.arange(first.shape[0])
        vmap = new_of_group[inv]
        return v[keep].copy(), vmap[t].astype(np.int32), vmap

    def mesh_topology(self, fetch: bool = False):
        """me_mesh_topology: the resident mesh's connectivity by the caller's vertex indices -> n_edges, n_boundary_edges,
        n_nonmanifold_edges, n_inconsistent_edges, n_zero_edges, n_zero_vertices, n_tainted_vertices, n_unreferenced_vertices, closed,
        oriented_manifold.  Built on first use and kept with the mesh.  With fetch=True also the dict of me_mesh_topology_fetch:
        vertex_normal (V,3), vertex_flags (V,), edge_normal (F,3,3) and edge_flags (F,3) per (triangle, local edge AB BC CA)."""
        o = _lib.MeshTopoOut()
        self._ck(self._L.me_mesh_topology(self._ctx, C.byref(o)))
        res = {k: int(getattr(o, k)) for k, _ in _lib.MeshTopoOut._fields_}
        res["closed"], res["oriented_manifold"] = bool(res["closed"]), bool(res["oriented_manifold"])
        if not fetch:
            return res
        info = self.mesh_info()
        nv, nt = info["vertices"], info["triangles"]
        d = {"vertex_normal": np.empty((nv, 3), np.float64), "vertex_flags": np.empty(nv, np.uint8),
             "edge_normal": np.empty((nt, 3, 3), np.float64), "edge_flags": np.empty((nt, 3), np.uint8)}
        self._ck(self._L.me_mesh_topology_fetch(self._ctx, _addr(d["vertex_normal"]), _addr(d["vertex_flags"]), _addr(d["edge_normal"]),
                                                _addr(d["edge_flags"])))
        return res, d

    def mesh_signed_distance(self, query_slot: int, max_distance: float = math.inf, fetch: bool = False):
        """me_mesh_signed_distance over the slot's current mesh_distance result: the sign from the face normal, the edge pseudo-normal
        or the angle-weighted vertex pseudo-normal of the feature the closest point lies on (signed_d > 0 outside).  Returns the totals
        over the matched points plus mean_signed, mean_abs (over the signed points), inside_share (inside / signed) and
        unreliable_share (unreliable / matched); zeros where the denominator is.  With fetch=True also the dict of mesh_signed_fetch."""
        p = _lib.MeshSignParams()
        p.max_distance = float(max_distance)
        o = _lib.MeshSignOut()
        self._ck(self._L.me_mesh_signed_distance(self._ctx, int(query_slot), C.byref(p), C.byref(o)))
        res = {k: int(getattr(o, k)) for k in ("n_query", "n_matched", "n_signed", "n_inside", "n_outside", "n_on", "n_unsigned",
                                                "n_unreliable", "argmin", "argmax")}
        res["n_by_region"] = np.array(list(o.n_by_region), np.int64)
        for k in ("sum_signed", "sum_abs_signed", "sum_signed2", "min_signed", "max_signed"):
            res[k] = float(getattr(o, k))
        ns, nm = res["n_signed"], res["n_matched"]
        res["mean_signed"] = o.sum_signed / ns if ns > 0 else 0.0
        res["mean_abs"] = o.sum_abs_signed / ns if ns > 0 else 0.0
        res["inside_share"] = res["n_inside"] / ns if ns > 0 else 0.0
        res["unreliable_share"] = res["n_unreliable"] / nm if nm > 0 else 0.0
        return (res, self.mesh_signed_fetch(query_slot)) if fetch else res

    def mesh_signed_fetch(self, query_slot: int) -> dict:
        """me_mesh_signed_fetch -> signed_d (float64, NaN where unsigned) and flags (uint8: 1 ON, 2 UNSIGNED, 4 UNRELIABLE), cloud order."""
        n = self.size(query_slot)
        d = {"signed_d": np.empty(n, np.float64), "flags": np.empty(n, np.uint8)}
        self._ck(self._L.me_mesh_signed_fetch(self._ctx, int(query_slot), _addr(d["signed_d"]), _addr(d["flags"])))
        return d

    def mesh_report(self, thresholds, quantiles=(0.5, 0.9, 0.95, 0.99), sample_points: int = 0, seed: int = 0,
                    max_distance: float = math.inf, signed: bool = False) -> dict:
        """The cloud-to-mesh figures of slot 0 (mesh_distance) plus prob / rank / quantile_d: exact nearest-rank quantiles of d over the
        matched points (rank_select on the fetched values).  With sample_points > 0 the mesh is then sampled into slot 1, nn1 runs both
        ways and "sampled" holds error_report(thresholds, quantiles): completeness (recall) and F-score per threshold."""
        rep, pts = self.mesh_distance(ME_SLOT_EST, max_distance, thresholds, fetch=True)
        d = np.sqrt(pts["d2"])
        nm = rep["n_matched"]
        probs = [float(x) for x in quantiles]
        ranks = [min(nm - 1, max(0, int(math.ceil(pr * float(nm))) - 1)) if nm > 0 else -1 for pr in probs]
        rep["prob"] = np.array(probs, np.float64)
        rep["rank"] = np.array(ranks, np.int64)
        if probs and nm > 0:
            rep["quantile_d"] = self.rank_select(d, ranks, use=pts["d2"] <= float(max_distance) * float(max_distance))["value"]
        else:
            rep["quantile_d"] = np.zeros(len(probs), np.float64)
        if signed:  # the sign everywhere (mesh_signed_distance) and exact nearest-rank quantiles of signed_d over the signed matched points
            srep, spts = self.mesh_signed_distance(ME_SLOT_EST, max_distance, fetch=True)
            srep["topology"] = self.mesh_topology()
            ns = srep["n_signed"]
            sranks = [min(ns - 1, max(0, int(math.ceil(pr * float(ns))) - 1)) if ns > 0 else -1 for pr in probs]
            srep["prob"], srep["rank"] = np.array(probs, np.float64), np.array(sranks, np.int64)
            if probs and ns > 0:
                # rank_select takes values >= 0: the ni negative ones come first in ascending order, by descending |s|
                sd = spts["signed_d"]
                use = (pts["d2"] <= float(max_distance) * float(max_distance)) & ~np.isnan(sd)
                neg = use & (sd < 0)
                ni = int(np.count_nonzero(neg))
                q = np.zeros(len(probs), np.float64)
                lo = [j for j, r in enumerate(sranks) if r < ni]
                hi = [j for j, r in enumerate(sranks) if r >= ni]
                if lo:
                    q[lo] = -self.rank_select(np.where(neg, -sd, 0.0), [ni - 1 - sranks[j] for j in lo], use=neg)["value"]
                if hi:
                    q[hi] = self.rank_select(np.where(use & ~neg, sd, 0.0), [sranks[j] - ni for j in hi], use=use & ~neg)["value"]
                srep["quantile_signed"] = q
            else:
                srep["quantile_signed"] = np.zeros(len(probs), np.float64)
            rep["signed"] = srep
        if sample_points > 0:
            self.mesh_sample(ME_SLOT_GT, sample_points, seed)
            self.nn1(ME_SLOT_EST, ME_SLOT_GT, fetch=False)
            self.nn1(ME_SLOT_GT, ME_SLOT_EST, fetch=False)
            rep["sampled"] = self.error_report(thresholds, quantiles)
        return rep

    # ---- rays against the resident mesh: casts, the simulated sensor, observability (me_ray.hip) ----
    def mesh_raycast(self, origins, directions, t_min: float = 0.0, t_max: float = math.inf, any_hit: bool = False) -> dict:
        """me_mesh_raycast: rays (origins[i], directions[i]) against the resident mesh, t in units of |direction| within [t_min, t_max].
        Returns per ray t (+inf on a miss), tri (the caller's triangle index, -1 on a miss), u, v (barycentric weights of B and C) and
        flags (RAY_HIT, RAY_BACKFACE, RAY_INVALID), plus the totals n_rays, n_hit, n_backface, n_invalid, min_t, max_t.  The closest hit
        is the smallest (t, triangle index); any_hit=True only answers whether a hit exists (flags; t, tri, u, v carry the miss values)."""
        o = np.ascontiguousarray(origins, dtype=np.float64)
        d = np.ascontiguousarray(directions, dtype=np.float64)
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError("expected (N,3) origins and directions of the same shape")
        n = int(o.shape[0])
        res = {"t": np.empty(n, np.float64), "tri": np.empty(n, np.int32), "u": np.empty(n, np.float64), "v": np.empty(n, np.float64),
               "flags": np.empty(n, np.uint8)}
        out = _lib.RayOut()
        self._ck(self._L.me_mesh_raycast(self._ctx, _addr(o), _addr(d), n, float(t_min), float(t_max),
                                         _lib.ME_RAY_ANY if any_hit else _lib.ME_RAY_CLOSEST, _addr(res["t"]), _addr(res["tri"]),
                                         _addr(res["u"]), _addr(res["v"]), _addr(res["flags"]), C.byref(out)))
        res.update({f: getattr(out, f) for f, _ in out._fields_})
        return res

    def mesh_scan(self, dst_slot: int, poses, directions, min_range: float = 0.0, max_range: float = math.inf, noise_std: float = 0.0,
                  seed: int = 0, fetch: bool = False) -> dict:
        """me_mesh_scan: a range sensor with the beam table `directions` (D,3, sensor frame) at every pose (M,4,4 sensor -> world) scans the
        resident mesh; the hits, in ray order (ray = pose * D + beam), become the cloud of dst_slot.  Returns n_rays, n_hit, n_backface,
        pose_hits (M,) and with fetch=True ray_id (int64 per point of the slot)."""
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)
        d = np.ascontiguousarray(directions, dtype=np.float64)
        if d.ndim != 2 or d.shape[1] != 3:
            raise ValueError("expected (D,3) directions")
        p = _lib.ScanParams()
        p.min_range, p.max_range, p.noise_std, p.seed = float(min_range), float(max_range), float(noise_std), int(seed) & ((1 << 64) - 1)
        out = _lib.ScanOut()
        hits = np.zeros(P.shape[0], np.int64)
        self._ck(self._L.me_mesh_scan(self._ctx, int(dst_slot), _addr(P), int(P.shape[0]), _addr(d), int(d.shape[0]), C.byref(p), _addr(hits),
                                      C.byref(out)))
        self._held.pop(int(dst_slot), None)
        res = {"n_rays": int(out.n_rays), "n_hit": int(out.n_hit), "n_backface": int(out.n_backface), "pose_hits": hits}
        if fetch:
            res["ray_id"] = self.mesh_scan_fetch(dst_slot) if res["n_hit"] > 0 else np.zeros(0, np.int64)
        return res

    def mesh_scan_fetch(self, slot: int) -> np.ndarray:
        """me_mesh_scan_fetch: the ray id of every point of a scanned slot, cloud order (pose = ray_id // D)."""
        ids = np.empty(self.size(slot), np.int64)
        self._ck(self._L.me_mesh_scan_fetch(self._ctx, int(slot), _addr(ids)))
        return ids

    def cloud_visibility(self, slot: int, origins, max_range: float = math.inf, min_range: float = 0.0, tolerance: float = 0.0,
                         first_only: bool = False, fetch: bool = False):
        """me_cloud_visibility: which points of the slot some origin (M,3) sees past the resident mesh — in range, and no triangle on the
        segment origin -> point short of `tolerance` metres before the point.  Returns n_points, n_visible, n_in_range, n_tests and
        visible_share; the slot's keep mask becomes "visible" (select_kept_into copies the observable points).  With fetch=True also
        the dict of visibility_fetch."""
        o = np.ascontiguousarray(origins, dtype=np.float64)
        if o.ndim != 2 or o.shape[1] != 3:
            raise ValueError("expected (M,3) origins")
        p = _lib.VisParams()
        p.min_range, p.max_range, p.tolerance, p.first_only = float(min_range), float(max_range), float(tolerance), 1 if first_only else 0
        out = _lib.VisOut()
        self._ck(self._L.me_cloud_visibility(self._ctx, int(slot), _addr(o), int(o.shape[0]), C.byref(p), C.byref(out)))
        res = {f: int(getattr(out, f)) for f, _ in out._fields_}
        res["visible_share"] = res["n_visible"] / res["n_points"] if res["n_points"] > 0 else 0.0
        return (res, self.visibility_fetch(slot)) if fetch else res

    def visibility_fetch(self, slot: int) -> dict:
        """me_cloud_visibility_fetch -> n_seen (int32, origins that see the point) and first_seen (int32, the first of them, -1), cloud order."""
        n = self.size(slot)
        d = {"n_seen": np.empty(n, np.int32), "first_seen": np.empty(n, np.int32)}
        self._ck(self._L.me_cloud_visibility_fetch(self._ctx, int(slot), _addr(d["n_seen"]), _addr(d["first_seen"])))
        return d

    def observable_report(self, origins, thresholds, tolerance: float = 0.05, max_range: float = math.inf, min_range: float = 0.0,
                          quantiles=(0.5, 0.9, 0.95, 0.99)) -> dict:
        """Completeness against the ground truth a sensor at `origins` could have seen.  In order: visibility of the ground-truth slot
        (first_only), its visible points into a private engine beside a copy of the map, nn1 both ways there and here, error_report
        on both.  Returns "all" (every ground-truth point), "observable" (the visible ones), "visibility" (the totals) and
        visible_share.  This engine's clouds are left as they were (their 1-NN results are renewed, the ground truth's keep mask is
        the visibility's)."""
        vis = self.cloud_visibility(ME_SLOT_GT, origins, max_range=max_range, min_range=min_range, tolerance=tolerance, first_only=True)
        self.nn1(ME_SLOT_EST, ME_SLOT_GT, fetch=False)
        self.nn1(ME_SLOT_GT, ME_SLOT_EST, fetch=False)
        rep_all = self.error_report(thresholds, quantiles)
        if vis["n_visible"] == 0:
            raise MapEvalError("[-3] observable_report: no ground-truth point is visible from the origins")
        with Engine(self.device) as priv:
            self.select_kept_into(ME_SLOT_GT, priv, ME_SLOT_GT)
            priv.upload(ME_SLOT_EST, self.download(ME_SLOT_EST))
            priv.nn1(ME_SLOT_EST, ME_SLOT_GT, fetch=False)
            priv.nn1(ME_SLOT_GT, ME_SLOT_EST, fetch=False)
            rep_obs = priv.error_report(thresholds, quantiles)
        return {"all": rep_all, "observable": rep_obs, "visibility": vis, "visible_share": vis["visible_share"]}

    # ---- neighbour lists between the resident clouds (me_search.hip) ----
    def _query_mask(self, query_slot: int, mask):
        if mask is None:
            return None
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1)
        if m.shape != (self.size(query_slot),):
            raise ValueError("mask must hold one entry per point of the query slot")
        return m

    def knn_search(self, query_slot: int, ref_slot: int, k: int, mask=None):
        """me_knn_search: the k nearest points of ref_slot for every point of query_slot (the slots may be equal) -> (idx[N, k] int32,
        d2[N, k] float64), rows ascending by (d2, index), -1 / inf where the reference cloud has fewer than k points or the query is
        masked out (mask: (N,) of zero / non-zero, cloud order).  Leaves everything resident on both slots as it is."""
        n = self.size(query_slot)
        m = self._query_mask(query_slot, mask)
        idx = np.empty((n, max(int(k), 0)), np.int32)
        d2 = np.empty((n, max(int(k), 0)), np.float64)
        self._ck(self._L.me_knn_search(self._ctx, int(query_slot), int(ref_slot), int(k), _addr(m), _addr(idx), _addr(d2)))
        return idx, d2

    def hybrid_search(self, query_slot: int, ref_slot: int, radius: float, max_nn: int, mask=None):
        """me_hybrid_search: the max_nn nearest among the points of ref_slot with d2 < radius^2 -> (counts[N] int32, idx[N, max_nn],
        d2[N, max_nn]), padded with -1 / inf past counts[i]."""
        n = self.size(query_slot)
        m = self._query_mask(query_slot, mask)
        cnt = np.empty(n, np.int32)
        idx = np.empty((n, max(int(max_nn), 0)), np.int32)
        d2 = np.empty((n, max(int(max_nn), 0)), np.float64)
        self._ck(self._L.me_hybrid_search(self._ctx, int(query_slot), int(ref_slot), float(radius), int(max_nn), _addr(m), _addr(cnt),
                                          _addr(idx), _addr(d2)))
        return cnt, idx, d2

    def radius_search(self, query_slot: int, ref_slot: int, radius: float, counts_only: bool = False, mask=None):
        """me_radius_search: every point of ref_slot with d2 < radius^2 (strict) per point of query_slot, as CSR -> (offsets int64[N + 1],
        idx int32[total], d2 float64[total]); row i is idx[offsets[i]:offsets[i + 1]], ascending by (d2, index).  The sizing call,
        the allocation and the filling call; counts_only=True returns the offsets alone."""
        n = self.size(query_slot)
        m = self._query_mask(query_slot, mask)
        off = np.empty(n + 1, np.int64)
        total = C.c_int64(0)
        self._ck(self._L.me_radius_search(self._ctx, int(query_slot), int(ref_slot), float(radius), _addr(m), _addr(off), 0, 0, 0,
                                          C.byref(total)))
        if counts_only:
            return off
        idx = np.empty(total.value, np.int32)
        d2 = np.empty(total.value, np.float64)
        if total.value > 0:
            self._ck(self._L.me_radius_search(self._ctx, int(query_slot), int(ref_slot), float(radius), _addr(m), _addr(off), _addr(idx),
                                              _addr(d2), total.value, C.byref(total)))
        return off, idx, d2

    def m3c2_report(self, normal_radius: float, projection_radius: float, max_depth: float, min_points: int = 5, reg_error: float = 0.0,
                    normal_min_points: int = 5, quantiles=(0.05, 0.5, 0.95), core_every: int = 1) -> dict:
        """radius_normals(normal_radius) on each slot in turn (the normals as Jacobi yields them: no viewpoint), then m3c2 in both
        directions: "est" / "gt" = the totals of m3c2 with that slot as the query, plus "normals" (the info of its radius_normals)
        and, for the quantiles given, rank / quantile_dist (nearest rank, exact: rank_select with use = valid, on the magnitudes of the
        negative distances and of the others in turn, since it orders non-negative keys).
        core_every = k > 1 keeps every k-th point of each cloud as a core point."""
        probs = [float(x) for x in quantiles]
        rep = {}
        infos = {slot: self.radius_normals(slot, normal_radius, normal_min_points) for slot in (ME_SLOT_EST, ME_SLOT_GT)}
        for name, slot in (("est", ME_SLOT_EST), ("gt", ME_SLOT_GT)):
            mask = None
            if int(core_every) > 1:
                mask = np.zeros(self.size(slot), np.uint8)
                mask[::int(core_every)] = 1
            d, pp = self.m3c2(slot, projection_radius, max_depth, min_points, reg_error, mask, fetch=True)
            nv = d["n_valid"]
            d["normals"] = infos[slot]
            d["prob"] = np.array(probs, np.float64)
            ranks = [min(nv - 1, max(0, int(math.ceil(pr * float(nv))) - 1)) if nv > 0 else -1 for pr in probs]
            d["rank"] = np.array(ranks, np.int64)
            if probs and nv > 0:
                # rank_select orders non-negative keys: the negative distances are selected by magnitude from their far end (the
                # k-th smallest of m negatives is minus the (m - 1 - k)-th smallest magnitude), the others directly
                dist, valid = pp["dist"], pp["valid"]
                neg = valid & (dist < 0)
                m = int(neg.sum())
                mag = np.abs(dist) + 0.0
                q = np.zeros(len(ranks), np.float64)
                lo = [j for j, r in enumerate(ranks) if r < m]
                hi = [j for j, r in enumerate(ranks) if r >= m]
                if lo:
                    q[lo] = -self.rank_select(mag, [m - 1 - ranks[j] for j in lo], use=neg)["value"]
                if hi:
                    q[hi] = self.rank_select(mag, [ranks[j] - m for j in hi], use=valid & ~neg)["value"]
                d["quantile_dist"] = q
            else:
                d["quantile_dist"] = np.zeros(len(probs), np.float64)
            rep[name] = d
        return rep

    # ---- voxels ----
    def voxel_build(self, slot: int, voxel_size: float) -> int:
        """Builds (and caches on the cloud) the voxel-Gaussian table without exporting it; returns the voxel count."""
        nv = C.c_int64(0)
        self._ck(self._L.me_voxel_gaussians(self._ctx, slot, float(voxel_size), 0, 0, 0, 0, 0, C.byref(nv)))
        return nv.value

    def voxel_gaussians(self, slot: int, voxel_size: float):
        nv = C.c_int64(0)
        self._ck(self._L.me_voxel_gaussians(self._ctx, slot, float(voxel_size), 0, 0, 0, 0, 0, C.byref(nv)))
        v = nv.value
        keys = np.empty((v, 3), np.int32)
        n = np.empty(v, np.int32)
        mu = np.empty((v, 3), np.float64)
        sg = np.empty((v, 9), np.float64)
        en = np.empty(v, np.float64)
        nv = C.c_int64(v)
        self._ck(self._L.me_voxel_gaussians(self._ctx, slot, float(voxel_size), _addr(keys), _addr(n), _addr(mu), _addr(sg),
                                            _addr(en), C.byref(nv)))
        return keys, n, mu, sg.reshape(v, 3, 3), en

    def voxel_metrics(self, slot: int, voxel_size: float, gate: float, gate_mode: int, trunc) -> dict:
        """me_voxel_metrics: the last me_nn1(slot, ..) statistics and the slot's last MME per voxel of the getVoxelIndex lattice
        (voxel_calculator.cpp:241-245), rows in ascending key order = the rows of voxel_gaussians(slot, voxel_size).
        -> dict(keys (V, 3) int32, n_query, n_corr, n_inl (V, 5), sum_d (V, 5), sum_d2 (V, 5), sum_sqrt_all, sum_H, n_H, have_mme)."""
        tr = np.ascontiguousarray(trunc, dtype=np.float64)
        nv, hm = C.c_int64(0), C.c_int(0)
        self._ck(self._L.me_voxel_metrics(self._ctx, slot, float(voxel_size), float(gate), int(gate_mode), _addr(tr), 0, 0, 0, 0,
                                          C.byref(hm), C.byref(nv)))
        v = nv.value
        keys = np.empty((v, 3), np.int32)
        nn = np.empty(v, _lib.NN_PARTIAL_DTYPE)
        sum_h = np.empty(v, np.float64)
        n_h = np.empty(v, np.int64)
        nv = C.c_int64(v)
        self._ck(self._L.me_voxel_metrics(self._ctx, slot, float(voxel_size), float(gate), int(gate_mode), _addr(tr), _addr(keys),
                                          _addr(nn), _addr(sum_h), _addr(n_h), C.byref(hm), C.byref(nv)))
        out = {f: np.ascontiguousarray(nn[f]) for f in _lib.NN_PARTIAL_DTYPE.names}
        out.update(keys=keys, sum_H=sum_h, n_H=n_h, have_mme=bool(hm.value))
        return out

    def deformation_field(self, query_slot: int, voxel_size: float, max_distance: float, min_pairs: int = 30,
                          min_spread: Optional[float] = None, fetch: bool = True) -> dict:
        """me_voxel_deformation: the rigid deformation of every voxel of the query cloud against the reference of the last
        nn1(query_slot, ..), on the lattice of voxel_gaussians(query_slot, voxel_size); min_spread None = voxel_size / 20.
        -> the totals of me_deform_summary (its n_pairs as n_pairs_total) and, computed here: mean_disp = sum n|t0| / sum n, rms_disp = sqrt(sum n|t0|^2 / sum n),
        max_disp and max_key (None without a fitted voxel), share_translation = 1 - sum e_t / sum e0 and share_rigid =
        1 - sum e_R / sum e0_fit (NaN when the denominator is 0).  With fetch also the rows: keys (V, 3), n_pairs, flags, sums (V, 23),
        t0, u (V, 3), R (V, 3, 3), e0, e_t, e_R and angle = rotation_angle(R) in radians."""
        ms = float(voxel_size) / 20.0 if min_spread is None else float(min_spread)
        o = _lib.DeformSummary()
        self._ck(self._L.me_voxel_deformation(self._ctx, query_slot, float(voxel_size), float(max_distance), int(min_pairs), ms, C.byref(o)))
        res = {f: getattr(o, f) for f in ("n_voxels", "n_with_pairs", "n_fit", "n_rot", "max_row", "sum_n_t0", "sum_n_t0sq",
                                          "sum_e0", "sum_e_t", "sum_e0_fit", "sum_e_R")}
        res["n_pairs_total"] = o.n_pairs  # (n_pairs is the per-voxel array of the rows)
        nan = float("nan")
        res["mean_disp"] = o.sum_n_t0 / o.n_pairs if o.n_pairs > 0 else nan
        res["rms_disp"] = math.sqrt(o.sum_n_t0sq / o.n_pairs) if o.n_pairs > 0 else nan
        res["max_disp"] = o.max_t0
        res["max_key"] = tuple(int(k) for k in o.max_key) if o.max_row >= 0 else None
        res["share_translation"] = 1.0 - o.sum_e_t / o.sum_e0 if o.sum_e0 != 0 else nan
        res["share_rigid"] = 1.0 - o.sum_e_R / o.sum_e0_fit if o.sum_e0_fit != 0 else nan
        if fetch:
            res.update(self.deformation_fetch(query_slot))
        return res

    def deformation_fetch(self, query_slot: int) -> dict:
        """me_voxel_deformation_fetch: the rows of the last deformation_field(query_slot, ..)."""
        nv = C.c_int64(0)
        self._ck(self._L.me_voxel_deformation_fetch(self._ctx, query_slot, 0, 0, 0, 0, 0, 0, 0, 0, C.byref(nv)))
        v = nv.value
        keys, n, fl = np.empty((v, 3), np.int32), np.empty(v, np.int64), np.empty(v, np.uint8)
        sums, t0, u = np.empty((v, _lib.ME_DEFORM_SUMS), np.float64), np.empty((v, 3), np.float64), np.empty((v, 3), np.float64)
        R, e = np.empty((v, 9), np.float64), np.empty((v, 3), np.float64)
        self._ck(self._L.me_voxel_deformation_fetch(self._ctx, query_slot, _addr(keys), _addr(n), _addr(fl), _addr(sums), _addr(t0), _addr(u),
                                                    _addr(R), _addr(e), C.byref(nv)))
        return dict(keys=keys, n_pairs=n, flags=fl, sums=sums, t0=t0, u=u, R=R.reshape(v, 3, 3), e0=np.ascontiguousarray(e[:, 0]),
                    e_t=np.ascontiguousarray(e[:, 1]), e_R=np.ascontiguousarray(e[:, 2]), angle=rotation_angle(R))

    def voxel_distances(self, voxel_size: float, sigmas, min_pts: int = 100, max_points: int = 2048, eig_floor: float = 1e-6,
                        fetch: bool = True) -> dict:
        """me_voxel_distances: per row of calculateVMD(voxel_size, min_pts) the point-set MMD of the two clouds' points in the voxel
        at 1 - 4 kernel bandwidths `sigmas`, and the Gaussian closed forms KL(est || gt), KL(gt || est), Bhattacharyya and the textbook
        W2 (definitions: include/mapeval_hip.h).  max_points: a fuller voxel is sub-sampled by a stride (0: never).
        -> the summary: n_rows, n_rows_subsampled, n_pairs_total, mean_mmd, mean_mmd2_u (one per bandwidth) and mean_kl_est_gt,
        mean_kl_gt_est, mean_bhattacharyya, mean_w2 (NaN without rows).  With fetch also the rows: keys (V, 3), n_pop, n_used (V, 2),
        ksum (V, n_sigma, 3: Sxx, Syy, Sxy), mmd2_u, mmd2_b, mmd (V, n_sigma), kl_est_gt, kl_gt_est, bhattacharyya, w2 (V)."""
        sg = np.atleast_1d(np.asarray(sigmas, dtype=np.float64)).ravel()
        if not 1 <= sg.shape[0] <= 4:
            raise ValueError("voxel_distances: 1 to 4 bandwidths")
        ns = int(sg.shape[0])
        p = _lib.VoxDistParams()
        p.voxel_size, p.min_pts, p.n_sigma, p.max_points, p.eig_floor = float(voxel_size), int(min_pts), ns, int(max_points), float(eig_floor)
        for b in range(ns):
            p.sigma[b] = float(sg[b])
        o = _lib.VoxDistOut()
        nr = C.c_int64(0)
        arrays = {}
        if fetch:
            self._ck(self._L.me_voxel_distances(self._ctx, C.byref(p), 0, 0, 0, 0, 0, 0, C.byref(nr), None))
            v = nr.value
            keys, pop, used = np.empty((v, 3), np.int32), np.empty((v, 2), np.int32), np.empty((v, 2), np.int32)
            ksum, mmd2, gauss = np.empty((v, ns, 3), np.float64), np.empty((v, ns, 2), np.float64), np.empty((v, 4), np.float64)
            self._ck(self._L.me_voxel_distances(self._ctx, C.byref(p), _addr(keys), _addr(pop), _addr(used), _addr(ksum), _addr(mmd2),
                                                _addr(gauss), C.byref(nr), C.byref(o)))
            mb = np.ascontiguousarray(mmd2[:, :, 1])
            arrays = dict(keys=keys, n_pop=pop, n_used=used, ksum=ksum, mmd2_u=np.ascontiguousarray(mmd2[:, :, 0]), mmd2_b=mb,
                          mmd=np.sqrt(np.maximum(0.0, mb)), kl_est_gt=np.ascontiguousarray(gauss[:, 0]),
                          kl_gt_est=np.ascontiguousarray(gauss[:, 1]), bhattacharyya=np.ascontiguousarray(gauss[:, 2]),
                          w2=np.ascontiguousarray(gauss[:, 3]))
        else:
            self._ck(self._L.me_voxel_distances(self._ctx, C.byref(p), 0, 0, 0, 0, 0, 0, C.byref(nr), C.byref(o)))
        res = dict(n_rows=o.n_rows, n_rows_subsampled=o.n_rows_subsampled, n_pairs_total=o.n_pairs, sigmas=sg.copy(),
                   mean_mmd=np.array(o.mean_mmd[:ns]), mean_mmd2_u=np.array(o.mean_mmd2_u[:ns]), mean_kl_est_gt=o.mean_gauss[0],
                   mean_kl_gt_est=o.mean_gauss[1], mean_bhattacharyya=o.mean_gauss[2], mean_w2=o.mean_gauss[3])
        res.update(arrays)
        return res

    def voxel_transport(self, voxel_size: float, blur=None, directions=32, min_pts: int = 100, max_points: int = 512, scaling: float = 0.5,
                        n_final: int = TRANSPORT_N_FINAL, eps_schedule=None, fetch: bool = True) -> dict:
        """me_voxel_transport: per row of calculateVMD(voxel_size, min_pts) the sliced 2-Wasserstein distance of the two clouds' points
        in the voxel (exact per direction) and the debiased Sinkhorn divergence on a fixed eps schedule (definitions:
        include/mapeval_hip.h).  directions: a count (the table synth.fibonacci_directions(count); 0: no sliced part) or an (L, 3) array
        used as given.  The schedule: eps_schedule as given (empty: no Sinkhorn part), else transport_schedule(voxel_size, blur, scaling,
        n_final) with `blur` in metres, which has no default.  max_points (11 .. 1024): a fuller voxel is sub-sampled by a stride.
        -> the summary: n_rows, n_rows_subsampled, n_pairs_total, n_used_est, n_used_gt, mean_sw2, mean_max_sw2, mean_s, mean_sinkhorn,
        mean_marginal_err, max_marginal_err, max_marginal_row (NaN / -1 for a part that did not run or without rows), and `directions`
        and `eps_schedule` as used, so that the call can be replayed.  With fetch also the rows: keys (V, 3), n_pop, n_used (V, 2),
        sw2_sq, sw2, max_sw2_sq (V), max_dir (V, int), per_direction (V, L), ot_xy, ot_xx, ot_yy, s, sinkhorn, marginal_err (V), and f, g:
        lists of V arrays, the cross problem's final potentials per used point."""
        if isinstance(directions, (int, np.integer)):
            from . import synth

            dirs = synth.fibonacci_directions(int(directions)) if int(directions) > 0 else np.empty((0, 3), np.float64)
        else:
            dirs = np.ascontiguousarray(np.asarray(directions, dtype=np.float64).reshape(-1, 3))
        if eps_schedule is None:
            if blur is None:
                raise ValueError("voxel_transport: blur (metres) is required when no eps_schedule is given")
            eps = transport_schedule(voxel_size, blur, scaling, n_final)
        else:
            eps = np.ascontiguousarray(np.asarray(eps_schedule, dtype=np.float64).ravel())
        nl, nt = int(dirs.shape[0]), int(eps.shape[0])
        p = _lib.VoxTransParams()
        p.voxel_size, p.min_pts, p.n_dir, p.n_eps, p.reserved, p.max_points = float(voxel_size), int(min_pts), nl, nt, 0, int(max_points)
        da, ea = (_addr(dirs) if nl else 0), (_addr(eps) if nt else 0)
        o = _lib.VoxTransOut()
        nr = C.c_int64(0)
        call = self._L.me_voxel_transport
        arrays = {}
        if fetch:
            self._ck(call(self._ctx, C.byref(p), da, ea, 0, 0, 0, 0, 0, 0, 0, C.byref(nr), None))
            v = nr.value
            keys, pop, used = np.empty((v, 3), np.int32), np.empty((v, 2), np.int32), np.empty((v, 2), np.int32)
            self._ck(call(self._ctx, C.byref(p), da, ea, 0, 0, _addr(used), 0, 0, 0, 0, C.byref(nr), None))  # (the rows alone: the sizes)
            nx, ny = int(used[:, 0].sum()), int(used[:, 1].sum())
            sl, sk = np.full((v, 4), np.nan), np.full((v, 6), np.nan)
            per, pot = np.empty((v, nl), np.float64), np.empty(nx + ny if nt else 0, np.float64)
            self._ck(call(self._ctx, C.byref(p), da, ea, _addr(keys), _addr(pop), _addr(used), _addr(sl), _addr(sk), _addr(per),
                          _addr(pot) if nt else 0, C.byref(nr), C.byref(o)))
            ox, oy = np.concatenate([[0], np.cumsum(used[:, 0])]), nx + np.concatenate([[0], np.cumsum(used[:, 1])])
            col = lambda a, k: np.ascontiguousarray(a[:, k])  # noqa: E731
            arrays = dict(keys=keys, n_pop=pop, n_used=used, sw2_sq=col(sl, 0), sw2=col(sl, 1), max_sw2_sq=col(sl, 2),
                          max_dir=(col(sl, 3).astype(np.int32) if nl else np.full(v, -1, np.int32)), per_direction=per,
                          ot_xy=col(sk, 0), ot_xx=col(sk, 1), ot_yy=col(sk, 2), s=col(sk, 3), sinkhorn=col(sk, 4), marginal_err=col(sk, 5),
                          f=[pot[ox[r]:ox[r + 1]].copy() for r in range(v)] if nt else [],
                          g=[pot[oy[r]:oy[r + 1]].copy() for r in range(v)] if nt else [])
        else:
            self._ck(call(self._ctx, C.byref(p), da, ea, 0, 0, 0, 0, 0, 0, 0, C.byref(nr), C.byref(o)))
        res = dict(n_rows=o.n_rows, n_rows_subsampled=o.n_rows_subsampled, n_pairs_total=o.n_pairs, n_used_est=o.n_used_est,
                   n_used_gt=o.n_used_gt, mean_sw2=o.mean_sw2, mean_max_sw2=o.mean_max_sw2, mean_s=o.mean_s, mean_sinkhorn=o.mean_sinkhorn,
                   mean_marginal_err=o.mean_marginal_err, max_marginal_err=o.max_marginal_err, max_marginal_row=o.max_marginal_row,
                   directions=dirs.copy(), eps_schedule=eps.copy())
        res.update(arrays)
        return res

    def voxel_metrics_table(self, voxel_size: float, gate: float, gate_mode: int, trunc, min_pts: int = 100,
                            scs_radius: int = 5) -> np.ndarray:
        """The joined per-voxel table of a finished suite — what the C++ host writes to voxel_metrics.txt: one row per voxel of
        the union of both clouds' keys, ascending, in the columns of VOXEL_METRICS_COLUMNS (a cloud without points in the voxel
        has zeros there); w2 = the voxel's W of me_awd_scs (voxel_errors.txt) where AWD defines one, NaN elsewhere."""
        e = self.voxel_metrics(ME_SLOT_EST, voxel_size, gate, gate_mode, trunc)
        g = self.voxel_metrics(ME_SLOT_GT, voxel_size, gate, gate_mode, trunc)
        vmd = self.calculateVMD(voxel_size, min_pts, scs_radius, rows=True)
        keys = np.unique(np.concatenate([e["keys"], g["keys"]]), axis=0)
        packed = _pack_keys(keys)
        t = np.zeros((keys.shape[0], len(VOXEL_METRICS_COLUMNS)), np.float64)
        t[:, 0:3] = keys
        for side, base, nq_col, h_col in ((e, 5, 3, 39), (g, 22, 4, 41)):
            at = np.searchsorted(packed, _pack_keys(side["keys"]))
            t[at, nq_col] = side["n_query"]
            t[at, base] = side["n_corr"]
            t[at, base + 1:base + 6] = side["n_inl"]
            t[at, base + 6:base + 11] = side["sum_d"]
            t[at, base + 11:base + 16] = side["sum_d2"]
            t[at, base + 16] = side["sum_sqrt_all"]
            t[at, h_col] = side["n_H"]
            t[at, h_col + 1] = side["sum_H"]
        t[:, 43] = np.nan
        rows = vmd["rows"]
        if rows.shape[0]:
            wk = np.rint(rows[:, 0:3] / voxel_size).astype(np.int64)  # (columns 0-2 of voxel_errors.txt: key * voxel_size)
            t[np.searchsorted(packed, _pack_keys(wk)), 43] = rows[:, 9]
        return t

    def calculateVMD(self, voxel_size: float, min_pts: int = 100, scs_radius: int = 5, rows: bool = True):
        """map_eval.cpp:240-390 -> dict(awd, scs, rows, w_sorted, counts)."""
        n = C.c_int64(0)
        awd, scs = C.c_double(), C.c_double()
        counts = np.zeros(3, np.int64)
        self._ck(self._L.me_awd_scs(self._ctx, float(voxel_size), min_pts, scs_radius, 0, 0, C.byref(n), C.byref(awd),
                                    C.byref(scs), _addr(counts)))
        res = dict(awd=awd.value, scs=scs.value, counts=tuple(int(c) for c in counts), n_rows=n.value)
        if rows and n.value > 0:
            r = np.empty((n.value, 27), np.float64)
            ws = np.empty(n.value, np.float64)
            cap = C.c_int64(n.value)
            self._ck(self._L.me_awd_scs(self._ctx, float(voxel_size), min_pts, scs_radius, _addr(r), _addr(ws), C.byref(cap),
                                        C.byref(awd), C.byref(scs), _addr(counts)))
            res.update(rows=r, w_sorted=ws)
        elif rows:
            res.update(rows=np.empty((0, 27)), w_sorted=np.empty(0))
        return res

    def w2_batch(self, mu1, sigma1, n1, mu2, sigma2, n2) -> np.ndarray:
        """Batched computeWassersteinDistanceGaussian(voxel1, voxel2) (voxel_calculator.cpp:115-140)."""
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (mu1, sigma1, mu2, sigma2)]
        n1 = np.ascontiguousarray(n1, dtype=np.int32)
        n2 = np.ascontiguousarray(n2, dtype=np.int32)
        cnt = n1.shape[0]
        w = np.empty(cnt, np.float64)
        self._ck(self._L.me_w2_batch(self._ctx, _addr(a[0]), _addr(a[1]), _addr(n1), _addr(a[2]), _addr(a[3]), _addr(n2), cnt,
                                     _addr(w)))
        return w

    def scs_table(self, keys, w, radius: int = 5) -> float:
        """SCS (map_eval.cpp:347-389) of a sparse W table."""
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        out = C.c_double()
        self._ck(self._L.me_scs_table(self._ctx, _addr(keys), _addr(w), w.shape[0], radius, C.byref(out)))
        return out.value

    # ---- multi-GPU spatial slab mode (include/mapeval_hip.h: me_set_slab ...) ----
    def set_slab(self, axis: int, lo: float = 0.0, hi: float = 0.0, halo: float = 0.0):
        """Keep lo-halo <= p[axis] < hi+halo at the next uploads; lo <= p[axis] < hi are the points this rank owns."""
        self._ck(self._L.me_set_slab(self._ctx, int(axis), float(lo), float(hi), float(halo)))

    def nn_unresolved_count(self, query_slot: int) -> int:
        n = C.c_int64(0)
        self._ck(self._L.me_nn_unresolved(self._ctx, query_slot, 0, 0, 0, C.byref(n)))
        return n.value

    def nn_unresolved(self, query_slot: int, with_d2: bool = False):
        """(count, 3) float64 cuda tensor: owned queries whose 1-NN may live on another rank; with_d2: (count, 4), the
        fourth column = their current best squared distance (the bound the other ranks have to beat)."""
        import torch

        cnt = self.nn_unresolved_count(query_slot)
        dev = torch.device("cuda", self.device)
        out = torch.empty((cnt, 3), dtype=torch.float64, device=dev)
        d2 = torch.empty(cnt, dtype=torch.float64, device=dev) if with_d2 else None
        if cnt:
            n = C.c_int64(0)
            self._ck(self._L.me_nn_unresolved(self._ctx, query_slot, out.data_ptr(), d2.data_ptr() if with_d2 else 0, cnt,
                                              C.byref(n)))
        return torch.cat([out, d2[:, None]], 1) if with_d2 else out

    def nn_points(self, ref_slot: int, xyz, bound=None, covered=None, axis: int = 0):
        """Exact squared distance of arbitrary points (cuda tensor (m,3) float64) to this rank's part of ref_slot;
        bound (m,): upper bounds -> min(bound, nearest here), far ranks prune at once (me_nn_points_bounded);
        covered (m,2) + axis: the band [lo, hi) of `axis` each query's owner has searched already (me_nn_points_covered)."""
        import torch

        xyz = xyz.to(torch.device("cuda", self.device), torch.float64).contiguous()
        cov = None
        if bound is None:
            d2 = torch.empty(xyz.shape[0], dtype=torch.float64, device=xyz.device)
            fn = self._L.me_nn_points
        else:
            d2 = bound.to(xyz.device, torch.float64).clone().contiguous()
            fn = self._L.me_nn_points_bounded
            if covered is not None:
                cov = covered.to(xyz.device, torch.float64).contiguous()
        torch.cuda.current_stream(xyz.device).synchronize()
        if cov is not None:
            self._ck(self._L.me_nn_points_covered(self._ctx, ref_slot, xyz.data_ptr(), int(xyz.shape[0]), d2.data_ptr(), int(axis), cov.data_ptr()))
        else:
            self._ck(fn(self._ctx, ref_slot, xyz.data_ptr(), int(xyz.shape[0]), d2.data_ptr()))
        return d2

    def nn_fetch(self, query_slot: int):
        """-> (idx, d2) of the last nn1(query_slot, ..) as it stands now (slab mode: after nn_patch; halo points d2 = -1)."""
        n = self.size(query_slot)
        idx, d2 = np.empty(n, np.int32), np.empty(n, np.float64)
        self._ck(self._L.me_nn_fetch(self._ctx, query_slot, _addr(idx), _addr(d2)))
        return idx, d2

    def set_mme_result(self, slot: int, entropies, valid):
        """Per-point MME results computed elsewhere (distributed run) -> ColorPointCloudByMME works on this context."""
        e = np.ascontiguousarray(entropies, dtype=np.float64)
        v = np.ascontiguousarray(valid, dtype=np.uint8)
        self._ck(self._L.me_set_mme_result(self._ctx, slot, _addr(e), _addr(v)))

    def set_nn_result(self, query_slot: int, ref_slot: int, d2):
        d = np.ascontiguousarray(d2, dtype=np.float64)
        self._ck(self._L.me_set_nn_result(self._ctx, query_slot, ref_slot, _addr(d)))

    def slab_points(self, slot: int):
        """Slab mode: (orig_index[n], owned[n]) of the points this context holds, in the order of its per-point outputs."""
        n = self.size(slot)
        orig, owned = np.empty(n, np.int64), np.empty(n, np.uint8)
        cnt = C.c_int64(0)
        self._ck(self._L.me_slab_points(self._ctx, slot, _addr(orig), _addr(owned), n, C.byref(cnt)))
        return orig, owned.astype(bool)

    # ---- the cross-rank 1-NN step on one fixed-capacity message (me_nn_cross_*) ----
    def nn_cross_message(self, cap: int, n_loc_est: int, n_loc_gt: int):
        """-> (message (1 + 2 cap, 4) cuda tensor, [open queries map -> gt, gt -> map])."""
        import torch

        msg = torch.empty((1 + 2 * cap, 4), dtype=torch.float64, device=torch.device("cuda", self.device))
        counts = np.zeros(2, np.int64)
        self._ck(self._L.me_nn_cross_message(self._ctx, msg.data_ptr(), int(cap), int(n_loc_est), int(n_loc_gt), _addr(counts)))
        return msg, [int(counts[0]), int(counts[1])]

    def nn_cross_answer(self, gathered, cap: int, own_rank: int, dir_mask: int, axis: int, cuts, halo: float):
        """gathered (world, 1 + 2 cap, 4) cuda tensor -> d2 (world, 1 + 2 cap): the block the ranks min-reduce."""
        import torch

        g = gathered.to(torch.device("cuda", self.device), torch.float64).contiguous()
        world = int(g.shape[0])
        d2 = torch.zeros((world, 1 + 2 * cap), dtype=torch.float64, device=g.device)
        c = np.ascontiguousarray(cuts, dtype=np.float64)
        torch.cuda.current_stream(g.device).synchronize()
        self._ck(self._L.me_nn_cross_answer(self._ctx, g.data_ptr(), world, int(cap), int(own_rank), int(dir_mask), int(axis), _addr(c), float(halo),
                                            d2.data_ptr()))
        return d2

    def nn_cross_patch(self, d2_reduced, cap: int, own_rank: int):
        import torch

        d = d2_reduced.to(torch.device("cuda", self.device), torch.float64).contiguous()
        torch.cuda.current_stream(d.device).synchronize()
        self._ck(self._L.me_nn_cross_patch(self._ctx, d.data_ptr(), int(cap), int(own_rank)))

    def nn_patch(self, query_slot: int, d2):
        import torch

        d2 = d2.to(torch.device("cuda", self.device), torch.float64).contiguous()
        torch.cuda.current_stream(d2.device).synchronize()
        self._ck(self._L.me_nn_patch(self._ctx, query_slot, d2.data_ptr(), int(d2.shape[0])))

    def voxel_partials(self, slot: int, voxel_size: float):
        """Owned-point voxel partials: keys[V,3] int32, n[V] int32, mu[V,3], raw M2[V,3,3]."""
        nv = C.c_int64(0)
        self._ck(self._L.me_voxel_partials(self._ctx, slot, float(voxel_size), 0, 0, 0, 0, C.byref(nv)))
        v = nv.value
        keys = np.empty((v, 3), np.int32)
        n = np.empty(v, np.int32)
        mu = np.empty((v, 3), np.float64)
        m2 = np.empty((v, 9), np.float64)
        if v:
            nv = C.c_int64(v)
            self._ck(self._L.me_voxel_partials(self._ctx, slot, float(voxel_size), _addr(keys), _addr(n), _addr(mu), _addr(m2),
                                               C.byref(nv)))
        return keys, n, mu, m2.reshape(v, 3, 3)

    # ---- multi-GPU with distributed input (include/mapeval_hip.h: me_halo_pack_device ...) ----
    def transform_points(self, xyz, T):
        """Open3D Transform (map_eval.cpp:1206) on a cuda tensor (n,3) float64, in place; returns it."""
        import torch

        Tm = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        assert xyz.is_cuda and xyz.dtype == torch.float64 and xyz.is_contiguous()
        torch.cuda.current_stream(xyz.device).synchronize()
        self._ck(self._L.me_transform_points_device(self._ctx, xyz.data_ptr(), int(xyz.shape[0]), _addr(Tm)))
        return xyz

    def halo_pack(self, xyz, axis: int, cuts, halo: float):
        """Send side of the halo exchange: xyz (n,3) cuda float64 -> (packed (m,3) cuda tensor, destination-major; counts
        list[world]).  Rank k receives every point with cuts[k] - halo <= p[axis] < cuts[k+1] + halo."""
        import torch

        world = len(cuts) - 1
        c = np.ascontiguousarray(cuts, dtype=np.float64)
        counts = np.zeros(world, np.int64)
        assert xyz.is_cuda and xyz.dtype == torch.float64 and xyz.is_contiguous()
        torch.cuda.current_stream(xyz.device).synchronize()
        n = int(xyz.shape[0])
        # one call: count + scatter into a buffer sized for the usual case (every point to its owner, a thin halo to the
        # neighbours); the rare overflow (halo wider than the slabs) comes back as ME_ERR_CAPACITY with the exact counts
        cap = n + n // 2 + 4096
        out = torch.empty((cap, 3), dtype=torch.float64, device=xyz.device)
        rc = self._L.me_halo_pack_device(self._ctx, xyz.data_ptr(), n, int(axis), _addr(c), world, float(halo), out.data_ptr(), cap,
                                         _addr(counts))
        total = int(counts.sum())
        if rc == _lib.ME_ERR_CAPACITY:
            out = torch.empty((total, 3), dtype=torch.float64, device=xyz.device)
            rc = self._L.me_halo_pack_device(self._ctx, xyz.data_ptr(), n, int(axis), _addr(c), world, float(halo), out.data_ptr(),
                                             total, _addr(counts))
        self._ck(rc)
        out = out[:total]
        return out, [int(x) for x in counts]

    def lattice_messages(self, parts, e0: int):
        """The rows of this rank's plan-gather message for its 1 or 2 pieces (cuda (n,3) float64 tensors): int64 (len(parts),
        8 + 3 ME_LATTICE_BINS) on the device, header included — me_lattice_messages_device."""
        import torch

        dev = torch.device("cuda", self.device)
        for p in parts:
            assert p.is_cuda and p.dtype == torch.float64 and p.is_contiguous()
        torch.cuda.current_stream(dev).synchronize()
        msg = torch.empty((len(parts), 8 + 3 * _lib.ME_LATTICE_BINS), dtype=torch.int64, device=dev)
        a = parts[0]
        b = parts[1] if len(parts) > 1 else parts[0]
        self._ck(self._L.me_lattice_messages_device(self._ctx, a.data_ptr(), int(a.shape[0]), b.data_ptr(), int(b.shape[0]) if len(parts) > 1 else 0,
                                                    len(parts), int(e0), msg.data_ptr()))
        return msg

    def lattice_plan_raw(self, allm, halo: float, e0: int):
        """The plan of the lean exchange from the gathered messages (world, clouds, 8 + 3 ME_LATTICE_BINS) int64 cuda tensor:
        me_lattice_plan_device's output vector as numpy int64 (dist.lattice_plan unpacks it)."""
        import torch

        g = allm.to(torch.device("cuda", self.device), torch.int64).contiguous()
        world, clouds = int(g.shape[0]), int(g.shape[1])
        out = np.zeros(4 + clouds + world - 1 + world * clouds * world, np.int64)
        torch.cuda.current_stream(g.device).synchronize()
        self._ck(self._L.me_lattice_plan_device(self._ctx, g.data_ptr(), world, clouds, float(halo), int(e0), out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def set_voxel_hint(self, voxel_size: float):
        """Index builds from now on also emit the voxel run records for this voxel size (0: off): me_set_voxel_hint."""
        self._ck(self._L.me_set_voxel_hint(self._ctx, float(voxel_size)))

    def lattice_histograms(self, xyz, e0: int):
        """Marginal histograms of a raw cuda (n,3) float64 buffer on the absolute lattice of bin width 2^(e0 + level):
        (level, origin_bin int64[3], neg_inf int64[3], hist (3, ME_LATTICE_BINS) cuda int32).  me_lattice_histograms_device."""
        import torch

        assert xyz.is_cuda and xyz.dtype == torch.float64 and xyz.is_contiguous()
        torch.cuda.current_stream(xyz.device).synchronize()
        hist = torch.empty((3, _lib.ME_LATTICE_BINS), dtype=torch.int32, device=xyz.device)
        level = C.c_int32(0)
        origin = (C.c_int64 * 3)()
        ninf = (C.c_int64 * 3)()
        self._ck(self._L.me_lattice_histograms_device(self._ctx, xyz.data_ptr(), int(xyz.shape[0]), int(e0), C.byref(level), origin, ninf,
                                                      hist.data_ptr()))
        return int(level.value), np.array(list(origin), dtype=np.int64), np.array(list(ninf), dtype=np.int64), hist

    def voxel_partial_rows(self, slot: int, voxel_size: float):
        """This rank's voxel partials as a (V,16) cuda tensor [kx,ky,kz,n,mu(3),M2(9)] (no host copy)."""
        import torch

        nv = C.c_int64(0)
        self._ck(self._L.me_voxel_partial_rows_device(self._ctx, slot, float(voxel_size), 0, 0, C.byref(nv)))
        rows = torch.empty((nv.value, 16), dtype=torch.float64, device=torch.device("cuda", self.device))
        if nv.value:
            self._ck(self._L.me_voxel_partial_rows_device(self._ctx, slot, float(voxel_size), rows.data_ptr(), nv.value, C.byref(nv)))
        return rows

    def voxel_merge(self, slot: int, voxel_size: float, rows):
        """Chan merge of the gathered partial rows of ALL ranks (cuda tensor (m,16); n == 0 rows are padding) into the slot's
        voxel table; calculateVMD then runs on the merged tables."""
        import torch

        rows = rows.to(torch.device("cuda", self.device), torch.float64).contiguous()
        torch.cuda.current_stream(rows.device).synchronize()
        self._ck(self._L.me_voxel_merge_device(self._ctx, slot, float(voxel_size), rows.data_ptr(), int(rows.shape[0])))

    # ---- whole suite ----
    def run_suite(self, p: Param, gate_mode: int = ME_GATE_LE_UNSQUARED) -> _lib.SuiteOut:
        sp = self._suite_params(p, gate_mode)
        out = _lib.SuiteOut()
        self._ck(self._L.me_run_suite(self._ctx, C.byref(sp), C.byref(out)))
        return out

    def _suite_params(self, p: Param, gate_mode: int) -> _lib.SuiteParams:
        sp = _lib.SuiteParams()
        sp.icp_max_distance = p.icp_max_distance_
        sp.gate_mode = gate_mode
        for k in range(5):
            sp.trunc[k] = p.trunc_dist_[k]
        sp.nn_radius = p.nn_radius_
        sp.vmd_voxel_size = p.vmd_voxel_size_
        sp.evaluate_mme = int(p.evaluate_mme_)
        sp.evaluate_gt_mme = int(p.evaluate_gt_mme_)
        sp.min_pts = 100
        sp.scs_radius = 5
        return sp

    def run_suite_from(self, est, gt, p: Param, overlap: bool = True, gate_mode: int = ME_GATE_LE_UNSQUARED,
                       pin_host_input: bool = False) -> _lib.SuiteOut:
        """me_run_suite_from: the whole pass of MapEval::process (map_eval.cpp:52-85) from the two raw clouds in ONE library call —
        uploads, index builds, MME x2 (the map as loaded), p.initial_matrix_ (:1206), both 1-NN directions + statistics, voxel
        Gaussians, AWD / CDF / SCS; overlap: the library's internal second lane (ME_SUITE_OVERLAP).  est / gt: (N,3) float64 numpy
        arrays or torch tensors (both host or both cuda); None, None: the clouds already uploaded."""
        flags = (_lib.ME_SUITE_OVERLAP if overlap else 0) | (_lib.ME_SUITE_PIN_HOST_INPUT if pin_host_input else 0)
        ne = ng = 0
        if est is not None:
            on_dev = []
            arrs = []
            for a in (est, gt):
                if isinstance(a, np.ndarray):
                    a = np.ascontiguousarray(a, dtype=np.float64)
                    on_dev.append(False)
                else:
                    import torch

                    if a.dtype != torch.float64 or not a.is_contiguous():
                        a = a.to(torch.float64).contiguous()
                    on_dev.append(bool(a.is_cuda))
                    if a.is_cuda:
                        torch.cuda.current_stream(a.device).synchronize()  # producer stream -> library stream hand-over
                if a.ndim != 2 or a.shape[1] != 3:
                    raise ValueError("expected (N,3) arrays")
                arrs.append(a)
            if on_dev[0] != on_dev[1]:
                raise ValueError("run_suite_from: both clouds in host memory, or both on the device")
            est, gt = arrs
            if on_dev[0]:
                flags |= _lib.ME_SUITE_DEVICE_INPUT
            ne, ng = int(est.shape[0]), int(gt.shape[0])
            self._held[ME_SLOT_EST], self._held[ME_SLOT_GT] = est, gt
        Tm = np.ascontiguousarray(p.initial_matrix_, dtype=np.float64).reshape(16)
        sp = self._suite_params(p, gate_mode)
        out = _lib.SuiteOut()
        self._ck(self._L.me_run_suite_from(self._ctx, _addr(est), ne, _addr(gt), ng, _addr(Tm), C.byref(sp), flags, C.byref(out)))
        return out

    @staticmethod
    def suite_dict(o: _lib.SuiteOut) -> dict:
        """A SuiteOut as the dict dist.suite_step returns (same keys, same numbers)."""
        def d(s):
            f = lambda x: np.array(list(x), dtype=np.float64)
            return dict(n_corr=int(s.n_corr), number=f(s.number), mean=f(s.mean), rmse=f(s.rmse), fitness=f(s.fitness),
                        sigma=f(s.sigma), mean_nn=float(s.mean_nn_dist))
        eg, ge = d(o.est_gt), d(o.gt_est)
        return dict(est_gt=eg, gt_est=ge, ac=eg["rmse"], com=eg["fitness"], cd=float(o.full_chamfer), mme_est=float(o.mme_est),
                    mme_gt=float(o.mme_gt), mme_valid=int(o.mme_est_valid), awd=float(o.awd), scs=float(o.scs), n_w=int(o.n_w_voxels),
                    n_est=int(o.est_gt.n_src), n_gt=int(o.gt_est.n_src), stage_ms=[float(x) for x in o.stage_ms])

    def mme_fetch(self, slot: int):
        """me_mme_fetch: (entropies[N], valid[N]) of the slot's last MME pass, cloud order."""
        n = self.size(slot)
        ent = np.zeros(n, np.float64)
        val = np.zeros(n, np.uint8)
        self._ck(self._L.me_mme_fetch(self._ctx, slot, _addr(ent), _addr(val)))
        return ent, val

    def cell_table(self, slot: int, which: int):
        """me_cell_table_fetch (debug): (hkeys[S], hvals[S], cell_start[C + 1], entries[S]) of the slot's radius (which = 0) or 1-NN
        (which = 1) cell table; entries is a record array with fields key, start, count."""
        ns, nc = C.c_int64(), C.c_int64()
        self._ck(self._L.me_cell_table_fetch(self._ctx, slot, which, C.byref(ns), C.byref(nc), None, None, None, None))
        hkeys = np.zeros(ns.value, np.uint64)
        hvals = np.zeros(ns.value, np.uint32)
        cell_start = np.zeros(nc.value + 1, np.uint32)
        ent = np.zeros(ns.value, np.dtype([("key", "<u8"), ("start", "<u4"), ("count", "<u4")]))
        self._ck(self._L.me_cell_table_fetch(self._ctx, slot, which, C.byref(ns), C.byref(nc), _addr(hkeys), _addr(hvals), _addr(cell_start),
                                              _addr(ent)))
        return hkeys, hvals, cell_start, ent

    # ---- instrumentation ----
    def timers_enable(self, on: bool = True):
        self._ck(self._L.me_timers_enable(self._ctx, int(on)))

    def timers_reset(self):
        self._ck(self._L.me_timers_reset(self._ctx))

    def timer(self, name: str):
        ms, cnt = C.c_double(), C.c_int64()
        self._ck(self._L.me_timer_get(self._ctx, name.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value
