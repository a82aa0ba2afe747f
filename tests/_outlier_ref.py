"""numpy restatement of the outlier filters (me_outlier.hip, include/mapeval_hip.h "outlier removal"), after Open3D 0.15's
PointCloud::RemoveStatisticalOutlier / RemoveRadiusOutlier.

Candidates come from scipy's cKDTree (k + 8 nearest, or the ball at r (1 + 1e-9)); their d2 is then recomputed exactly as the device
does, ((dx*dx + dy*dy) + dz*dz) in fp64, and re-ranked, so the tree's own rounding never decides anything.  brute_* are the O(n^2)
definitions the tests hold the restatement to on small clouds."""
from __future__ import annotations

import itertools
import os

import numpy as np

_WORKERS = min(16, os.cpu_count() or 1)  # (cKDTree threads)


def d2_exact(q: np.ndarray, p: np.ndarray) -> np.ndarray:
    """((dx*dx + dy*dy) + dz*dz), fp64, broadcast over the leading axes."""
    d = q - p
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _avg_from_sorted_d2(d2s: np.ndarray) -> np.ndarray:
    """avg_i from each row's ascending d2 (inf = no neighbour): sqrt summed left to right from 0, / the finite count."""
    s = np.zeros(d2s.shape[0])
    cnt = np.zeros(d2s.shape[0], np.int64)
    for j in range(d2s.shape[1]):  # (column by column: the device's sequential order)
        v = d2s[:, j]
        f = np.isfinite(v)
        s = s + np.where(f, np.sqrt(np.where(f, v, 0.0)), 0.0)
        cnt += f
    return np.where(cnt > 0, s / np.maximum(cnt, 1), 0.0)


def sor_avg(xyz: np.ndarray, k: int) -> np.ndarray:
    from scipy.spatial import cKDTree

    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    kq = min(n, k + 8)
    tree = cKDTree(xyz)
    out = np.empty(n)
    step = 1 << 20
    for b in range(0, n, step):  # (chunks: the candidate arrays of a 5 M-point cloud would hold gigabytes)
        q = xyz[b:b + step]
        _, idx = tree.query(q, k=kq, workers=_WORKERS)
        idx = np.asarray(idx).reshape(len(q), kq)
        d2 = d2_exact(q[:, None, :], xyz[idx])
        d2.sort(axis=1)
        kk = min(k, kq)
        # the k-th d2 must be settled by the candidates: the last one must be larger, or every tie of the k-th is in
        bad = (d2[:, kq - 1] <= d2[:, kk - 1]) & (kq < n)
        for i in np.nonzero(bad)[0]:  # (many exact ties: the whole cloud for those queries)
            d2[i, :kk] = np.sort(d2_exact(q[i], xyz))[:kk]
        out[b:b + step] = _avg_from_sorted_d2(d2[:, :kk])
    return out


def sor_stats(avg: np.ndarray, std_ratio: float):
    """mean, std, threshold as Open3D computes them (serial sums)."""
    n = len(avg)
    pos = avg[avg > 0]
    mean = float(np.sum(pos)) / n if n else float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = float(np.sum((pos - mean) ** 2))
        std = float(np.sqrt(np.float64(sq) / np.float64(n - 1)))
    return mean, std, mean + std_ratio * std


def sor_keep(avg: np.ndarray, threshold: float) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return (avg > 0) & (avg < threshold)


def sor(xyz: np.ndarray, k: int, std_ratio: float):
    avg = sor_avg(xyz, k)
    mean, std, thr = sor_stats(avg, std_ratio)
    return avg, sor_keep(avg, thr), (mean, std, thr)


def ror_counts(xyz: np.ndarray, radius: float) -> np.ndarray:
    from scipy.spatial import cKDTree

    xyz = np.ascontiguousarray(xyz, np.float64)
    lists = cKDTree(xyz).query_ball_point(xyz, radius * (1 + 1e-9), workers=_WORKERS)
    lens = np.fromiter((len(js) for js in lists), np.int64, len(lists))
    js = np.fromiter(itertools.chain.from_iterable(lists), np.int64, int(lens.sum()))
    qs = np.repeat(np.arange(len(xyz)), lens)
    inside = d2_exact(xyz[qs], xyz[js]) < radius * radius
    return np.bincount(qs[inside], minlength=len(xyz)).astype(np.int32)


def ror(xyz: np.ndarray, nb_points: int, radius: float):
    c = ror_counts(xyz, radius)
    return c, c > nb_points


# ---- O(n^2) definitions ----
def brute_sor_avg(xyz: np.ndarray, k: int) -> np.ndarray:
    xyz = np.asarray(xyz, np.float64)
    d2 = np.sort(d2_exact(xyz[:, None, :], xyz[None, :, :]), axis=1)[:, :k]
    out = np.empty(len(xyz))
    for i in range(len(xyz)):
        s = 0.0
        for v in d2[i]:
            s += float(np.sqrt(v))
        out[i] = s / len(d2[i])
    return out


def brute_ror_counts(xyz: np.ndarray, radius: float) -> np.ndarray:
    xyz = np.asarray(xyz, np.float64)
    return np.count_nonzero(d2_exact(xyz[:, None, :], xyz[None, :, :]) < radius * radius, axis=1).astype(np.int32)
