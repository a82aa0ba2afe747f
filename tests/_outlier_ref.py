"""numpy restatement of the outlier filters (me_outlier.hip, include/mapeval_hip.h "outlier removal"), after Open3D 0.15's
PointCloud::RemoveStatisticalOutlier / RemoveRadiusOutlier.

Candidates come from scipy's cKDTree (k + 8 nearest, or the ball at r (1 + 1e-9)); their d2 is then recomputed exactly as the device
does, ((dx*dx + dy*dy) + dz*dz) in fp64, and re-ranked, so the tree's own rounding never decides anything.  brute_* are the O(n^2)
definitions the tests hold the restatement to on small clouds (chunked over rows).  sor_stats is Open3D's serial definition of the
statistics; sor_stats_device restates the device's fixed summation tree operation for operation, so that mean, std, threshold and
every keep bit can be compared with ==."""
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


# ---- the statistics as the device sums them (k_sor_partials / k_sor_final, block_sum_256 and wave_sum of me_internal.hpp) ----
def sor_launch(n: int):
    """(nb, per) of statistical_outlier(): nb blocks of 256 threads, block b owns [b * per, min((b + 1) * per, n))."""
    nb = min(1024, max(1, (n + 255) // 256))
    per = ((n + nb - 1) // nb + 255) // 256 * 256
    return nb, per


def _block_sum_256(v: np.ndarray) -> np.ndarray:
    """block_sum_256 over the last axis (256 thread values): each wave's shuffle tree v += shfl_down(v, o) for o = 32 .. 1 as lane 0
    sees it, then (s0 + s1) + (s2 + s3)."""
    w = v.reshape(v.shape[:-1] + (4, 64))
    o = 32
    while o:
        w = w[..., :o] + w[..., o:2 * o]
        o >>= 1
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def device_tree_sum(vals: np.ndarray) -> float:
    """The sum of vals in the order of k_sor_partials + k_sor_final.  Thread t of block b adds b * per + t, + 256, ... serially from
    0.0; the four waves of a block are combined by _block_sum_256; one block adds the nb partials in the same pattern.  (An entry the
    kernel skips is a 0.0 here: s + 0.0 == s for every s >= 0.)"""
    vals = np.ascontiguousarray(vals, np.float64)
    n = len(vals)
    nb, per = sor_launch(n)
    a = np.zeros(nb * per)
    a[:n] = vals
    a = a.reshape(nb, per // 256, 256)
    s = np.zeros((nb, 256))
    for j in range(per // 256):
        s = s + a[:, j, :]
    part = np.zeros(1024)
    part[:nb] = _block_sum_256(s)
    part = part.reshape(4, 256)
    s = np.zeros(256)
    for j in range(4):  # (nb <= 1024: thread t adds part[t], part[t + 256], ...)
        s = s + part[j]
    return float(_block_sum_256(s))


def sor_stats_device(avg: np.ndarray, std_ratio: float):
    """mean, std, threshold bit for bit as k_sor_partials<0>, k_sor_final<0>, k_sor_partials<1>, k_sor_final<1> compute them."""
    avg = np.ascontiguousarray(avg, np.float64)
    n = len(avg)
    pos = avg > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float64(device_tree_sum(np.where(pos, avg, 0.0))) / np.float64(n)
        d = avg - mean
        sq = np.float64(device_tree_sum(np.where(pos, d * d, 0.0)))
        std = np.sqrt(sq / np.float64(n - 1))
        thr = mean + np.float64(std_ratio) * std
    return float(mean), float(std), float(thr)


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
_BRUTE_ROWS = 256  # (rows per chunk: a 4097-point cloud never holds n^2 x 3 doubles at once)


def brute_sor_avg(xyz: np.ndarray, k: int) -> np.ndarray:
    xyz = np.asarray(xyz, np.float64)
    n = len(xyz)
    kk = min(k, n)
    out = np.empty(n)
    for b in range(0, n, _BRUTE_ROWS):
        d2 = d2_exact(xyz[b:b + _BRUTE_ROWS, None, :], xyz[None, :, :])
        d2 = np.sort(np.partition(d2, kk - 1, axis=1)[:, :kk], axis=1)  # (the kk smallest of every row, ascending)
        s = np.zeros(len(d2))
        for j in range(kk):  # (every row's serial sum from 0.0, ascending d2)
            s = s + np.sqrt(d2[:, j])
        out[b:b + _BRUTE_ROWS] = s / kk
    return out


def brute_ror_counts(xyz: np.ndarray, radius: float) -> np.ndarray:
    xyz = np.asarray(xyz, np.float64)
    n = len(xyz)
    out = np.empty(n, np.int32)
    for b in range(0, n, _BRUTE_ROWS):
        out[b:b + _BRUTE_ROWS] = np.count_nonzero(d2_exact(xyz[b:b + _BRUTE_ROWS, None, :], xyz[None, :, :]) < radius * radius, axis=1)
    return out
