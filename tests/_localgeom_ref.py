"""numpy / scipy model of me_local_geometry (csrc/me_localgeom.hip): per point the radius neighbourhood under the library's convention,
its covariance formed two-pass in extended precision (centre first), eigenvalues by numpy.linalg.eigvalsh, the clamp, the validity rule
and the four shape features.  The model's own rounding is a few ulp of the largest eigenvalue; the device's error bound is
eig_bound()."""
import os

import numpy as np
from scipy.spatial import cKDTree

EPS = 2.0 ** -53
_LD = np.longdouble
_WORKERS = max(1, min(16, os.cpu_count() or 1))


def eig_bound(k, r):
    """|l_device - l_exact| <= 8 k 2^-53 r^2 per eigenvalue: each of the 9 sums holds k terms <= r^2 in magnitude, so any summation
    order errs by <= k eps sum|x| <= k^2 eps r^2; the division by k - 1 leaves ~ k eps r^2 per covariance entry; a symmetric
    perturbation moves an eigenvalue by at most its 2-norm (<= 3 x the entry error); Jacobi adds a few eps l1 <= a few eps r^2."""
    return 8.0 * np.asarray(k, np.float64) * EPS * r * r


def d2_lib(q, p):
    """((dx*dx + dy*dy) + dz*dz) in fp64, the library's expression (no FMA)."""
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def features(eig):
    """(linearity, planarity, sphericity, surface variation) of rows l1 >= l2 >= l3 with l1 > 0."""
    l1, l2, l3 = eig[:, 0], eig[:, 1], eig[:, 2]
    return np.stack([(l1 - l2) / l1, (l2 - l3) / l1, l3 / l1, l3 / ((l1 + l2) + l3)], 1)


def _finish(k, cov, min_k):
    """eigenvalues (clamped at 0, descending), validity; zeros where invalid"""
    n = len(k)
    eig = np.zeros((n, 3))
    have = k >= min_k
    if have.any():
        w = np.linalg.eigvalsh(cov[have])[:, ::-1]
        eig[have] = np.maximum(w, 0.0)
    valid = have & (eig[:, 0] > 0.0)
    eig[~valid] = 0.0
    return eig, valid


def local_geometry(xyz, r, min_k=5, queries=None, chunk=20_000, tree=None):
    """-> (eig[m, 3], k[m], valid[m]) for the points `queries` (indices into xyz; default: all) against the whole cloud."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    q_idx = np.arange(len(xyz)) if queries is None else np.asarray(queries, np.int64)
    tree = cKDTree(xyz) if tree is None else tree
    r2 = r * r
    m = len(q_idx)
    k_out = np.zeros(m, np.int64)
    cov = np.zeros((m, 3, 3))
    for c0 in range(0, m, chunk):
        qi = q_idx[c0:c0 + chunk]
        lists = tree.query_ball_point(xyz[qi], r * (1.0 + 1e-9), workers=_WORKERS)
        lens = np.fromiter((len(l) for l in lists), np.int64, len(lists))
        j = np.fromiter((v for l in lists for v in l), np.int64, int(lens.sum()))
        row = np.repeat(np.arange(len(qi)), lens)
        d = xyz[j] - xyz[qi][row]  # p_j - q, the device's own subtraction
        keep = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r2
        keep &= j != qi[row]  # the query itself, once (its coincident duplicates have other indices and stay)
        d, row = d[keep], row[keep]
        k = np.bincount(row, minlength=len(qi))
        k_out[c0:c0 + chunk] = k
        has = k > 0
        if not has.any():
            continue
        starts = np.concatenate([[0], np.cumsum(k)[:-1]])[has]  # (row is ascending: the pairs of a query are contiguous)
        dl = d.astype(_LD)
        kk = k[has].astype(_LD)
        mean = np.add.reduceat(dl, starts, axis=0) / kk[:, None]
        e = dl - np.repeat(mean, k[has], axis=0)
        s = np.zeros((int(has.sum()), 3, 3), _LD)
        for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
            s[:, a, b] = s[:, b, a] = np.add.reduceat(e[:, a] * e[:, b], starts)
        den = np.maximum(kk - 1, 1)
        cc = np.zeros((len(qi), 3, 3))
        cc[has] = (s / den[:, None, None]).astype(np.float64)
        cov[c0:c0 + chunk] = cc
    eig, valid = _finish(k_out, cov, min_k)
    return eig, k_out.astype(np.int32), valid


def brute(xyz, r, min_k=5):
    """The same quantities by O(N^2) brute force, the covariance summed with math.fsum-grade care (longdouble, two-pass)."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    k = np.zeros(n, np.int64)
    cov = np.zeros((n, 3, 3))
    for i in range(n):
        d = xyz - xyz[i]
        inside = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r * r
        inside[i] = False
        k[i] = inside.sum()
        if k[i] >= 2:
            e = d[inside].astype(_LD)
            e = e - e.mean(0)
            cov[i] = ((e.T @ e) / _LD(k[i] - 1)).astype(np.float64)
    eig, valid = _finish(k, cov, min_k)
    return eig, k.astype(np.int32), valid


def summary(eig, k, valid):
    """The info dict of Engine.local_geometry from per-point arrays (means over the valid points, 0.0 without one)."""
    import math

    v = valid.astype(bool)
    nv = int(v.sum())
    out = {"n": len(k), "n_valid": nv, "sum_k": int(k[v].sum())}
    f = features(eig[v]) if nv else np.zeros((0, 4))

    def mean(a):
        return math.fsum(a) / nv if nv else 0.0

    out["mpv"] = mean(eig[v, 2])
    for i, name in enumerate(("linearity", "planarity", "sphericity", "surface_variation")):
        out[name] = mean(f[:, i])
    out["mean_k"] = out["sum_k"] / nv if nv else 0.0
    return out
