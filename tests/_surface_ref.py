"""numpy models of me_radius_normals (csrc/me_localgeom.hip) and me_nn_surface_error (csrc/me_surface.hip).

Normals: the neighbours by brute force with the library's own expression, the covariance centred first and summed in extended
precision (as tests/_localgeom_ref.py does), eigenpairs by numpy.linalg.eigh.  The device's covariance is within B = 8 k 2^-53 r^2 of
the exact one in 2-norm, so its normal n is the exact minimiser of C + E with |E| <= B:
    n^T C n <= l3 + 2 B            (the Rayleigh quotient; + 2 B for Jacobi's own residual: rayleigh_tol = 4 B), and
    |n x n_model| <= 4 B / (l2 - l3)   (Davis-Kahan with the same margin) wherever that is <= 1e-6.
Neither needs an eigen-gap heuristic; the first holds on every valid point.

Surface error: the expressions of include/mapeval_hip.h written in numpy in the same order — e, t2 and c are bit-identical to the
device's and every count is exact; the sums are compared with math.fsum."""
import math

import numpy as np

EPS = 2.0 ** -53
_LD = np.longdouble


def cov_bound(k, r):
    """B = 8 k 2^-53 r^2"""
    return 8.0 * np.asarray(k, np.float64) * EPS * r * r


def neighbours(xyz, i, r):
    """indices j != i with ((dx*dx + dy*dy) + dz*dz) < r*r, d = p_j - p_i (fp64, no FMA); coincident duplicates of i stay"""
    d = xyz - xyz[i]
    inside = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r * r
    inside[i] = False
    return np.nonzero(inside)[0]


def covariance(xyz, i, nb):
    """the sample covariance of the offsets p_j - p_i, centred first, every sum by math.fsum on longdouble-centred terms"""
    e = (xyz[nb] - xyz[i]).astype(_LD)
    k = len(nb)
    mean = np.array([math.fsum(e[:, a].astype(np.float64)) for a in range(3)], _LD) / _LD(k)
    # (the offsets are fp64 values: their fsum is exact; the centring and the products are carried in longdouble)
    e = e - mean
    c = np.zeros((3, 3))
    for a in range(3):
        for b in range(a, 3):
            c[a, b] = c[b, a] = float(np.sum(e[:, a] * e[:, b], dtype=_LD) / _LD(k - 1))
    return c


def radius_normals(xyz, r, min_k=5):
    """-> dict: k[n] int32, have[n] (k >= min_k), cov[n,3,3], eig[n,3] ascending (l3 first, UNclamped), normal[n,3] (unit, sign
    arbitrary; zeros where k < min_k), valid[n] = have & (l1 > 0)"""
    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    k = np.zeros(n, np.int32)
    cov = np.zeros((n, 3, 3))
    for i in range(n):
        nb = neighbours(xyz, i, r)
        k[i] = len(nb)
        if k[i] >= 2:
            cov[i] = covariance(xyz, i, nb)
    have = k >= min_k
    eig = np.zeros((n, 3))
    nrm = np.zeros((n, 3))
    if have.any():
        w, v = np.linalg.eigh(cov[have])
        eig[have] = w
        nrm[have] = v[:, :, 0]
    valid = have & (np.maximum(eig[:, 2], 0.0) > 0.0)
    return {"k": k, "have": have, "cov": cov, "eig": eig, "normal": nrm, "valid": valid}


def rayleigh(cov, n):
    """n^T C n per row, in longdouble"""
    c = cov.astype(_LD)
    v = n.astype(_LD)
    return np.einsum("ia,iab,ib->i", v, c, v).astype(np.float64)


def norm_ld(n):
    v = n.astype(_LD)
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def cross_norm(a, b):
    return np.linalg.norm(np.cross(a, b), axis=1)


def gate_pass(d2, gate, gate_mode):
    """me_nn_stats' gate: mode 0 d2 <= gate (unsquared), mode 1 d2 < gate * gate; gate < 0: everything"""
    if gate < 0:
        return np.ones(len(d2), bool)
    return d2 < gate * gate if gate_mode == 1 else d2 <= gate


def surface_error(q_xyz, r_xyz, idx, d2, r_nrm, q_nrm=None, taus=(), cos_min=(), gate=-1.0, gate_mode=0):
    """The model of me_nn_surface_error: per-point e / c in cloud order (-1 where unused) and the dict of counts, sums (math.fsum),
    max_e / argmax."""
    n = len(q_xyz)
    idx = np.asarray(idx, np.int64)
    ok_j = (idx >= 0) & (idx < len(r_xyz))
    j = np.where(ok_j, idx, 0)
    nr = r_nrm[j]
    used = (d2 >= 0.0) & gate_pass(d2, gate, gate_mode) & ok_j & ~np.all(nr == 0.0, axis=1)
    d = q_xyz - r_xyz[j]
    e = np.abs((nr[:, 0] * d[:, 0] + nr[:, 1] * d[:, 1]) + nr[:, 2] * d[:, 2])
    t2 = np.maximum(d2 - e * e, 0.0)
    if q_nrm is None:
        nused = np.zeros(n, bool)
        c = np.zeros(n)
    else:
        nused = used & ~np.all(q_nrm == 0.0, axis=1)
        c = np.abs((q_nrm[:, 0] * nr[:, 0] + q_nrm[:, 1] * nr[:, 1]) + q_nrm[:, 2] * nr[:, 2])
    e_out = np.where(used, e, -1.0)
    c_out = np.where(nused, c, -1.0)
    out = {"n_query": int((d2 >= 0.0).sum()), "n_used": int(used.sum()), "n_normal_used": int(nused.sum()),
           "sum_e": math.fsum(e[used]), "sum_e2": math.fsum((e * e)[used]), "sum_t2": math.fsum(t2[used]), "sum_c": math.fsum(c[nused]),
           "max_e": 0.0, "argmax": -1, "t2": np.where(used, t2, -1.0)}
    if used.any():
        out["max_e"] = float(e[used].max())
        out["argmax"] = int(np.nonzero(used & (e == out["max_e"]))[0][0])
    out["n_within"] = np.array([int((used & (e <= t)).sum()) for t in taus], np.int64)
    out["sum_e2_within"] = np.array([math.fsum((e * e)[used & (e <= t)]) for t in taus], np.float64)
    out["n_angle"] = np.array([int((nused & (c >= cm)).sum()) for cm in cos_min], np.int64)
    return e_out, c_out, out


def nearest_rank(p, n_used):
    """me_nn_error_distribution's rank: min(n - 1, max(0, ceil(p n) - 1))"""
    return min(n_used - 1, max(0, int(math.ceil(p * float(n_used))) - 1)) if n_used > 0 else -1
