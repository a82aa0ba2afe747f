"""Brute-force model of me_m3c2 (include/mapeval_hip.h) over all pairs, in numpy.

The membership test restates the device's expression in fp64 with the same association (numpy evaluates one rounded operation per
ufunc call: no FMA), so the sets are the device's bit for bit.  The moments S = sum t and Q = sum t*t are summed EXACTLY over those
sets (fractions of the fp64 values of t), and mean, variance and distance are formed exactly and rounded once at the end."""
from fractions import Fraction

import numpy as np


def members(q, nrm, pts, rp, L):
    """inside (bool[len(pts)]) and t (float64[len(pts)]) of the cylinder of core point q with stored normal nrm"""
    dx = pts[:, 0] - q[0]
    dy = pts[:, 1] - q[1]
    dz = pts[:, 2] - q[2]
    d2 = (dx * dx + dy * dy) + dz * dz
    t = (nrm[0] * dx + nrm[1] * dy) + nrm[2] * dz
    return (np.abs(t) < L) & (d2 - t * t < rp * rp), t


def _moments(t):
    s = Fraction(0)
    q = Fraction(0)
    for v in t:
        f = Fraction(float(v))
        s += f
        q += f * f
    return s, q


def m3c2(own, other, normals, rp, L, min_points=5, reg=0.0, mask=None, exact=True):
    """The per-point result of me_m3c2 with `own` as the query cloud: dict of n_own, n_other (int32), valid, significant (bool), dist,
    var_own, var_other, lod (float64; zeros where invalid or masked out; the counts are kept on invalid core points).  exact=False skips
    the exact moments (counts and validity only: dist, var and lod stay 0)."""
    own = np.ascontiguousarray(own, np.float64).reshape(-1, 3)
    other = np.ascontiguousarray(other, np.float64).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    n = len(own)
    out = {"n_own": np.zeros(n, np.int32), "n_other": np.zeros(n, np.int32), "valid": np.zeros(n, bool), "significant": np.zeros(n, bool),
           "dist": np.zeros(n), "var_own": np.zeros(n), "var_other": np.zeros(n), "lod": np.zeros(n)}
    for i in range(n):
        if mask is not None and not mask[i]:
            continue
        in0, t0 = members(own[i], normals[i], own, rp, L)
        in1, t1 = members(own[i], normals[i], other, rp, L)
        n0, n1 = int(in0.sum()), int(in1.sum())
        out["n_own"][i], out["n_other"][i] = n0, n1
        if not normals[i].any() or n0 < min_points or n1 < min_points:
            continue
        out["valid"][i] = True
        if not exact:
            continue
        s0, q0 = _moments(t0[in0])
        s1, q1 = _moments(t1[in1])
        v0 = (q0 - s0 * s0 / n0) / (n0 - 1)
        v1 = (q1 - s1 * s1 / n1) / (n1 - 1)
        dist = s1 / n1 - s0 / n0
        out["dist"][i] = float(dist)
        out["var_own"][i] = float(v0)
        out["var_other"][i] = float(v1)
        lod = 1.96 * (float(v0 / n0 + v1 / n1) ** 0.5 + reg)
        out["lod"][i] = lod
        out["significant"][i] = abs(float(dist)) > lod
    return out
