"""Brute-force model of me_m3c2 (include/mapeval_hip.h) over all pairs, in numpy.

The membership test restates the device's expression in fp64 with the same association (numpy evaluates one rounded operation per
ufunc call: no FMA), so the sets are the device's bit for bit.  The moments S = sum t and Q = sum t*t are summed EXACTLY over those
sets (fractions of the fp64 values of t), and mean, variance and distance are formed exactly and rounded once at the end."""
import math
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


# ---- the device's own arithmetic, restated (tests/_m3c2_edge_cases.py) -----------------------------------------------------------
def sequential_sum(terms):
    """one accumulator, one rounded fp64 addition per term, in the order given: S += t as a lane of k_m3_stream adds"""
    s = 0.0
    for v in terms:
        s = s + float(v)
    return s


def order_free(t):
    """True where the sequential sums of t and of t*t are the same number in every order of the terms: all terms are equal (the
    same additions whatever the order), or every t is a multiple of 2^-20, so that every product is exact, every partial sum of t
    is a multiple of 2^-20 and every partial sum of t*t a multiple of 2^-40, and the sum of t*t stays below 2^13 (an integer below
    2^53 in units of 2^-40: no partial sum ever rounds)."""
    t = np.asarray(t, np.float64)
    if len(t) == 0 or (t == t[0]).all():
        return True
    k = t * 2.0 ** 20
    return bool((k == np.rint(k)).all() and np.abs(t).sum() < 2.0 ** 13 and (t * t).sum() < 2.0 ** 13)


def raw_variance(n, S, Q):
    """(Q - S*S/n) / (n - 1) as k_m3_final forms it before its clamp: one rounded operation at a time, no FMA"""
    nf = float(n)
    return (Q - S * S / nf) / (nf - 1.0)


def final_fp64(n0, S0, Q0, n1, S1, Q1, reg):
    """dist, var_own, var_other, lod, significant of a valid core point from its counts and moments, operation by operation as
    k_m3_final (fp64, no FMA; the square root is correctly rounded on both sides)"""
    no, nt = float(n0), float(n1)
    dist = S1 / nt - S0 / no
    r0, r1 = raw_variance(n0, S0, Q0), raw_variance(n1, S1, Q1)
    vo = r0 if r0 > 0.0 else 0.0
    vt = r1 if r1 > 0.0 else 0.0
    lod = 1.96 * (math.sqrt(vo / no + vt / nt) + reg)
    return dist, vo, vt, lod, abs(dist) > lod


def m3c2_fp64(own, other, normals, rp, L, min_points=5, reg=0.0, mask=None):
    """The result of me_m3c2 as m3c2() returns it, with S and Q summed SEQUENTIALLY in fp64 (in the order of the cloud sorted by x) and the values formed by
    final_fp64: the device's bits wherever the sums do not depend on the order of their terms, which "order_free" (bool per point)
    says for the two member sets of every valid core point.  Also "raw_own" / "raw_other", the variances before the clamp.
    The candidates of a core point are cut to the slab |dx| <= 2 R of a cloud sorted by x once (R = sqrt(L*L + rp*rp): a member has
    d2 < rp*rp + t*t < R*R up to rounding, so none lies outside), which keeps a large cloud with few core points cheap."""
    own = np.ascontiguousarray(own, np.float64).reshape(-1, 3)
    other = np.ascontiguousarray(other, np.float64).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    n = len(own)
    out = {"n_own": np.zeros(n, np.int32), "n_other": np.zeros(n, np.int32), "valid": np.zeros(n, bool), "significant": np.zeros(n, bool),
           "dist": np.zeros(n), "var_own": np.zeros(n), "var_other": np.zeros(n), "lod": np.zeros(n), "raw_own": np.zeros(n),
           "raw_other": np.zeros(n), "order_free": np.ones(n, bool)}
    reach = 2.0 * float(np.hypot(L, rp))
    sorted_by_x = []
    for pts in (own, other):
        o = np.argsort(pts[:, 0], kind="stable")
        sorted_by_x.append((np.ascontiguousarray(pts[o]), np.ascontiguousarray(pts[o, 0])))
    core = range(n) if mask is None else np.flatnonzero(np.asarray(mask) != 0)
    for i in core:
        sets = []
        for pts, xs in sorted_by_x:
            a, b = np.searchsorted(xs, own[i, 0] - reach, "left"), np.searchsorted(xs, own[i, 0] + reach, "right")
            inside, t = members(own[i], normals[i], pts[a:b], rp, L)
            sets.append(t[inside])
        t0, t1 = sets
        n0, n1 = len(t0), len(t1)
        out["n_own"][i], out["n_other"][i] = n0, n1
        if not normals[i].any() or n0 < min_points or n1 < min_points:
            continue
        out["valid"][i] = True
        out["order_free"][i] = order_free(t0) and order_free(t1)
        S0, Q0, S1, Q1 = sequential_sum(t0), sequential_sum(t0 * t0), sequential_sum(t1), sequential_sum(t1 * t1)
        out["raw_own"][i], out["raw_other"][i] = raw_variance(n0, S0, Q0), raw_variance(n1, S1, Q1)
        out["dist"][i], out["var_own"][i], out["var_other"][i], out["lod"][i], out["significant"][i] = final_fp64(n0, S0, Q0, n1, S1, Q1, reg)
    return out
