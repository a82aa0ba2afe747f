"""Brute-force model of me_mesh_distance and me_mesh_sample (include/mapeval_hip.h) in numpy: every query
against every triangle, in chunks.  The closest-point routine restates the device's sequence of fp64 operations one by one (numpy
neither contracts nor reorders them), so d2, triangle, region and closest point are compared for EQUALITY with the device."""
from __future__ import annotations

import math

import numpy as np

import _perturb_ref as P

FACE, EDGE_AB, EDGE_BC, EDGE_CA, VERT_A, VERT_B, VERT_C = range(7)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _clamp01(x):
    return np.fmin(np.fmax(x, 0.0), 1.0)  # (fmax(NaN, 0) = 0)


def _d2(p, c):
    d = p - c
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def areas(vertices, triangles):
    """(area[T], degenerate[T]): area = 0.5 sqrt((nx nx + ny ny) + nz nz), n = (B - A) x (C - A); degenerate iff n == 0 exactly."""
    v = np.asarray(vertices, np.float64)[np.asarray(triangles)]
    n = cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return 0.5 * np.sqrt(_dot(n, n)), (n == 0.0).all(axis=1)


def _segment(p, p0, p1, code_edge, code0, code1):
    e = p1 - p0
    l = _dot(e, e)
    t = _dot(e, p - p0)
    with np.errstate(all="ignore"):
        s = t / l
    c = np.where((t <= 0.0)[..., None], p0, np.where((t >= l)[..., None], p1, p0 + s[..., None] * e))
    r = np.where(t <= 0.0, code0, np.where(t >= l, code1, code_edge))
    return c, r


def closest(p, a, b, g, degenerate=None):
    """Broadcasting closest point of the triangles (a, b, g) to the points p (all (..., 3)): (d2, closest, region)."""
    p, a, b, g = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (p, a, b, g)))
    ab, ac = b - a, g - a
    d1, d2 = _dot(ab, p - a), _dot(ac, p - a)
    d3, d4 = _dot(ab, p - b), _dot(ac, p - b)
    d5, d6 = _dot(ab, p - g), _dot(ac, p - g)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    with np.errstate(all="ignore"):
        t_ab = _clamp01(d1 / (d1 - d3))
        t_ca = _clamp01(d2 / (d2 - d6))
        t_bc = _clamp01((d4 - d3) / ((d4 - d3) + (d5 - d6)))
        den = (va + vb) + vc
        s = _clamp01(vb / den)
        t = np.fmin(np.fmax(vc / den, 0.0), 1.0 - s)
    conds = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), (d6 >= 0.0) & (d5 <= d6),
             (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), (va <= 0.0) & (d4 - d3 >= 0.0) & (d5 - d6 >= 0.0)]
    pts = [a, b, a + t_ab[..., None] * ab, g, a + t_ca[..., None] * ac, b + t_bc[..., None] * (g - b)]
    codes = [VERT_A, VERT_B, EDGE_AB, VERT_C, EDGE_CA, EDGE_BC]
    c = (a + s[..., None] * ab) + t[..., None] * ac
    r = np.full(d1.shape, FACE, np.int64)
    for cond, pt, code in reversed(list(zip(conds, pts, codes))):  # the FIRST condition that holds decides
        c = np.where(cond[..., None], pt, c)
        r = np.where(cond, code, r)
    dd = _d2(p, c)
    if degenerate is not None and np.any(degenerate):
        deg = np.broadcast_to(degenerate, dd.shape)
        sc, sr = _segment(p, a, b, EDGE_AB, VERT_A, VERT_B)
        sd = _d2(p, sc)
        for p0, p1, codes3 in ((b, g, (EDGE_BC, VERT_B, VERT_C)), (g, a, (EDGE_CA, VERT_C, VERT_A))):
            qc, qr = _segment(p, p0, p1, *codes3)
            qd = _d2(p, qc)
            better = qd < sd
            sc, sr, sd = np.where(better[..., None], qc, sc), np.where(better, qr, sr), np.where(better, qd, sd)
        c, r, dd = np.where(deg[..., None], sc, c), np.where(deg, sr, r), np.where(deg, sd, dd)
    return dd, c, r


def distance(points, vertices, triangles, chunk=256):
    """The per-point result of me_mesh_distance: dict of d2, tri (the smallest index among the bitwise-minimal d2), region, closest,
    signed_d (NaN outside the face region)."""
    pts = np.asarray(points, np.float64)
    tri = np.asarray(triangles)
    v = np.asarray(vertices, np.float64)[tri]  # (T, 3, 3); unreferenced vertices never enter
    _, deg = areas(vertices, tri)
    n = len(pts)
    out = {"d2": np.empty(n), "tri": np.empty(n, np.int32), "region": np.empty(n, np.uint8), "closest": np.empty((n, 3)),
           "signed_d": np.full(n, np.nan)}
    for s in range(0, n, chunk):
        p = pts[s:s + chunk]
        dd, c, r = closest(p[:, None, :], v[None, :, 0], v[None, :, 1], v[None, :, 2], deg[None, :])
        k = np.argmin(dd, axis=1)  # (the first index of the minimum)
        rows = np.arange(len(p))
        out["d2"][s:s + chunk], out["tri"][s:s + chunk], out["region"][s:s + chunk] = dd[rows, k], k, r[rows, k]
        out["closest"][s:s + chunk] = c[rows, k]
        w = v[k]
        nn = cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0])
        with np.errstate(all="ignore"):
            sd = _dot(p - c[rows, k], nn) / np.sqrt(_dot(nn, nn))
        out["signed_d"][s:s + chunk] = np.where(r[rows, k] == FACE, sd, np.nan)
    return out


def totals(res, max_distance=math.inf, thresholds=()):
    """The gate and the counts of me_mesh_out from a per-point result; the sums with math.fsum (the device's are compared to 1e-9)."""
    d2 = res["d2"]
    m = d2 <= max_distance * max_distance
    d = np.sqrt(d2)
    face = m & (res["region"] == FACE)
    worst = -1
    if m.any():
        worst = int(np.flatnonzero(m & (d == d[m].max()))[0])
    return {"n_query": len(d2), "n_matched": int(m.sum()), "n_face": int(face.sum()), "sum_d": math.fsum(d[m]), "sum_d2": math.fsum(d2[m]),
            "max": float(d[m].max()) if m.any() else 0.0, "worst_index": worst,
            "n_within": np.array([int((m & (d2 <= t * t)).sum()) for t in thresholds], np.int64),
            "sum_signed": math.fsum(res["signed_d"][face]), "sum_abs_signed": math.fsum(np.abs(res["signed_d"][face]))}


def sample(vertices, triangles, n_points, seed):
    """me_mesh_sample: (points (n, 3), triangle index (n,)), bit for bit."""
    v = np.asarray(vertices, np.float64)[np.asarray(triangles)]
    area, _ = areas(vertices, triangles)
    cum = np.cumsum(area)
    w = P.philox4x64_10(np.arange(n_points, dtype=np.uint64), 0, 0, 0, int(seed), 0)
    u = P.u01(w[0]) * cum[-1]
    t = np.minimum(np.searchsorted(cum, u, side="right"), len(cum) - 1)  # the first index whose cumulative area exceeds u
    r1, r2 = np.sqrt(P.u01(w[1])), P.u01(w[2])
    wa, wb, wc = (1.0 - r1)[:, None], (r1 * (1.0 - r2))[:, None], (r1 * r2)[:, None]
    return (wa * v[t, 0] + wb * v[t, 1]) + wc * v[t, 2], t


MORTON_BITS = 21


def _spread21(x):
    out = np.zeros(len(x), np.uint64)
    for b in range(MORTON_BITS):
        out |= ((x >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton_codes(vertices, triangles):
    """k_mesh_codes with the origin and the cell edge me_mesh_upload passes it: the Morton code of every triangle's centroid on the
    2^21 lattice over the bounding box of the referenced vertices."""
    v = np.asarray(vertices, np.float64)[np.asarray(triangles)]
    corners = v.reshape(-1, 3)
    lo, hi = corners.min(0), corners.max(0)
    extent = float((hi - lo).max())
    h = math.ldexp(extent, -MORTON_BITS) * (1.0 + 2.0 ** -20) if extent > 0 else 1.0
    c = ((v[:, 0] + v[:, 1]) + v[:, 2]) / 3.0
    g = np.fmin(np.fmax(np.floor((c - lo) / h), 0.0), 2097151.0).astype(np.uint64)
    return _spread21(g[:, 0]) | (_spread21(g[:, 1]) << np.uint64(1)) | (_spread21(g[:, 2]) << np.uint64(2))


def morton_rank(vertices, triangles):
    """rank[t]: where the caller's triangle t stands after the upload's stable sort by Morton code (a leaf is 8 consecutive ranks)."""
    order = np.argsort(morton_codes(vertices, triangles), kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank
