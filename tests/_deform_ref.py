"""The numpy model of me_voxel_deformation (include/mapeval_hip.h; csrc/me_deform.hip).

  pair_mask        the pair predicate: d2 >= 0, d2 < max_distance^2 (strict), and the neighbour index names a reference point
  voxel_sums       the 23 sums per voxel by math.fsum (exact to one rounding), with the scale sum |term| the summation bound needs
  fit              pass 3 (k_deform_fit) on given sums, operation by operation; Jacobi / Horn from tests/_globreg_ref.py
  totals           pass 4: the totals over the rows in the device's fixed order (me_reduce.hpp)
  kabsch, direct_residuals   independent checks of the fit (numpy.linalg.svd; the residuals summed over the points)
"""
from __future__ import annotations

import math

import numpy as np

from _errdist_ref import block_order_sum
from _globreg_ref import horn_rotation, jacobi_sym

FIT, ROT_OK, NSUMS = 1, 2, 23
TOTAL_BLOCKS = 1024  # kDfBlocks


def pair_mask(d2, idx, n_ref: int, max_distance: float) -> np.ndarray:
    d2, idx = np.asarray(d2, np.float64), np.asarray(idx, np.int64)
    gate2 = np.float64(max_distance) * np.float64(max_distance)
    return (d2 >= 0.0) & (d2 < gate2) & (idx >= 0) & (idx < n_ref)


def voxel_keys(p, vs: float) -> np.ndarray:
    """voxel_key_of: floor(p / vs), a division."""
    return np.floor(np.asarray(p, np.float64) / np.float64(vs)).astype(np.int64)


def terms(p, q, d2, keys, vs: float) -> np.ndarray:
    """The 23 terms of every point taken as a pair, (n, 23), in the device's arithmetic: o = k vs + 0.5 vs, a = p - o, b = q - o."""
    vs = np.float64(vs)
    o = keys.astype(np.float64) * vs + 0.5 * vs
    a, b = np.asarray(p, np.float64) - o, np.asarray(q, np.float64) - o
    t = np.empty((len(a), NSUMS))
    t[:, 0:3], t[:, 3:6] = a, b
    for r in range(3):
        for c in range(3):
            t[:, 6 + 3 * r + c] = a[:, r] * b[:, c]
    for k, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        t[:, 15 + k] = a[:, r] * a[:, c]
    t[:, 21] = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
    t[:, 22] = d2
    return t


def voxel_sums(p, q, d2, pair, vs: float) -> dict:
    """-> keys (V, 3) ascending, n_points, n_pairs, sums (V, 23) by fsum, scale (V, 23) = fsum |term|, point_voxel (n,) the row of
    every point.  q rows of non-pairs are ignored."""
    p = np.asarray(p, np.float64)
    pair = np.asarray(pair, bool)
    k3 = voxel_keys(p, vs)
    keys, inv = np.unique(k3, axis=0, return_inverse=True)  # (lexicographic: ascending (ix, iy, iz))
    inv = inv.reshape(-1)
    V = len(keys)
    qq = np.where(pair[:, None], np.asarray(q, np.float64), p)
    t = terms(p, qq, np.where(pair, d2, 0.0), k3, vs)
    t[~pair] = 0.0
    order = np.argsort(inv, kind="stable")
    bounds = np.searchsorted(inv[order], np.arange(V + 1))
    sums, scale = np.zeros((V, NSUMS)), np.zeros((V, NSUMS))
    n_pairs = np.zeros(V, np.int64)
    for v in range(V):
        rows = order[bounds[v]:bounds[v + 1]]
        rows = rows[pair[rows]]
        n_pairs[v] = len(rows)
        if len(rows):
            tv = t[rows]
            for k in range(NSUMS):
                col = tv[:, k].tolist()
                sums[v, k] = math.fsum(col)
                scale[v, k] = math.fsum(abs(x) for x in col)
    return dict(keys=keys.astype(np.int32), n_points=np.diff(bounds).astype(np.int64), n_pairs=n_pairs, sums=sums, scale=scale,
                point_voxel=inv)


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def fit(n: int, s, min_pairs: int, min_spread: float):
    """k_deform_fit on one voxel's sums -> (flags, t0[3], u[3], R[9], e0, e_t, e_R), Python floats in the device's order."""
    s = [float(x) for x in s]
    t0, u, R = [0.0] * 3, [0.0] * 3, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    e0 = et = eR = 0.0
    fl = 0
    if n > 0:
        dn = float(n)
        sa, sb = s[0:3], s[3:6]
        ab = [sa[k] / dn for k in range(3)]
        bb = [sb[k] / dn for k in range(3)]
        t0 = [bb[k] - ab[k] for k in range(3)]
        u = list(t0)
        tt = _dot3(t0, t0)
        e0 = s[22]
        rt = s[22] - dn * tt
        et = rt if rt > 0.0 else 0.0
        eR = et
        if n >= min_pairs:
            fl = FIT
            cxx, cxy, cxz = s[15] - (sa[0] * sa[0]) / dn, s[16] - (sa[0] * sa[1]) / dn, s[17] - (sa[0] * sa[2]) / dn
            cyy, cyz, czz = s[18] - (sa[1] * sa[1]) / dn, s[19] - (sa[1] * sa[2]) / dn, s[20] - (sa[2] * sa[2]) / dn
            d, _ = jacobi_sym(3, [cxx, cxy, cxz, cxy, cyy, cyz, cxz, cyz, czz])
            lo01, hi01 = (d[0], d[1]) if d[0] < d[1] else (d[1], d[0])
            mid = lo01 if d[2] < lo01 else (d[2] if d[2] < hi01 else hi01)
            if mid >= dn * (float(min_spread) * float(min_spread)):
                fl |= ROT_OK
                S = [s[6 + 3 * r + c] - (sa[r] * sb[c]) / dn for r in range(3) for c in range(3)]
                R = horn_rotation(S)
                u = [bb[r] - _dot3(R[3 * r:3 * r + 3], ab) for r in range(3)]
                trC = (cxx + cyy) + czz
                vb = s[21] - _dot3(sb, sb) / dn
                trRS = (_dot3(R[0:3], S[0::3]) + _dot3(R[3:6], S[1::3])) + _dot3(R[6:9], S[2::3])  # tr(R S) = sum b'^T R a'
                rr = (trC + vb) - 2.0 * trRS
                eR = rr if rr > 0.0 else 0.0
    return fl, t0, u, R, e0, et, eR


def fit_rows(n_pairs, sums, min_pairs: int, min_spread: float) -> dict:
    V = len(n_pairs)
    out = dict(flags=np.zeros(V, np.uint8), t0=np.zeros((V, 3)), u=np.zeros((V, 3)), R=np.zeros((V, 3, 3)), e0=np.zeros(V), e_t=np.zeros(V),
               e_R=np.zeros(V))
    for v in range(V):
        fl, t0, u, R, e0, et, eR = fit(int(n_pairs[v]), sums[v], min_pairs, min_spread)
        out["flags"][v], out["t0"][v], out["u"][v], out["R"][v] = fl, t0, u, np.reshape(R, (3, 3))
        out["e0"][v], out["e_t"][v], out["e_R"][v] = e0, et, eR
    return out


def _in_order(x) -> float:
    """One value per row -> the total in the order of k_deform_totals + k_red_total: thread (b, t) of min(1024, ceil(V / 256)) blocks
    adds the rows 256 b + t, + the grid, ...; block_sum_256; one block adds the block records t, t + 256, ... and the same tree.
    (Every term here is >= +0: a padding zero changes no bit.)"""
    x = np.asarray(x, np.float64)
    V = len(x)
    nb = min(TOTAL_BLOCKS, max(1, -(-V // 256)))
    grid = 256 * nb
    rounds = max(1, -(-V // grid))
    pad = np.zeros(rounds * grid)
    pad[:V] = x
    per_block = pad.reshape(rounds, nb, 256).transpose(1, 0, 2).reshape(nb, rounds * 256)
    return float(block_order_sum(block_order_sum(per_block)))


def totals(n_pairs, flags, t0, e0, e_t, e_R) -> dict:
    n_pairs, flags = np.asarray(n_pairs, np.int64), np.asarray(flags, np.uint8)
    t0 = np.asarray(t0, np.float64)
    dn = n_pairs.astype(np.float64)
    tt = (t0[:, 0] * t0[:, 0] + t0[:, 1] * t0[:, 1]) + t0[:, 2] * t0[:, 2]
    tn = np.sqrt(tt)
    isfit = (flags & FIT) != 0
    out = dict(n_voxels=len(n_pairs), n_with_pairs=int((n_pairs > 0).sum()), n_fit=int(isfit.sum()), n_rot=int(((flags & ROT_OK) != 0).sum()),
               n_pairs=int(n_pairs.sum()), sum_n_t0=_in_order(dn * tn), sum_n_t0sq=_in_order(dn * tt), sum_e0=_in_order(e0),
               sum_e_t=_in_order(e_t), sum_e0_fit=_in_order(np.where(isfit, e0, 0.0)), sum_e_R=_in_order(np.where(isfit, e_R, 0.0)))
    if isfit.any():
        m = tn[isfit].max()
        out["max_row"] = int(np.flatnonzero(isfit & (tn == m))[0])  # ties: the smallest row
        out["max_disp"] = float(m)
    else:
        out["max_row"], out["max_disp"] = -1, 0.0
    return out


def kabsch(a, b) -> np.ndarray:
    """The rotation of the least-squares rigid fit a -> b by SVD, determinant fixed (independent of Horn's closed form)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    H = (a - a.mean(0)).T @ (b - b.mean(0))
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    return Vt.T @ D @ U.T


def direct_residuals(a, b, R):
    """(e_t, e_R) summed over the points: sum |a' + t0 - b'|^2 - i.e. sum |a' - b'|^2 about the means - and sum |R a' - b'|^2."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ac, bc = a - a.mean(0), b - b.mean(0)
    et = math.fsum(((ac - bc) ** 2).sum(1).tolist())
    eR = math.fsum(((ac @ np.asarray(R, np.float64).reshape(3, 3).T - bc) ** 2).sum(1).tolist())
    return et, eR
