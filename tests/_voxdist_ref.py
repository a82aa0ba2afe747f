"""The numpy model of me_voxel_distances (include/mapeval_hip.h; csrc/me_voxdist.hip).

rows()        the voxel lists from floor(p / vs) and the original index, the min_pts gate on the full populations, the stride rule
mmd_row()     k = exp(-(d2 * g)) formed as the kernel forms it (one multiplication, then np.exp), the three sums by math.fsum (exact)
gauss_row()   k_vd_gauss operation by operation, floats only, with the Python jacobi_sym the other models share
gauss_formula() the same four numbers from numpy's eigh / inv / slogdet: the formula-level check of the model
scene()       the hand-built clouds of tests/test_gpu_voxdist_edges.py
"""
from __future__ import annotations

import math

import numpy as np

from _deform_ref import jacobi_sym

TILE = 256  # ME_TUNE_VOXDIST_TILE


# ------------------------------------------------------------------------------------------------------------ rows and point lists
def stride_rule(n: int, max_points: int):
    """-> (s, used): every s-th point of the list, starting at the first"""
    s = 1
    if max_points > 0 and n > max_points:
        s = -(-n // max_points)
    return s, -(-n // s)


def voxel_lists(p, vs: float) -> dict:
    """key (ix, iy, iz) -> the original indices of the voxel's points, ascending"""
    k = np.floor(np.asarray(p, np.float64) / vs).astype(np.int64)
    out: dict = {}
    for i, key in enumerate(k.tolist()):
        out.setdefault(tuple(key), []).append(i)
    return out


def rows(est, gt, vs: float, min_pts: int, max_points: int):
    """-> list of (key, idx_est_used, idx_gt_used, pop_est, pop_gt) in ascending key order"""
    le, lg = voxel_lists(est, vs), voxel_lists(gt, vs)
    out = []
    for key in sorted(set(le) & set(lg)):
        a, b = le[key], lg[key]
        if len(a) < min_pts or len(b) < min_pts:
            continue
        sa, _ = stride_rule(len(a), max_points)
        sb, _ = stride_rule(len(b), max_points)
        out.append((key, a[::sa], b[::sb], len(a), len(b)))
    return out


# ----------------------------------------------------------------------------------------------------------------------------- MMD
def _kernel(A, B, g: float) -> np.ndarray:
    dx = A[:, None, 0] - B[None, :, 0]
    dy = A[:, None, 1] - B[None, :, 1]
    dz = A[:, None, 2] - B[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    with np.errstate(under="ignore"):
        return np.exp(-(d2 * g))


def mmd_row(X, Y, sigma: float) -> dict:
    """the three sums (exact, then rounded once), the two estimates and, for the tolerances, the absolute sum of their terms"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    n, m = X.shape[0], Y.shape[0]
    g = 1.0 / (2.0 * sigma * sigma)
    kxx, kyy, kxy = _kernel(X, X, g), _kernel(Y, Y, g), _kernel(X, Y, g)
    sxx = math.fsum(kxx[np.triu_indices(n, 1)])
    syy = math.fsum(kyy[np.triu_indices(m, 1)])
    sxy = math.fsum(kxy.ravel())
    dn, dm = float(n), float(m)
    cross = (2.0 * sxy) / (dn * dm)
    ux, uy = (2.0 * sxx) / (dn * (dn - 1.0)), (2.0 * syy) / (dm * (dm - 1.0))
    bx, by = (dn + 2.0 * sxx) / (dn * dn), (dm + 2.0 * syy) / (dm * dm)
    return dict(ksum=(sxx, syy, sxy), terms=(n * (n - 1) // 2, m * (m - 1) // 2, n * m), u=(ux + uy) - cross, b=(bx + by) - cross,
                u_abs=ux + uy + cross, b_abs=bx + by + cross)


# ---------------------------------------------------------------------------------------------------------------- the closed forms
def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _matmul(A, B):
    return [(A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c] for r in range(3) for c in range(3)]


def _compose(V, w):
    return [((V[3 * r] * w[0]) * V[3 * c] + (V[3 * r + 1] * w[1]) * V[3 * c + 1]) + (V[3 * r + 2] * w[2]) * V[3 * c + 2]
            for r in range(3) for c in range(3)]


def _decompose(Cm, floor: float):
    A = [0.5 * (Cm[3 * r + c] + Cm[3 * c + r]) for r in range(3) for c in range(3)]
    lam, V = jacobi_sym(3, A)
    lam = [floor if x < floor else x for x in lam]
    return lam, V, (math.log(lam[0]) + math.log(lam[1])) + math.log(lam[2])


def _quad(P, d):
    return _dot3(d, [_dot3(P[0:3], d), _dot3(P[3:6], d), _dot3(P[6:9], d)])


def _trace_prod(P, Q):
    return (_dot3(P[0:3], [Q[0], Q[3], Q[6]]) + _dot3(P[3:6], [Q[1], Q[4], Q[7]])) + _dot3(P[6:9], [Q[2], Q[5], Q[8]])


def gauss_row(n_e: int, mu_e, sig_e, n_g: int, mu_g, sig_g, floor: float = 1e-6) -> dict:
    """sig_*: the 9 entries AS STORED (M2 / (n - 1)^2, n > 10).  -> values (kl_eg, kl_ge, bd, w2) and `abs`, the sum of the absolute
    terms of each column (W2: of D, carried through the square root by the caller)"""
    fe, fg = float(n_e - 1), float(n_g - 1)
    Ce = [float(x) * fe for x in np.asarray(sig_e).ravel()]
    Cg = [float(x) * fg for x in np.asarray(sig_g).ravel()]
    d = [float(mu_g[k]) - float(mu_e[k]) for k in range(3)]
    le, Ve, lde = _decompose(Ce, floor)
    lg, Vg, ldg = _decompose(Cg, floor)
    Se, Sg = _compose(Ve, le), _compose(Vg, lg)
    Ie, Ig = _compose(Ve, [1.0 / x for x in le]), _compose(Vg, [1.0 / x for x in lg])
    t_eg, q_eg = _trace_prod(Ig, Se), _quad(Ig, d)
    t_ge, q_ge = _trace_prod(Ie, Sg), _quad(Ie, d)
    kl_eg = 0.5 * ((((t_eg + q_eg) - 3.0) + ldg) - lde)
    kl_ge = 0.5 * ((((t_ge + q_ge) - 3.0) + lde) - ldg)
    Sm = [0.5 * (Se[k] + Sg[k]) for k in range(9)]
    ls, Vs, lds = _decompose(Sm, floor)
    Is = _compose(Vs, [1.0 / x for x in ls])
    q_s = _quad(Is, d)
    bd = 0.125 * q_s + 0.5 * (lds - 0.5 * (lde + ldg))
    He = _compose(Ve, [math.sqrt(x) for x in le])
    Mm = _matmul(_matmul(He, Sg), He)
    A = [0.5 * (Mm[3 * r + c] + Mm[3 * c + r]) for r in range(3) for c in range(3)]
    lm, _ = jacobi_sym(3, A)
    w = [math.sqrt(x if x > 0.0 else 0.0) for x in lm]
    tre, trg, trm = (le[0] + le[1]) + le[2], (lg[0] + lg[1]) + lg[2], (w[0] + w[1]) + w[2]
    dd = _dot3(d, d)
    D = ((dd + tre) + trg) - 2.0 * trm
    logs = sum(abs(math.log(x)) for x in le + lg)
    a_kl_eg = 0.5 * (abs(t_eg) + abs(q_eg) + 3.0 + logs)
    a_kl_ge = 0.5 * (abs(t_ge) + abs(q_ge) + 3.0 + logs)
    a_bd = 0.125 * abs(q_s) + 0.5 * (sum(abs(math.log(x)) for x in ls) + 0.5 * logs)
    a_D = dd + tre + trg + 2.0 * trm
    return dict(values=(kl_eg, kl_ge, bd, math.sqrt(D if D > 0.0 else 0.0)), abs=(a_kl_eg, a_kl_ge, a_bd, a_D), D=D)


def gauss_formula(mu_e, Ce, mu_g, Cg):
    """the four formulas from numpy's linear algebra, on covariances that need no floor"""
    Ce, Cg = np.asarray(Ce, np.float64), np.asarray(Cg, np.float64)
    d = np.asarray(mu_g, np.float64) - np.asarray(mu_e, np.float64)

    def kl(A, B):  # KL(N(., A) || N(., B))
        Bi = np.linalg.inv(B)
        return 0.5 * (np.trace(Bi @ A) + d @ Bi @ d - 3.0 + np.linalg.slogdet(B)[1] - np.linalg.slogdet(A)[1])

    S = 0.5 * (Ce + Cg)
    bd = 0.125 * d @ np.linalg.inv(S) @ d + 0.5 * (np.linalg.slogdet(S)[1] - 0.5 * (np.linalg.slogdet(Ce)[1] + np.linalg.slogdet(Cg)[1]))
    w, V = np.linalg.eigh(Ce)
    H = (V * np.sqrt(w)) @ V.T
    lm = np.linalg.eigvalsh(H @ Cg @ H)
    D = d @ d + np.trace(Ce) + np.trace(Cg) - 2.0 * np.sqrt(np.maximum(lm, 0.0)).sum()
    return kl(Ce, Cg), kl(Cg, Ce), bd, math.sqrt(max(0.0, D))


# ------------------------------------------------------------------------------------------------------------------- the GPU scene
MIN_PTS = 11
VS = 1.0
SIGMAS = (0.25, 0.05, 0.0125, 1.0)  # 0.0125: g = 3200, a pair more than 0.483 apart underflows (d2 g > 745.2), one 0.474 apart is a denormal

# (key, n_est, n_gt): used counts at T = 256 around the tile edge, around the wave edge, one tile and more than one tile per side
ROW_VOXELS = [((-2, -1, 0), 11, 63), ((-1, 0, -3), 64, 65), ((0, 0, 0), 255, 256), ((0, 1, 0), 257, 255), ((1, -1, 2), 256, 257),
              ((2, 0, 0), 1025, 11), ((3, 3, -1), 65, 1025), ((4, 0, 1), 63, 64)]
NO_ROW_VOXELS = [((-5, 0, 0), 40, 0), ((6, 0, 0), 0, 40), ((0, -4, 0), 10, 300), ((0, 5, 0), 300, 10), ((7, 7, 7), 10, 10)]
PLANAR = (-1, 0, -3)   # its est points lie in one plane: the eigenvalue floor bites
EDGE = (-2, -1, 0)     # holds the duplicate point, the underflowing pair and the denormal pair


def scene(seed: int = 7):
    """-> est, gt (shuffled original order), the keys that must give a row"""
    rng = np.random.default_rng(seed)
    pe, pg = [], []
    for key, ne, ng in ROW_VOXELS + NO_ROW_VOXELS:
        o = np.array(key, np.float64) * VS
        a = o + 0.05 + 0.9 * rng.random((ne, 3))
        b = o + 0.05 + 0.9 * rng.random((ng, 3))
        if key == PLANAR:
            a[:, 2] = o[2] + 0.5  # a plane z = const: one eigenvalue of its covariance is 0
        if key == EDGE:
            # the ground truth: a cluster in one corner; the map: point 0 a duplicate of a ground-truth point (d2 = 0, k = 1), point 1
            # 0.49 from everything of the ground truth along x at least (underflow at sigma 0.0125), point 2 at the denormal distance
            b = o + np.array([0.1, 0.1, 0.1]) + 0.01 * rng.random((ng, 3))
            b[0] = o + np.array([0.1, 0.1, 0.1])
            a[0] = b[0]
            a[1] = b[0] + np.array([0.6, 0.0, 0.0])
            dn = math.sqrt(720.0 / (1.0 / (2.0 * SIGMAS[2] ** 2)))  # d2 g = 720: exp(-720) = 2.0e-313, a denormal
            a[2] = b[0] + np.array([0.0, 0.0, dn])
        pe.append(a)
        pg.append(b)
    est, gt = np.concatenate(pe), np.concatenate(pg)
    est, gt = est[rng.permutation(est.shape[0])], gt[rng.permutation(gt.shape[0])]
    return np.ascontiguousarray(est), np.ascontiguousarray(gt), sorted(k for k, _, _ in ROW_VOXELS)
