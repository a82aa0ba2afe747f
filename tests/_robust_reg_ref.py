"""Plain numpy model of the robust registration step (me_reg.hip: k_lsq_sums_robust<MODE, KERNEL>, k_info_sums; icp.py: _icp_lsq with
a kernel, icp_multi_scale), next to tests/_reg_ref.py and independent of oracle/.

The weights restate Open3D's RobustKernel.cpp [upstream] from their definitions with + - * / fabs fmin fmax only, the generalized rows
restate W = (Ct + Cs)^(-1/2) through the Jacobi decomposition of csrc/me_horn.hpp (jacobi_sym, restated scalar in _globreg_ref.py and
vectorised here, operation by operation), so every per-correspondence term equals the device's bit for bit and the only difference
left is the order of the sum (R.lsq_bound)."""
from __future__ import annotations

import math

import numpy as np

import _reg_ref as R

L2, L1, HUBER, CAUCHY, GM, TUKEY = range(6)
KERNELS = dict(l1=L1, huber=HUBER, cauchy=CAUCHY, gm=GM, tukey=TUKEY)
ROB_D = 31  # the 29 of R.lsq_terms, then sum w and sum w r^2
INFO_D = 21


def weight(kernel: int, r, k: float) -> np.ndarray:
    """w(r) [upstream RobustKernel.cpp]; L1 at r == 0 is 0 here (upstream divides by zero)"""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    with np.errstate(all="ignore"):
        if kernel == L2:
            return np.ones_like(r)
        if kernel == L1:
            return np.where(a == 0.0, 0.0, 1.0 / np.where(a == 0.0, 1.0, a))
        if kernel == HUBER:
            return k / np.fmax(a, k)
        if kernel == CAUCHY:
            q = r / k
            return 1.0 / (1.0 + q * q)
        if kernel == GM:
            t = k + r * r
            return k / (t * t)
        if kernel == TUKEY:
            q = np.fmin(1.0, a / k)
            u = 1.0 - q * q
            return u * u
    raise ValueError(kernel)


def jacobi3(M):
    """jacobi_sym(3, ...) of csrc/me_horn.hpp on a batch: M (N,3,3) -> (d (N,3), V (N,3,3) eigenvectors in the columns).  The same
    sweeps, the same rotation order (0,1), (0,2), (1,2), the same three update loops; a matrix leaves the iteration at the sweep
    whose off-diagonal sum is < 1e-300 and a zero entry skips its rotation, per matrix."""
    M = np.asarray(M, np.float64).reshape(-1, 3, 3)
    n = len(M)
    A = M.copy()
    V = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    live = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(100):
            if len(live) == 0:
                break
            a = A[live]
            off = ((0.0 + a[:, 0, 1] * a[:, 0, 1]) + a[:, 0, 2] * a[:, 0, 2]) + a[:, 1, 2] * a[:, 1, 2]
            live = live[~(off < 1e-300)]
            if len(live) == 0:
                break
            a = [[A[live, i, j].copy() for j in range(3)] for i in range(3)]
            v = [[V[live, i, j].copy() for j in range(3)] for i in range(3)]
            for p in range(3):
                for q in range(p + 1, 3):
                    apq = a[p][q]
                    rot = ~(apq == 0.0)
                    theta = (a[q][q] - a[p][p]) / (2.0 * apq)
                    t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    sn = t * c
                    for k in range(3):
                        akp, akq = a[k][p], a[k][q]
                        a[k][p] = np.where(rot, c * akp - sn * akq, akp)
                        a[k][q] = np.where(rot, sn * akp + c * akq, akq)
                    for k in range(3):
                        apk, aqk = a[p][k], a[q][k]
                        a[p][k] = np.where(rot, c * apk - sn * aqk, apk)
                        a[q][k] = np.where(rot, sn * apk + c * aqk, aqk)
                    for k in range(3):
                        vkp, vkq = v[k][p], v[k][q]
                        v[k][p] = np.where(rot, c * vkp - sn * vkq, vkp)
                        v[k][q] = np.where(rot, sn * vkp + c * vkq, vkq)
            for i in range(3):
                for j in range(3):
                    A[live, i, j] = a[i][j]
                    V[live, i, j] = v[i][j]
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], -1), V


def w_matrix(M):
    """W = V diag(1 / sqrt(lam)) V^T as the kernel writes it: the upper triangle ((V_i0 s0) V_j0 + (V_i1 s1) V_j1) + (V_i2 s2) V_j2 with
    s = 1 / sqrt(lam), mirrored.  -> (W (N,3,3), lam (N,3), ok (N,) bool: every lam > 0 and finite)."""
    lam, V = jacobi3(M)
    with np.errstate(all="ignore"):
        ok = np.all(lam > 0.0, axis=1) & np.all(np.isfinite(lam), axis=1)
        s = 1.0 / np.sqrt(lam)
        W = np.empty((len(lam), 3, 3))
        for a in range(3):
            for b in range(a, 3):
                v = ((V[:, a, 0] * s[:, 0]) * V[:, b, 0] + (V[:, a, 1] * s[:, 1]) * V[:, b, 1]) + (V[:, a, 2] * s[:, 2]) * V[:, b, 2]
                W[:, a, b] = v
                W[:, b, a] = v
    return W, lam, ok


def gicp_rows(src, d, W):
    """the three rows per correspondence: J_i = W_i [-skew(vs) | I] (list of 3 lists of 6 arrays), r_i = W_i d (list of 3 arrays)"""
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    zero, one = np.zeros(len(src)), np.ones(len(src))
    Jm = [zero, z, -y, one, zero, zero, -z, zero, x, zero, one, zero, y, -x, zero, zero, zero, one]
    with np.errstate(all="ignore"):
        WJ = [[(W[:, a, 0] * Jm[c] + W[:, a, 1] * Jm[6 + c]) + W[:, a, 2] * Jm[12 + c] for c in range(6)] for a in range(3)]
        r = [(W[:, a, 0] * d[0] + W[:, a, 1] * d[1]) + W[:, a, 2] * d[2] for a in range(3)]
    return WJ, r


def robust_terms(mode: int, kernel: int, k: float, src, src_cov, tgt, tgt_attr, idx, d2, max_d: float):
    """The 31 quantities of k_lsq_sums_robust<mode, kernel> per gated correspondence, fp64, the kernel's operation order.
    -> (terms (M,31), keep (N,), n_zero_weight, n_degenerate).  A degenerate correspondence (mode 2) keeps its d2 column only."""
    src = np.ascontiguousarray(src, np.float64)
    tgt = np.ascontiguousarray(tgt, np.float64)
    d2 = np.asarray(d2, np.float64)
    keep = (d2 >= 0.0) & (d2 < max_d * max_d)
    si = np.nonzero(keep)[0]
    j = np.asarray(idx)[si]
    o = np.zeros((len(si), ROB_D))
    vs = [src[si, 0], src[si, 1], src[si, 2]]
    d = [vs[0] - tgt[j, 0], vs[1] - tgt[j, 1], vs[2] - tgt[j, 2]]
    o[:, 28] = d2[si]
    n_deg = 0
    with np.errstate(all="ignore"):
        if mode == 1:
            ta = np.asarray(tgt_attr, np.float64).reshape(len(tgt), 3)
            nt = [ta[j, 0], ta[j, 1], ta[j, 2]]
            J = R._cross3(vs, nt) + nt
            r = R._dot3(d, nt)
            w = weight(kernel, r, k)
            n_zero = int((w == 0.0).sum())
            t = 0
            for a in range(6):
                Jw = J[a] * w
                for b in range(a, 6):
                    o[:, t] = Jw * J[b]
                    t += 1
                o[:, 21 + a] = Jw * r
            o[:, 27] = r * r
            o[:, 29] = w
            o[:, 30] = w * (r * r)
        else:
            ta = np.asarray(tgt_attr, np.float64).reshape(len(tgt), 3, 3)
            sa = np.asarray(src_cov, np.float64).reshape(len(src), 3, 3)
            W, _, ok = w_matrix(ta[j] + sa[si])
            n_deg = int((~ok).sum())
            WJ, r = gicp_rows(src[si], d, W)
            w = [weight(kernel, r[a], k) for a in range(3)]
            n_zero = int(sum(((w[a] == 0.0) & ok).sum() for a in range(3)))
            t = 0
            for a in range(6):
                Jw = [WJ[i][a] * w[i] for i in range(3)]
                for b in range(a, 6):
                    o[:, t] = (Jw[0] * WJ[0][b] + Jw[1] * WJ[1][b]) + Jw[2] * WJ[2][b]
                    t += 1
                o[:, 21 + a] = (Jw[0] * r[0] + Jw[1] * r[1]) + Jw[2] * r[2]
            o[:, 27] = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
            o[:, 29] = (w[0] + w[1]) + w[2]
            o[:, 30] = (w[0] * (r[0] * r[0]) + w[1] * (r[1] * r[1])) + w[2] * (r[2] * r[2])
            bad = ~ok
            o[bad, :28] = 0.0
            o[bad, 29:] = 0.0
    return o, keep, n_zero, n_deg


def info_terms(tgt, idx, d2, max_d: float):
    """k_info_sums: the 21 upper-triangle entries of G^T G, G = [-skew(t) | I], per gated correspondence -> (terms (M,21), keep)"""
    tgt = np.ascontiguousarray(tgt, np.float64)
    d2 = np.asarray(d2, np.float64)
    keep = (d2 >= 0.0) & (d2 < max_d * max_d)
    t = tgt[np.asarray(idx)[keep]]
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    zero, one = np.zeros(len(t)), np.ones(len(t))
    G = [zero, z, -y, one, zero, zero, -z, zero, x, zero, one, zero, y, -x, zero, zero, zero, one]
    o = np.empty((len(t), INFO_D))
    c = 0
    for a in range(6):
        for b in range(a, 6):
            o[:, c] = (G[a] * G[b] + G[6 + a] * G[6 + b]) + G[12 + a] * G[12 + b]
            c += 1
    return o, keep


def tri_to_sym(s21) -> np.ndarray:
    A = np.zeros((6, 6))
    t = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = s21[t]
            t += 1
    return A


def device_sums(s) -> np.ndarray:
    """the 31 numbers of an IcpRobust in the order of robust_terms"""
    return np.r_[R.device_sums(s), s.sum_w, s.sum_wr2]


def sums_and_bound(terms, n_source: int):
    """-> (math.fsum of every column, R.lsq_bound of the launch for n_source queries: the bound reads no column count)"""
    exact, _ = R.lsq_sums_exact(terms) if len(terms) else (np.zeros(terms.shape[1]), None)
    return exact, R.lsq_bound(n_source, np.abs(terms).sum(0))


def check_sums(dev, terms, n_source: int, tag=""):
    exact, B = sums_and_bound(terms, n_source)
    with np.errstate(all="ignore"):
        ratio = np.where(B > 0, np.abs(dev - exact) / np.where(B > 0, B, 1.0), np.where(dev == exact, 0.0, np.inf))
    print(f"{tag}: max |device - fsum| / B = {ratio.max():.3f}")
    assert np.all(np.abs(dev - exact) <= B), (tag, ratio)
    return exact


def robust_loop(mode: int, kernel: int, k: float, src, tgt, max_d: float, *, src_cov=None, tgt_attr=None, max_iteration: int = 30,
                relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, exact: bool = False):
    """R.icp_lsq_loop with weights: the same evaluations, updates and stopping rule, the terms from robust_terms (kernel L2: R.lsq_terms).
    Column sums are numpy's pairwise ones unless exact (math.fsum): the comparisons made with it are at 1e-8."""
    from scipy.spatial import cKDTree

    src = np.ascontiguousarray(src, np.float64).copy()
    tgt = np.ascontiguousarray(tgt, np.float64)
    tree = cKDTree(tgt)
    cs = None if src_cov is None else np.asarray(src_cov, np.float64).reshape(-1, 3, 3).copy()
    hist = []

    def evaluate():
        idx, d2 = R.nn1(tree, tgt, src)
        if kernel == L2:
            terms, keep = R.lsq_terms(mode, src, cs, tgt, tgt_attr, idx, d2, max_d)
        else:
            terms, keep, _, _ = robust_terms(mode, kernel, k, src, cs, tgt, tgt_attr, idx, d2, max_d)
        s = R.lsq_sums_exact(terms)[0] if exact else terms.sum(0)
        n = int(keep.sum())
        fit = n / len(src) if len(src) else 0.0
        rmse = float(np.sqrt(s[28] / n)) if n else 0.0
        hist.append((n, fit, rmse))
        return s, n, fit, rmse

    total = np.eye(4)
    s, n, fit, rmse = evaluate()
    it = 0
    for it in range(1, max_iteration + 1):
        if n == 0:
            break
        JTJ, JTr, _, _ = R.sums_to_system(s)
        upd = R.lsq_update(JTJ, JTr)
        total = upd @ total
        src = R.transform_points(src, upd)
        if cs is not None:
            _, cs = R.rotate_attr(upd, cov=cs)
        pf, pr = fit, rmse
        s, n, fit, rmse = evaluate()
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return dict(transformation=total, fitness=fit, inlier_rmse=rmse, n_corr=n, iterations=it, cloud=src, history=hist)


# ---------------------------------------------------------------- scenes shared by the CPU and the GPU tests ----
def lsq_pair(kind: str, n: int, shift):
    """the two pairs the plain step is tested on (test_gpu_registration_edges._lsq_pair, restated)"""
    from cloud_map_evaluation_amd import synth

    if kind == "campus":
        est, gt = synth.campus_pair(n, seed=5)
        est, gt = est.numpy(), gt.numpy()
        est = est[:256 * ((len(est) - 1) // 256) + 1]
    else:
        est, gt = synth.scan_pair(n, seed=5)
        est, gt = est.numpy(), gt.numpy()
    sh = np.array(shift)
    return est + sh, gt + sh


OUTLIER_POSE = [0.004, -0.003, 0.006, 0.05, -0.04, 0.03]  # the small motion of the loop tests
OUTLIER_SHARE = 0.2
OUTLIER_GHOST = (0.12, -0.09, 0.15)  # a rigid ghost copy (a double wall): one direction, so its pull does not average out
OUTLIER_GATE = 0.5
OUTLIER_TUKEY_K = 0.05


def outlier_scene(n: int = 100_000, seed: int = 5):
    """-> (gt, map, pose): gt = R.scene("campus", n); map = gt moved by the known small pose, every fifth point (20 %) moved on by the ghost
    offset.  Registering map to gt should return pose^-1."""
    gt = R.scene("campus", n, seed)
    pose = R.vector6_to_matrix(OUTLIER_POSE)
    m = gt.copy()
    ghost = np.arange(len(m)) % 5 == 0
    assert abs(ghost.mean() - OUTLIER_SHARE) < 1e-3
    m[ghost] += np.array(OUTLIER_GHOST)
    return gt, R.transform_points(m, pose), pose


def pose_error(total, pose) -> float:
    """largest entry of total @ pose - I: 0 when the loop undid the known pose"""
    return float(np.abs(np.asarray(total) @ pose - np.eye(4)).max())
