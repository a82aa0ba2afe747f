"""Plain numpy model of the registration path (me_reg.hip: k_knn_normals + fast_eigen3x3, k_gicp_cov, k_rotate_attr, k_lsq_sums,
k_lsq_final; icp.py: lsq_update, _icp_lsq), independent of oracle/.

Two kinds of reference live here.  The *_exact functions state WHAT is computed in higher precision (the centred covariance in
np.longdouble, column sums with math.fsum): they carry no operation order and no sign.  The others restate HOW the kernels compute
it, operation by operation in fp64 (numpy does not contract a*b+c across ufuncs), so they carry the sign of a normal, the branch
of fast_eigen3x3 that was taken, and the per-correspondence terms whose only difference from the device is the order of the sum."""
from __future__ import annotations

import math
import os

import numpy as np

_WORKERS = min(16, os.cpu_count() or 1)  # (cKDTree threads)
U = 2.0 ** -53

# ---- branch ids of fast_eigen3x3, as normal_open3d reports them ----
BR_ZERO = 0       # max_coeff == 0: zero vector (the caller turns it into (0,0,1))
BR_DIAG_X = 1     # norm == 0, cov[0] strictly smallest
BR_DIAG_Y = 2     # norm == 0, cov[4] strictly smallest
BR_DIAG_Z = 3     # norm == 0, otherwise (ties included; also the identity of a neighbourhood of < 3 points)
BR_POS_EV2 = 4    # half_det >= 0, ev2 strictly smallest: return eigvec0(ev2)
BR_POS_EV1 = 5    # half_det >= 0, ev1 strictly smallest: return eigvec1
BR_POS_CROSS = 6  # half_det >= 0, otherwise: evec1 x evec2
BR_NEG_EV0 = 7    # half_det < 0, ev0 strictly smallest: return eigvec0(ev0)
BR_NEG_EV1 = 8    # half_det < 0, ev1 strictly smallest: return eigvec1
BR_NEG_CROSS = 9  # half_det < 0, otherwise: evec0 x evec1
# Of the ten, seven can be reached.  With angle = acos(half_det) / 3 in [0, pi/3] the closed form gives beta0 = 2 cos(angle + 2 pi / 3)
# <= beta1 = -(beta0 + beta2) <= beta2, and ev = q + p * beta is rounded monotonically, so ev0 <= ev1 <= ev2 always: a STRICT
# ev2 < ev0 (4) or ev1 < ev0 (5, 8) cannot hold (at angle == 0 the rounding of cos(2.0943951023931953) even leaves beta0 an ulp below
# beta1).  The eigvec1 early returns and the ev2-smallest return are dead.  The cross product on the half_det < 0 side (9) is NOT:
# when p is below an ulp of q (a near-isotropic neighbourhood) the three eigenvalues round to the same number, ev0 < ev1 is false and
# the code falls through to evec0 x evec1; degenerate_clouds()["isotropic_k7"] does that.  A NaN covariance fails every comparison
# and falls to a cross product as well.
BR_REACHABLE = (BR_ZERO, BR_DIAG_X, BR_DIAG_Y, BR_DIAG_Z, BR_POS_CROSS, BR_NEG_EV0, BR_NEG_CROSS)


def d2_exact(q: np.ndarray, p: np.ndarray) -> np.ndarray:
    """((dx*dx + dy*dy) + dz*dz), fp64 (dist2_exact of the library)."""
    d = q - p
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _mm(a, b):
    """(N,3,3) x (N,3,3) or broadcastable, each entry (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j"""
    return np.stack([np.stack([(a[..., i, 0] * b[..., 0, j] + a[..., i, 1] * b[..., 1, j]) + a[..., i, 2] * b[..., 2, j]
                               for j in range(3)], -1) for i in range(3)], -2)


def _mm_bt(a, b):
    """a * b^T with the same association"""
    return np.stack([np.stack([(a[..., i, 0] * b[..., j, 0] + a[..., i, 1] * b[..., j, 1]) + a[..., i, 2] * b[..., j, 2]
                               for j in range(3)], -1) for i in range(3)], -2)


# ---------------------------------------------------------------- normals: the definition, in extended precision ----
def normal_exact(xyz, idx, chunk: int = 1 << 17):
    """Per row of neighbour indices (-1 = no neighbour): the CENTRED covariance in np.longdouble (mean first, then the second moments of
    the differences, / count), rounded to fp64 (centred, it is well scaled) and decomposed with numpy.linalg.eigh.
    -> dict(vec (N,3) unit eigenvector of the smallest eigenvalue, sign-free; w (N,3) ascending eigenvalues; gap01 = w1 - w0;
            gap12 = w2 - w1; S (N,) the largest raw second moment max_i E[x_i^2] of the neighbourhood in the given coordinates;
            count (N,)).  Rows with fewer than 3 neighbours get the identity covariance, as the kernel does."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    idx = np.asarray(idx)
    n, k = idx.shape
    vec = np.empty((n, 3))
    w = np.empty((n, 3))
    S = np.empty(n)
    count = np.empty(n, np.int64)
    for b in range(0, n, chunk):
        ix = idx[b:b + chunk]
        have = ix >= 0
        cnt = have.sum(1)
        P = xyz[np.where(have, ix, 0)].astype(np.longdouble)  # (m,k,3)
        hv = have[:, :, None]
        cl = np.maximum(cnt, 1).astype(np.longdouble)[:, None]
        mean = np.where(hv, P, 0).sum(1) / cl
        D = np.where(hv, P - mean[:, None, :], 0)
        Cm = np.empty((len(ix), 3, 3), np.longdouble)
        for i in range(3):
            for j in range(i, 3):
                Cm[:, i, j] = Cm[:, j, i] = (D[:, :, i] * D[:, :, j]).sum(1) / cl[:, 0]
        Cd = Cm.astype(np.float64)
        Cd[cnt < 3] = np.eye(3)
        ww, vv = np.linalg.eigh(Cd)
        vec[b:b + chunk] = vv[:, :, 0]
        w[b:b + chunk] = ww
        S[b:b + chunk] = (np.where(hv, P * P, 0).sum(1) / cl).max(1).astype(np.float64)
        count[b:b + chunk] = cnt
    return dict(vec=vec, w=w, gap01=w[:, 1] - w[:, 0], gap12=w[:, 2] - w[:, 1], S=S, count=count)


def angle_sign_free(a, b) -> np.ndarray:
    """angle in [0, pi/2] between the LINES spanned by the rows of a and b (atan2 of |a x b| and |a . b|: accurate near 0)"""
    c = np.cross(a, b)
    return np.arctan2(np.sqrt((c * c).sum(1)), np.abs((a * b).sum(1)))


# ---------------------------------------------------------------- normals: the kernel's own operation order ----
def raw_covariance(xyz, idx):
    """utility::ComputeCovariance as k_knn_normals does it: raw moments summed neighbour by neighbour (ascending distance), / count,
    c[3] - c[0] * c[0] ...; identity for < 3 neighbours.  -> (cov as a list of 9 (N,) arrays, count)."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    idx = np.asarray(idx)
    n, k = idx.shape
    c = [np.zeros(n) for _ in range(9)]
    cnt = (idx >= 0).sum(1)
    for j in range(k):
        have = idx[:, j] >= 0  # (the valid entries are a prefix of the row)
        p = xyz[np.where(have, idx[:, j], 0)]
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        for e, v in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            c[e] = np.where(have, c[e] + v, c[e])
    m = np.maximum(cnt, 1).astype(np.float64)
    c = [v / m for v in c]
    cov = [None] * 9
    cov[0] = c[3] - c[0] * c[0]
    cov[4] = c[6] - c[1] * c[1]
    cov[8] = c[8] - c[2] * c[2]
    cov[1] = cov[3] = c[4] - c[0] * c[1]
    cov[2] = cov[6] = c[5] - c[0] * c[2]
    cov[5] = cov[7] = c[7] - c[1] * c[2]
    few = cnt < 3
    for e in range(9):
        cov[e] = np.where(few, 1.0 if e % 4 == 0 else 0.0, cov[e])
    return cov, cnt


def _eigvec0(A, ev):
    row0 = [A[0] - ev, A[1], A[2]]
    row1 = [A[1], A[4] - ev, A[5]]
    row2 = [A[2], A[5], A[8] - ev]
    r01, r02, r12 = _cross3(row0, row1), _cross3(row0, row2), _cross3(row1, row2)
    d0, d1, d2 = _dot3(r01, r01), _dot3(r02, r02), _dot3(r12, r12)
    dmax = d0
    imax = np.zeros(d0.shape, np.int8)
    t = d1 > dmax
    dmax = np.where(t, d1, dmax)
    imax = np.where(t, 1, imax)
    imax = np.where(d2 > dmax, 2, imax)
    ln = np.sqrt(np.where(imax == 0, d0, np.where(imax == 1, d1, d2)))
    return [np.where(imax == 0, r01[k], np.where(imax == 1, r02[k], r12[k])) / ln for k in range(3)]


def _eigvec1(A, e0, ev1):
    """-> (vector, plain): plain = the (cu, cv) == (1, 0) case, which returns U itself"""
    bx = np.abs(e0[0]) > np.abs(e0[1])
    ia = 1.0 / np.sqrt(e0[0] * e0[0] + e0[2] * e0[2])
    ib = 1.0 / np.sqrt(e0[1] * e0[1] + e0[2] * e0[2])
    zero = np.zeros_like(ia)
    Uv = [np.where(bx, -e0[2] * ia, zero), np.where(bx, zero, e0[2] * ib), np.where(bx, e0[0] * ia, -e0[1] * ib)]
    Vv = _cross3(e0, Uv)

    def mul(v):
        return [(A[0] * v[0] + A[1] * v[1]) + A[2] * v[2], (A[1] * v[0] + A[4] * v[1]) + A[5] * v[2],
                (A[2] * v[0] + A[5] * v[1]) + A[8] * v[2]]

    AU, AV = mul(Uv), mul(Vv)
    m00, m01, m11 = _dot3(Uv, AU) - ev1, _dot3(Uv, AV), _dot3(Vv, AV) - ev1
    a00, a01, a11 = np.abs(m00), np.abs(m01), np.abs(m11)

    def solve(md, ad):  # the (m00 | m11) arm: -> (first, second) coefficients and whether the arm is live
        live = np.fmax(ad, a01) > 0
        big = ad >= a01
        q1 = m01 / md
        d1 = 1 / np.sqrt(1 + q1 * q1)
        o1 = q1 * d1                      # big:  (md, m01) <- (d1, o1)
        q2 = md / m01
        o2 = 1 / np.sqrt(1 + q2 * q2)
        d2 = q2 * o2                      # else: (md, m01) <- (d2, o2)
        return np.where(big, d1, d2), np.where(big, o1, o2), live

    d_a, o_a, live_a = solve(m00, a00)  # a00 >= a11: cu = m01, cv = m00
    d_b, o_b, live_b = solve(m11, a11)  # else:       cu = m11, cv = m01
    first = a00 >= a11
    cu = np.where(first, np.where(live_a, o_a, 1.0), np.where(live_b, d_b, 1.0))
    cv = np.where(first, np.where(live_a, d_a, 0.0), np.where(live_b, o_b, 0.0))
    plain = (cu == 1) & (cv == 0)
    return [np.where(plain, Uv[k], cu * Uv[k] - cv * Vv[k]) for k in range(3)], plain


def _libm(f, x):
    """math.acos / math.cos element by element: the C library's own functions, the ones a CPU build of the same arithmetic calls
    (numpy's vectorised arccos / cos may differ from them by an ulp)"""
    return np.frompyfunc(f, 1, 1)(x).astype(np.float64)


def fast_eigen3x3(cov):
    """cov: list of 9 (N,) arrays -> (vector as (N,3), branch id (N,), plain (N,) bool: eigvec1 ran and took its `plain` case)"""
    with np.errstate(all="ignore"):
        n = cov[0].shape[0]
        mc = cov[0]
        for e in range(1, 9):
            mc = np.fmax(mc, cov[e])
        A = [cov[e] / mc for e in range(9)]
        norm = (A[1] * A[1] + A[2] * A[2]) + A[5] * A[5]
        q = ((A[0] + A[4]) + A[8]) / 3
        b00, b11, b22 = A[0] - q, A[4] - q, A[8] - q
        p = np.sqrt((((b00 * b00 + b11 * b11) + b22 * b22) + norm * 2) / 6)
        c00 = b11 * b22 - A[5] * A[5]
        c01 = A[1] * b22 - A[5] * A[2]
        c02 = A[1] * A[5] - b11 * A[2]
        det = ((b00 * c00 - A[1] * c01) + A[2] * c02) / ((p * p) * p)
        half_det = np.fmin(np.fmax(det * 0.5, -1.0), 1.0)
        angle = _libm(math.acos, half_det) / 3.0
        beta2 = _libm(math.cos, angle) * 2
        beta0 = _libm(math.cos, angle + 2.09439510239319549) * 2
        beta1 = -(beta0 + beta2)
        ev0, ev1, ev2 = q + p * beta0, q + p * beta1, q + p * beta2
        pos = half_det >= 0
        ea = _eigvec0(A, np.where(pos, ev2, ev0))
        eb, plain = _eigvec1(A, ea, ev1)
        ret_a = np.where(pos, (ev2 < ev0) & (ev2 < ev1), (ev0 < ev1) & (ev0 < ev2))
        ret_b = ~ret_a & (ev1 < ev0) & (ev1 < ev2)
        cr_pos, cr_neg = _cross3(eb, ea), _cross3(ea, eb)
        out = np.empty((n, 3))
        for k in range(3):
            out[:, k] = np.where(ret_a, ea[k], np.where(ret_b, eb[k], np.where(pos, cr_pos[k], cr_neg[k])))
        br = np.where(pos, np.where(ret_a, BR_POS_EV2, np.where(ret_b, BR_POS_EV1, BR_POS_CROSS)),
                      np.where(ret_a, BR_NEG_EV0, np.where(ret_b, BR_NEG_EV1, BR_NEG_CROSS))).astype(np.int8)
        diag = ~(norm > 0)
        dx = (cov[0] < cov[4]) & (cov[0] < cov[8])
        dy = ~dx & (cov[4] < cov[0]) & (cov[4] < cov[8])
        dz = ~dx & ~dy
        for k, sel in enumerate((dx, dy, dz)):
            out[:, k] = np.where(diag, sel.astype(np.float64), out[:, k])
        br = np.where(diag, np.where(dx, BR_DIAG_X, np.where(dy, BR_DIAG_Y, BR_DIAG_Z)), br).astype(np.int8)
        zero = mc == 0
        out[zero] = 0.0
        br[zero] = BR_ZERO
        plain = plain & ~diag & ~zero & ~ret_a
    return out, br, plain


def normal_open3d(xyz, idx):
    """The literal operation order of k_knn_normals + fast_eigen3x3 in fp64 -> (normals (N,3), branch (N,), plain (N,))."""
    cov, _ = raw_covariance(xyz, idx)
    nv, br, plain = fast_eigen3x3(cov)
    with np.errstate(invalid="ignore"):
        z = np.sqrt(_dot3(nv.T, nv.T)) == 0.0  # (false for NaN: a NaN normal is stored as it is)
    nv[z] = (0.0, 0.0, 1.0)
    return nv, br, plain


# ---------------------------------------------------------------- attributes ----
def gicp_cov(normals, eps: float) -> np.ndarray:
    """k_gicp_cov: C = Rx diag(eps,1,1) Rx^T, Rx = I + [v]x + [v]x^2 / (1 + x0), v = e1 x n; identity where x0 < -0.99 (sic)."""
    nrm = np.ascontiguousarray(normals, np.float64)
    n = len(nrm)
    x0, x1, x2 = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    zero = np.zeros(n)
    v = [zero, -x2, x1]
    sv = np.stack([np.stack([zero, -v[2], v[1]], -1), np.stack([v[2], zero, -v[0]], -1), np.stack([-v[1], v[0], zero], -1)], -2)
    with np.errstate(all="ignore"):
        sv2 = _mm(sv, sv)
        factor = 1 / (1 + x0)
        R = (np.eye(3)[None] + sv) + sv2 * factor[:, None, None]
    ident = x0 < -0.99
    R[ident] = np.eye(3)
    Cd = np.broadcast_to(np.diag([eps, 1.0, 1.0]), (n, 3, 3))
    with np.errstate(all="ignore"):
        return _mm_bt(_mm(R, Cd), R)


def gicp_cov_definition(normals, eps: float) -> np.ndarray:
    """what the covariance IS for a unit normal off the identity branch: I - (1 - eps) n n^T"""
    nrm = np.asarray(normals, np.float64)
    return np.eye(3)[None] - (1 - eps) * nrm[:, :, None] * nrm[:, None, :]


def rotate_attr(T, normals=None, cov=None):
    """k_rotate_attr: n <- R n, C <- (R C) R^T with the kernel's association; returns rotated copies"""
    R = np.asarray(T, np.float64).reshape(4, 4)[:3, :3]
    n2 = c2 = None
    if normals is not None:
        v = np.asarray(normals, np.float64)
        n2 = np.stack([(R[r, 0] * v[:, 0] + R[r, 1] * v[:, 1]) + R[r, 2] * v[:, 2] for r in range(3)], -1)
    if cov is not None:
        Cm = np.asarray(cov, np.float64).reshape(-1, 3, 3)
        Rb = np.broadcast_to(R, Cm.shape)
        c2 = _mm_bt(_mm(Rb, Cm), Rb)
    return n2, c2


def transform_points(xyz, T):
    """PointCloud::Transform on the points: h_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3, p = h[:3] / h[3]"""
    xyz = np.asarray(xyz, np.float64)
    T = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    h = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(4)]
    return np.stack([h[0] / h[3], h[1] / h[3], h[2] / h[3]], -1)


# ---------------------------------------------------------------- the least-squares step ----
LSQ_D = 29  # JTJ upper triangle (21, row-major a <= b) + JTr (6) + r2 + sum_d2


def _inv3(m):
    """Eigen Matrix3d::inverse() as inv3 of the kernel: cofactors, determinant along column 0; m, result: lists of 9 arrays"""
    c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    c10, c11, c12 = m[7] * m[2] - m[8] * m[1], m[8] * m[0] - m[6] * m[2], m[6] * m[1] - m[7] * m[0]
    c20, c21, c22 = m[1] * m[5] - m[2] * m[4], m[2] * m[3] - m[0] * m[5], m[0] * m[4] - m[1] * m[3]
    det = (c00 * m[0] + c10 * m[3]) + c20 * m[6]
    inv = 1.0 / det
    return [c00 * inv, c10 * inv, c20 * inv, c01 * inv, c11 * inv, c21 * inv, c02 * inv, c12 * inv, c22 * inv]


def lsq_terms(mode: int, src, src_cov, tgt, tgt_attr, idx, d2, max_d: float, chunk: int = 1 << 19):
    """The 29 quantities of k_lsq_sums<mode> per correspondence, fp64, the kernel's operation order.  src (N,3) in the caller's
    order with idx / d2 (N,) from nn1 in the same order; tgt_attr = target normals (mode 1) or covariances (mode 2); src_cov the
    source covariances (mode 2; ignored in mode 1).  -> (terms (M, 29), keep (N,) bool), M = keep.sum(), rows in source order."""
    src = np.ascontiguousarray(src, np.float64)
    tgt = np.ascontiguousarray(tgt, np.float64)
    d2 = np.asarray(d2, np.float64)
    keep = (d2 >= 0.0) & (d2 < max_d * max_d)
    sel = np.nonzero(keep)[0]
    out = np.empty((len(sel), LSQ_D))
    ta = np.asarray(tgt_attr, np.float64).reshape(len(tgt), -1)
    sa = None if mode == 1 else np.asarray(src_cov, np.float64).reshape(len(src), 9)
    for b in range(0, len(sel), chunk):
        si = sel[b:b + chunk]
        j = np.asarray(idx)[si]
        o = out[b:b + chunk]
        vs = [src[si, 0], src[si, 1], src[si, 2]]
        d = [vs[0] - tgt[j, 0], vs[1] - tgt[j, 1], vs[2] - tgt[j, 2]]
        if mode == 1:
            nt = [ta[j, 0], ta[j, 1], ta[j, 2]]
            J = _cross3(vs, nt) + nt
            r = _dot3(d, nt)
            t = 0
            for a in range(6):
                for c in range(a, 6):
                    o[:, t] = J[a] * J[c]
                    t += 1
            for a in range(6):
                o[:, 21 + a] = J[a] * r
            o[:, 27] = r * r
        else:
            M = [ta[j, e] + sa[si, e] for e in range(9)]
            with np.errstate(all="ignore"):
                B = _inv3(M)
            x, y, z = vs
            zero, one = np.zeros(len(si)), np.ones(len(si))
            Jm = [zero, z, -y, one, zero, zero, -z, zero, x, zero, one, zero, y, -x, zero, zero, zero, one]  # [-skew(vs) | I]
            with np.errstate(all="ignore"):
                BJ = [(B[3 * r] * Jm[c] + B[3 * r + 1] * Jm[6 + c]) + B[3 * r + 2] * Jm[12 + c] for r in range(3) for c in range(6)]
                Bd = [(B[3 * r] * d[0] + B[3 * r + 1] * d[1]) + B[3 * r + 2] * d[2] for r in range(3)]
                t = 0
                for a in range(6):
                    for c in range(a, 6):
                        o[:, t] = (Jm[a] * BJ[c] + Jm[6 + a] * BJ[6 + c]) + Jm[12 + a] * BJ[12 + c]
                        t += 1
                for a in range(6):
                    o[:, 21 + a] = (Jm[a] * Bd[0] + Jm[6 + a] * Bd[1]) + Jm[12 + a] * Bd[2]
                o[:, 27] = _dot3(d, Bd)
        o[:, 28] = d2[si]
    return out, keep


def lsq_sums_exact(terms):
    """-> (sums (29,), abs_sums (29,)): every column summed with math.fsum, which returns the correctly rounded sum of the fp64
    terms at any length (Shewchuk's exact partials), so the reference carries no summation error of its own at 100 000 or at
    5 000 000 rows (29 columns of 5 M Python floats cost a few seconds; np.longdouble pairwise would be faster but inexact)."""
    terms = np.asarray(terms, np.float64)
    s = np.array([math.fsum(terms[:, k].tolist()) for k in range(terms.shape[1])])
    a = np.array([math.fsum(np.abs(terms[:, k]).tolist()) for k in range(terms.shape[1])])
    return s, a


def sums_to_system(s):
    """29 sums -> (JTJ (6,6) symmetric, JTr (6,), r2, sum_d2)"""
    JTJ = np.zeros((6, 6))
    t = 0
    for a in range(6):
        for b in range(a, 6):
            JTJ[a, b] = JTJ[b, a] = s[t]
            t += 1
    return JTJ, np.array(s[21:27]), float(s[27]), float(s[28])


def device_sums(s) -> np.ndarray:
    """the 29 numbers of an IcpLsq / oracle dict in the order of lsq_terms"""
    if isinstance(s, dict):
        JTJ, JTr, r2, sd = np.asarray(s["JTJ"]).reshape(6, 6), np.asarray(s["JTr"]), s["r2"], s["sum_d2"]
    else:
        JTJ, JTr, r2, sd = np.array(list(s.JTJ)).reshape(6, 6), np.array(list(s.JTr)), s.r2, s.sum_d2
    return np.r_[[JTJ[a, b] for a in range(6) for b in range(a, 6)], JTr, r2, sd]


def lsq_launch(n: int):
    """(nblocks, m): the launch of me_icp_lsq_sums for n queries — min(1024, ceil(n / 256)) blocks of 256 threads, at least 1 — and
    the largest number of rows one thread visits in the grid-stride loop, ceil(n / (256 nblocks))."""
    nb = max(1, min(1024, (n + 255) // 256))
    return nb, max(1, -(-n // (256 * nb)))


def lsq_bound(n: int, abs_sums) -> np.ndarray:
    """B_k = (m + 8 + ceil(nblocks / 256) + 8) u sum|term_k|: m sequential additions per thread, the 8 levels of the 256-wide tree
    (6 of the wave reduction, then (s0 + s1) + (s2 + s3)), k_lsq_final's ceil(nblocks / 256) sequential additions per thread and
    its own 8 levels.  First order in u; every partial sum is bounded by sum|term_k|."""
    nb, m = lsq_launch(n)
    return (m + 8 + -(-nb // 256) + 8) * U * np.asarray(abs_sums)


# ---------------------------------------------------------------- the loop of methods 1 / 2 ----
def vector6_to_matrix(x) -> np.ndarray:
    a, b, g = float(x[0]), float(x[1]), float(x[2])
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = np.asarray(x[3:6], float)
    return T


def lsq_update(JTJ, JTr) -> np.ndarray:
    """icp.lsq_update's rule, restated: x = solve(JTJ, -JTr); the identity when LAPACK reports an exactly singular factor or the
    solution is not finite"""
    try:
        x = np.linalg.solve(np.asarray(JTJ, float).reshape(6, 6), -np.asarray(JTr, float).reshape(6))
    except np.linalg.LinAlgError:
        return np.eye(4)
    return vector6_to_matrix(x) if np.all(np.isfinite(x)) else np.eye(4)


def nn1(tgt_tree, tgt, q, k: int = 4):
    """1-NN of q in tgt as the library defines it: smallest ((dx*dx + dy*dy) + dz*dz), ties to the smaller index.  Candidates: the k
    nearest of scipy's cKDTree, d2 recomputed and re-ranked; a row whose candidates all tie is settled against the whole target."""
    kk = min(k, len(tgt))
    _, ci = tgt_tree.query(q, k=kk, workers=_WORKERS)
    ci = np.asarray(ci).reshape(len(q), kk)
    cd = d2_exact(q[:, None, :], tgt[ci])
    order = np.lexsort((ci, cd), axis=1)
    ci, cd = np.take_along_axis(ci, order, 1), np.take_along_axis(cd, order, 1)
    idx, d2 = ci[:, 0].copy(), cd[:, 0].copy()
    if kk < len(tgt):
        for i in np.nonzero(cd[:, kk - 1] <= cd[:, 0])[0]:
            full = d2_exact(q[i], tgt)
            idx[i] = int(np.argmin(full))  # (argmin: the first, i.e. smallest, index of the minimum)
            d2[i] = full[idx[i]]
    return idx.astype(np.int32), d2


def icp_lsq_loop(mode: int, src, tgt, max_d: float, transform=transform_points, *, src_cov=None, tgt_attr=None, max_iteration: int = 30,
                 relative_fitness: float = 1e-6, relative_rmse: float = 1e-6):
    """icp._icp_lsq on numpy arrays: per iteration nn1 (cKDTree candidates, d2 recomputed), lsq_terms + exact sums, lsq_update with
    its singular rule, the update applied to the points by `transform(xyz, T)` (the caller passes the point transform it compares
    with) and to the source covariances by rotate_attr.  tgt_attr: target normals (mode 1) / covariances (mode 2).
    -> dict(transformation, fitness, inlier_rmse, n_corr, iterations, cloud, history [(n_corr, fitness, rmse) per evaluation])."""
    from scipy.spatial import cKDTree

    src = np.ascontiguousarray(src, np.float64).copy()
    tgt = np.ascontiguousarray(tgt, np.float64)
    tree = cKDTree(tgt)
    cs = None if src_cov is None else np.asarray(src_cov, np.float64).reshape(-1, 3, 3).copy()
    hist = []

    def evaluate():
        idx, d2 = nn1(tree, tgt, src)
        terms, keep = lsq_terms(mode, src, cs, tgt, tgt_attr, idx, d2, max_d)
        s, _ = lsq_sums_exact(terms)
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
        JTJ, JTr, _, _ = sums_to_system(s)
        upd = lsq_update(JTJ, JTr)
        total = upd @ total
        src = transform(src, upd)
        if cs is not None:
            _, cs = rotate_attr(upd, cov=cs)
        pf, pr = fit, rmse
        s, n, fit, rmse = evaluate()
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return dict(transformation=total, fitness=fit, inlier_rmse=rmse, n_corr=n, iterations=it, cloud=src, history=hist)


# ---------------------------------------------------------------- scenes and constants shared by the CPU and the GPU tests ----
SHIFT_NONE = (0.0, 0.0, 0.0)
SHIFT_NEAR = (812.0, -455.0, 31.0)
SHIFT_FAR = (8192.0, -6144.0, 31.0)  # a local-frame map far from its datum: x^2 ~ 7e7 m^2, one ulp of it ~ 1.5e-8 m^2
SHIFTS = dict(none=SHIFT_NONE, near=SHIFT_NEAR, far=SHIFT_FAR)
KS = (3, 4, 5, 20, 40)
G_REL = 1e-3  # relative gap (w1 - w0) / w2 above which a normal is compared with the oracle at 1e-9
# The constant of the perturbation bound C u S / (w1 - w0): the largest normal_ratio of oracle.estimate_normals_knn (the reference) over
# NORMAL_CASES (below), measured on the CPU (DESIGN.md section 4.5.1 has the figures); the device is given twice that.
# C is a property of these scenes, not of the method: at k = 3 the ratio has a heavy tail (491 on a 20 000-point campus scene), so a new
# scene needs its own measurement of the reference before it joins NORMAL_CASES.
C_REF = 92.1
C_DEV = 2 * C_REF


def scene(name: str, n: int, seed: int = 5) -> np.ndarray:
    """scan: the estimated map of synth.scan_pair (an independent noisy scan with sparse outliers); campus: the ground truth of
    synth.campus_pair (2 mm jitter); cube: the ground truth of synth.cube_pair (1 mm jitter)"""
    from cloud_map_evaluation_amd import synth

    if name == "scan":
        return synth.scan_pair(n, seed=seed)[0].numpy()
    if name == "campus":
        return synth.campus_pair(n, seed=seed)[1].numpy()
    if name == "cube":
        return synth.cube_pair(n, seed=seed)[1].numpy()
    raise ValueError(name)


# (scene, points, k, shift): every scene x k x shift at 100 000; a covering set at 1 000 000 (every k, every shift twice, every
# scene twice); one 5 000 000 case
NORMAL_CASES = [(s, 100_000, k, sh) for s in ("scan", "campus", "cube") for k in KS for sh in ("none", "near", "far")] + [
    ("scan", 1_000_000, 5, "near"), ("campus", 1_000_000, 20, "far"), ("cube", 1_000_000, 40, "none"),
    ("scan", 1_000_000, 3, "far"), ("campus", 1_000_000, 4, "near"), ("cube", 1_000_000, 20, "none"),
    ("campus", 5_000_000, 20, "near")]


def normal_ratio(nrm, ex) -> np.ndarray:
    """angle(nrm, exact eigenvector) * (w1 - w0) / (u S): the measured constant of the perturbation bound, per point (NaN where the
    gap is exactly 0)"""
    with np.errstate(all="ignore"):
        return angle_sign_free(nrm, ex["vec"]) * ex["gap01"] / (U * ex["S"])


# ---------------------------------------------------------------- degenerate clouds (every one is an input the API accepts) ----
def _rot(axis: int, deg: float) -> np.ndarray:
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def plane_lattice(normal_axis: int, nu: int = 9, nv: int = 8, step: float = 0.25, level: float = 1.5) -> np.ndarray:
    """nu x nv square lattice of dyadic coordinates in the plane (coordinate normal_axis) = level: every raw moment of a symmetric
    neighbourhood is exact, so the off-diagonal covariances are exactly 0 (the norm == 0 branch)"""
    g = np.stack(np.meshgrid(np.arange(nu) * step, np.arange(nv) * step, indexing="ij"), -1).reshape(-1, 2)
    out = np.full((len(g), 3), level)
    out[:, [a for a in range(3) if a != normal_axis]] = g
    return out


def lattice_interior(nu: int = 9, nv: int = 8) -> np.ndarray:
    """rows of plane_lattice whose 4- and 8-neighbourhoods are complete (k = 5 and k = 9 are symmetric there)"""
    iu, iv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    return ((iu > 0) & (iu < nu - 1) & (iv > 0) & (iv < nv - 1)).reshape(-1)


def degenerate_clouds() -> dict:
    """name -> (xyz, k)"""
    rng = np.random.default_rng(12)
    out = {}
    for a, nm in enumerate("xyz"):
        out[f"plane_{nm}_k5"] = (plane_lattice(a), 5)
        out[f"plane_{nm}_k9"] = (plane_lattice(a), 9)
    g3 = np.stack(np.meshgrid(*[np.arange(5) * 0.25] * 3, indexing="ij"), -1).reshape(-1, 3)
    out["cubic_lattice_k7"] = (g3, 7)  # interior: diag(v, v, v), a three-way tie
    tilt = _rot(1, 30.0) @ _rot(0, 30.0)
    out["plane_tilted_k9"] = (plane_lattice(2) @ tilt.T, 9)
    out["plane_tilted_k20"] = (plane_lattice(2) @ tilt.T, 20)
    t = np.arange(12) * 0.25
    for a, nm in enumerate("xyz"):
        line = np.zeros((12, 3))
        line[:, a] = t
        out[f"line_{nm}_k5"] = (line, 5)
    out["line_diag_k5"] = (np.stack([t, t, t], -1), 5)
    out["line_diag_k12"] = (np.stack([t, t, t], -1), 12)
    others = rng.uniform(2, 4, (40, 3))
    pile = np.vstack([np.tile([0.5, 0.75, 0.25], (5, 1)), others])
    out["pile_k3"] = (pile, 3)
    out["pile_k5"] = (pile, 5)
    tri = np.array([[0.0, 0, 0], [1.0, 0.25, 0], [0.5, 1.0, 0.75]])
    out["three_k3"] = (tri, 3)
    out["three_k40"] = (tri, 40)
    out["two_k20"] = (tri[:2], 20)
    d = 1e-18  # a near-isotropic octahedron: the off-diagonal covariances are ~1e-19, p is far below an ulp of q, ev0 == ev1 == ev2
    out["isotropic_k7"] = (np.array([[0, 0, 0], [1, d, 0], [-1, 0, 0], [0, 1, -d], [0, -1, 0], [d, 0, 1], [0, 0, -1.0]]), 7)
    far = plane_lattice(2, 12, 12, 0.01, 0.3) @ _rot(0, 20.0).T + np.array([1e5, -1e5, 1e5])
    out["far_lattice_k9"] = (far, 9)  # one ulp of x^2 (2e-6) is far above the variance (1e-4 m^2 .. 0): the covariance is rounding
    out["far_lattice_k20"] = (far, 20)
    return out


# ---------------------------------------------------------------- the literal Open3D per-row form (independent of lsq_terms) ----
def lsq_open3d_rows(mode: int, src, src_cov, tgt, tgt_attr, idx, keep):
    """J^T J, J^T r, sum r^2 from the per-row Jacobians as Open3D writes them: point-to-plane J = [vs x nt, nt], r = (vs - vt) . nt;
    generalized W = (Ct + Cs)^(-1/2) (scipy's matrix square root), three rows W [-skew(vs) | I] per correspondence, r = W (vs - vt)."""
    import scipy.linalg

    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    m = np.asarray(keep, bool)
    if mode == 1:
        nt = np.asarray(tgt_attr, np.float64)[idx[m]]
        J = np.hstack([np.cross(src[m], nt), nt])
        r = np.einsum("ij,ij->i", src[m] - tgt[idx[m]], nt)
        return J.T @ J, J.T @ r, float(r @ r)
    JTJ, JTr, r2 = np.zeros((6, 6)), np.zeros(6), 0.0
    for i in np.nonzero(m)[0]:
        W = np.real(scipy.linalg.sqrtm(np.linalg.inv(tgt_attr[idx[i]] + src_cov[i])))
        x, y, z = src[i]
        Jm = W @ np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1.0]])
        rr = W @ (src[i] - tgt[idx[i]])
        JTJ += Jm.T @ Jm
        JTr += Jm.T @ rr
        r2 += rr @ rr
    return JTJ, JTr, float(r2)
