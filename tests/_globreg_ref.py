"""numpy model of the coarse global registration (csrc/me_globreg.hip, csrc/me_horn.hpp): FPFH features, feature-space matching and
the RANSAC hypotheses, with every operation in the library's order (include/mapeval_hip.h), so that the device results can be compared
bit for bit.  Philox and the 64-bit high product come from _perturb_ref.py.

The only libm call on the device side is atan2 (f0 of the pair feature); it may differ from numpy's by an ulp, which only matters for a
pair feature that lies on a bin edge.  fpfh() therefore also reports, per point, whether any pair feature that its FPFH depends on lies
within EDGE_TOL of a bin edge.
"""
from __future__ import annotations

import math

import numpy as np

from _perturb_ref import mulhilo64, philox4x64_10

EDGE_TOL = 1e-12
TWO_PI = 2.0 * math.pi


# ---- neighbours -----------------------------------------------------------------------------------------------------------------------
def knn_lists(xyz: np.ndarray, k: int, chunk: int = 512):
    """The k nearest points of every point in the same cloud (itself included), ascending by (d2, index): (idx [n, k], d2 [n, k])."""
    n = len(xyz)
    k = min(k, n)
    idx = np.empty((n, k), np.int64)
    d2 = np.empty((n, k), np.float64)
    for a in range(0, n, chunk):
        q = xyz[a:a + chunk]
        dx = q[:, None, 0] - xyz[None, :, 0]
        dy = q[:, None, 1] - xyz[None, :, 1]
        dz = q[:, None, 2] - xyz[None, :, 2]
        D = (dx * dx + dy * dy) + dz * dz
        order = np.lexsort((np.broadcast_to(np.arange(n), D.shape), D), axis=1)[:, :k]
        idx[a:a + chunk] = order
        d2[a:a + chunk] = np.take_along_axis(D, order, axis=1)
    return idx, d2


def hybrid(idx: np.ndarray, d2: np.ndarray, radius: float):
    """KDTreeSearchParamHybrid on the k-NN lists: d2 < radius^2 and not the query itself -> boolean mask [n, k]."""
    return (d2 < radius * radius) & (idx != np.arange(len(idx))[:, None])


# ---- pair features --------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_features(p1, n1, p2, n2):
    """ComputePairFeatures for arrays of pairs [..., 3] -> [..., 3] (f0, f1, f2)."""
    p1, n1, p2, n2 = (np.asarray(a, np.float64) for a in (p1, n1, p2, n2))
    d = p2 - p1
    L = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        a1 = _dot(n1, d) / L
        a2 = _dot(n2, d) / L
        swap = np.abs(a1) < np.abs(a2)
        m1 = np.where(swap[..., None], n2, n1)
        m2 = np.where(swap[..., None], n1, n2)
        d = np.where(swap[..., None], -d, d)
        f2 = np.where(swap, -a2, a1)
        v = _cross(d, m1)
        vn = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        v = v / vn[..., None]
        w = _cross(m1, v)
        f1 = _dot(v, m2)
        f0 = np.arctan2(_dot(w, m2), _dot(m1, m2))
    f = np.stack([f0, f1, f2], axis=-1)
    zero = (L == 0.0) | (vn == 0.0)
    f[zero] = 0.0
    return f


def bin_positions(f):
    """The unfloored bin coordinates of pair features [..., 3]: 11 (f0 + pi) / (2 pi), 11 (f1 + 1) / 2, 11 (f2 + 1) / 2."""
    return np.stack([11.0 * (f[..., 0] + math.pi) / TWO_PI, 11.0 * (f[..., 1] + 1.0) * 0.5, 11.0 * (f[..., 2] + 1.0) * 0.5], axis=-1)


def bins(f):
    """Histogram bins (three per pair feature, already offset by 0 / 11 / 22)."""
    b = np.floor(bin_positions(f))
    b = np.where(~(b > 0.0), 0.0, np.where(b >= 10.0, 10.0, b)).astype(np.int64)
    return b + np.array([0, 11, 22])


def near_edge(f, tol: float = EDGE_TOL):
    """Whether any of the three features lies within tol of a bin edge (in feature units)."""
    x = bin_positions(f)
    e = np.abs(x - np.round(x))
    scale = np.array([TWO_PI / 11.0, 2.0 / 11.0, 2.0 / 11.0])
    return np.any(e * scale < tol, axis=-1)


# ---- SPFH / FPFH ---------------------------------------------------------------------------------------------------------------------
def fpfh(xyz: np.ndarray, normals: np.ndarray, radius: float, max_nn: int, lists=None):
    """FPFH [n, 33] and the mask of points whose features depend on a pair feature near a bin edge."""
    xyz = np.asarray(xyz, np.float64)
    normals = np.asarray(normals, np.float64)
    n = len(xyz)
    idx, d2 = knn_lists(xyz, max_nn) if lists is None else lists
    keep = hybrid(idx, d2, radius)
    m = keep.sum(axis=1)
    qi = np.repeat(np.arange(n), keep.sum(axis=1))
    nj = idx[keep]
    f = pair_features(xyz[qi], normals[qi], xyz[nj], normals[nj])
    b = bins(f)
    inc = np.zeros(n)
    inc[m > 0] = 100.0 / m[m > 0]
    spfh = np.zeros((n, 33))
    # each neighbour adds inc to three bins; a bin that receives c increments holds inc + inc + ... (c times, sequential)
    cnt = np.zeros((n, 33), np.int64)
    for c in range(3):
        np.add.at(cnt, (qi, b[:, c]), 1)
    for t in range(int(cnt.max()) if cnt.size else 0):
        spfh = np.where(cnt > t, spfh + inc[:, None], spfh)
    edge_pt = np.zeros(n, bool)
    np.logical_or.at(edge_pt, qi, near_edge(f))
    # FPFH: sum over the list in order of SPFH(j) / d2 (d2 == 0 skipped), per-block scale 100 / sum, + SPFH(i)
    use = keep & (d2 != 0.0)
    acc = np.zeros((n, 33))
    s = np.zeros((n, 3))
    edge = edge_pt.copy()
    for j in range(idx.shape[1]):
        u = use[:, j]
        if not u.any():
            continue
        jj = idx[u, j]
        val = spfh[jj] / d2[u, j][:, None]
        for c in range(3):  # block sums: sequential over (list entry, bin) inside the block
            sc = s[u, c]
            for bb in range(11 * c, 11 * c + 11):
                sc = sc + val[:, bb]
            s[u, c] = sc
        acc[u] = acc[u] + val
        edge[u] |= edge_pt[jj]
    with np.errstate(divide="ignore"):
        scale = np.where(s != 0.0, 100.0 / s, 0.0)
    sc33 = np.repeat(scale, 11, axis=1)
    out = np.where(sc33 != 0.0, acc * sc33, acc) + spfh
    return out, edge, m


def fpfh_scalar(xyz, normals, radius: float, max_nn: int):
    """A plain scalar-loop transcription of the definition (the check of fpfh() above, on small clouds)."""
    n = len(xyz)
    P = [tuple(map(float, p)) for p in xyz]
    N = [tuple(map(float, v)) for v in normals]
    lists = []
    for i in range(n):
        cand = []
        for j in range(n):
            dx, dy, dz = P[i][0] - P[j][0], P[i][1] - P[j][1], P[i][2] - P[j][2]
            cand.append(((dx * dx + dy * dy) + dz * dz, j))
        cand.sort()
        lists.append([(j, d) for d, j in cand[:max_nn] if j != i and d < radius * radius])

    def pf(p1, n1, p2, n2):
        d = [p2[a] - p1[a] for a in range(3)]
        L = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        if L == 0.0:
            return (0.0, 0.0, 0.0)
        dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
        cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])  # noqa: E731
        a1, a2 = dot(n1, d) / L, dot(n2, d) / L
        if abs(a1) < abs(a2):
            n1, n2, d, f2 = n2, n1, [-x for x in d], -a2
        else:
            f2 = a1
        v = cross(d, n1)
        vn = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        if vn == 0.0:
            return (0.0, 0.0, 0.0)
        v = (v[0] / vn, v[1] / vn, v[2] / vn)
        w = cross(n1, v)
        return (math.atan2(dot(w, n2), dot(n1, n2)), dot(v, n2), f2)

    def clamp(x):
        b = math.floor(x)
        return 0 if not b > 0 else (10 if b >= 10 else int(b))

    spfh = [[0.0] * 33 for _ in range(n)]
    for i in range(n):
        if not lists[i]:
            continue
        inc = 100.0 / len(lists[i])
        for j, _ in lists[i]:
            f = pf(P[i], N[i], P[j], N[j])
            spfh[i][clamp(11.0 * (f[0] + math.pi) / (2.0 * math.pi))] += inc
            spfh[i][11 + clamp(11.0 * (f[1] + 1.0) * 0.5)] += inc
            spfh[i][22 + clamp(11.0 * (f[2] + 1.0) * 0.5)] += inc
    out = np.zeros((n, 33))
    for i in range(n):
        feat = [0.0] * 33
        s = [0.0, 0.0, 0.0]
        for j, d in lists[i]:
            if d == 0.0:
                continue
            for b in range(33):
                val = spfh[j][b] / d
                s[b // 11] += val
                feat[b] += val
        for c in range(3):
            if s[c] != 0.0:
                s[c] = 100.0 / s[c]
        for b in range(33):
            out[i, b] = (feat[b] * s[b // 11] if s[b // 11] != 0.0 else feat[b]) + spfh[i][b]
    return out


# ---- feature matching ----------------------------------------------------------------------------------------------------------------
def feature_nn(Q: np.ndarray, R: np.ndarray, chunk: int = 256) -> np.ndarray:
    """Exact 1-NN of every row of Q among the rows of R: sequential fp64 sum over the 33 dimensions, ties to the smallest index."""
    out = np.empty(len(Q), np.int64)
    for a in range(0, len(Q), chunk):
        q = Q[a:a + chunk]
        D = np.zeros((len(q), len(R)))
        for b in range(Q.shape[1]):
            e = q[:, None, b] - R[None, :, b]
            D = D + e * e
        out[a:a + chunk] = np.argmin(D, axis=1)
    return out


def match(Fs: np.ndarray, Fr: np.ndarray, mutual: bool = True):
    """corr [n_src] (-1 = none) as me_fpfh_match, and the two raw directions."""
    sr = feature_nn(Fs, Fr)
    rs = feature_nn(Fr, Fs)
    corr = sr.copy()
    if mutual:
        corr[rs[sr] != np.arange(len(sr))] = -1
    return corr, sr, rs


# ---- Jacobi / Horn (csrc/me_horn.hpp, operation by operation) ------------------------------------------------------------------------
def jacobi_sym(n: int, a: list):
    a = [float(x) for x in a]
    V = [1.0 if i == j else 0.0 for i in range(n) for j in range(n)]
    for _ in range(100):
        off = 0.0
        for p in range(n):
            for q in range(p + 1, n):
                off += a[n * p + q] * a[n * p + q]
        if off < 1e-300:
            break
        for p in range(n):
            for q in range(p + 1, n):
                apq = a[n * p + q]
                if apq == 0.0:
                    continue
                theta = (a[n * q + q] - a[n * p + p]) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * c
                for k in range(n):
                    akp, akq = a[n * k + p], a[n * k + q]
                    a[n * k + p] = c * akp - sn * akq
                    a[n * k + q] = sn * akp + c * akq
                for k in range(n):
                    apk, aqk = a[n * p + k], a[n * q + k]
                    a[n * p + k] = c * apk - sn * aqk
                    a[n * q + k] = sn * apk + c * aqk
                for k in range(n):
                    vkp, vkq = V[n * k + p], V[n * k + q]
                    V[n * k + p] = c * vkp - sn * vkq
                    V[n * k + q] = sn * vkp + c * vkq
    return [a[n * i + i] for i in range(n)], V


def horn_rotation(S):
    S = [float(x) for x in S]
    N = [S[0] + S[4] + S[8], S[5] - S[7], S[6] - S[2], S[1] - S[3],
         S[5] - S[7], S[0] - S[4] - S[8], S[1] + S[3], S[6] + S[2],
         S[6] - S[2], S[1] + S[3], -S[0] + S[4] - S[8], S[5] + S[7],
         S[1] - S[3], S[6] + S[2], S[5] + S[7], -S[0] - S[4] + S[8]]
    d, V = jacobi_sym(4, N)
    best = 0
    for i in range(1, 4):
        if d[i] > d[best]:
            best = i
    w, x, y, z = V[best], V[4 + best], V[8 + best], V[12 + best]
    return [w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]


def horn_fit3(p, q):
    """[R | t] (3 x 4) of three pairs p_j -> q_j, p and q as [3][3]."""
    p = [[float(v) for v in r] for r in p]
    q = [[float(v) for v in r] for r in q]
    pb = [((p[0][k] + p[1][k]) + p[2][k]) / 3.0 for k in range(3)]
    qb = [((q[0][k] + q[1][k]) + q[2][k]) / 3.0 for k in range(3)]
    S = [((p[0][r] - pb[r]) * (q[0][c] - qb[c]) + (p[1][r] - pb[r]) * (q[1][c] - qb[c])) + (p[2][r] - pb[r]) * (q[2][c] - qb[c])
         for r in range(3) for c in range(3)]
    R = horn_rotation(S)
    T = np.zeros((3, 4))
    for r in range(3):
        T[r, :3] = R[3 * r:3 * r + 3]
        T[r, 3] = qb[r] - ((R[3 * r] * pb[0] + R[3 * r + 1] * pb[1]) + R[3 * r + 2] * pb[2])
    return T


def kabsch_svd(p, q):
    """The reference rotation / translation by SVD (checks horn_fit3 to rounding)."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    pb, qb = p.mean(0), q.mean(0)
    H = (p - pb).T @ (q - qb)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    T = np.zeros((3, 4))
    T[:, :3] = R
    T[:, 3] = qb - R @ pb
    return T


# ---- RANSAC -------------------------------------------------------------------------------------------------------------------------
def samples(seed: int, h: np.ndarray, n_corr: int) -> np.ndarray:
    """The three correspondence indices of hypotheses h: Philox counter (h, 4, 0, 0), key (seed, 0); k_j = mulhi64(w_j, n_corr)."""
    w = philox4x64_10(np.asarray(h, dtype=np.uint64), 4, 0, 0, seed, 0)
    return np.stack([mulhilo64(int(n_corr), w[j])[0] for j in range(3)], axis=-1).astype(np.int64)


def moved_d2(T, s, q):
    x = ((T[0, 0] * s[..., 0] + T[0, 1] * s[..., 1]) + T[0, 2] * s[..., 2]) + T[0, 3]
    y = ((T[1, 0] * s[..., 0] + T[1, 1] * s[..., 1]) + T[1, 2] * s[..., 2]) + T[1, 3]
    z = ((T[2, 0] * s[..., 0] + T[2, 1] * s[..., 1]) + T[2, 2] * s[..., 2]) + T[2, 3]
    dx, dy, dz = x - q[..., 0], y - q[..., 1], z - q[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _norm(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def hypothesis(cs: np.ndarray, cq: np.ndarray, k, eps: float, edge_ratio: float):
    """(valid, T) of one hypothesis with samples k over the correspondence coordinates cs / cq [n_corr, 3]."""
    k0, k1, k2 = (int(v) for v in k)
    if k0 == k1 or k0 == k2 or k1 == k2:
        return False, None
    p = [list(map(float, cs[j])) for j in (k0, k1, k2)]
    q = [list(map(float, cq[j])) for j in (k0, k1, k2)]
    ok = True
    for a in range(3):
        for b in range(a + 1, 3):
            ds, dt = _norm(p[a], p[b]), _norm(q[a], q[b])
            if ds < dt * edge_ratio or dt < ds * edge_ratio:
                ok = False
    e1 = [p[1][a] - p[0][a] for a in range(3)]
    e2 = [p[2][a] - p[0][a] for a in range(3)]
    cr = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
    if dot(cr, cr) <= (1e-12 * dot(e1, e1)) * dot(e2, e2):
        ok = False
    if not ok:
        return False, None
    T = horn_fit3(p, q)
    d2 = moved_d2(T, np.array(p), np.array(q))
    if np.any(d2 > eps * eps):
        return False, None
    return True, T


def ransac_scores_scalar(cs, cq, seed: int, n_hyp: int, eps: float, edge_ratio: float = 0.9):
    """scores [n_hyp] (-1 = invalid) and the fitted T of every valid hypothesis (dict h -> [3, 4]): hypothesis() on every h in turn
    (the check of ransac_scores() below)."""
    cs, cq = np.asarray(cs, np.float64), np.asarray(cq, np.float64)
    ks = samples(seed, np.arange(n_hyp), len(cs))
    scores = np.full(n_hyp, -1, np.int64)
    fits = {}
    for h in range(n_hyp):
        ok, T = hypothesis(cs, cq, ks[h], eps, edge_ratio)
        if ok:
            scores[h] = int(np.count_nonzero(moved_d2(T, cs, cq) < eps * eps))
            fits[h] = T
    return scores, fits


def _edge_len(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def sample_checks(cs, cq, ks, edge_ratio: float):
    """The checks of hypotheses with samples ks [m, 3] that come before the fit, for all of them at once (the same operations as
    hypothesis(), element by element): (coincide [m], passes [m]) — two samples coincide; distinct samples, every edge inside the
    two-sided length check and a non-degenerate source triangle."""
    cs, cq, ks = np.asarray(cs, np.float64), np.asarray(cq, np.float64), np.asarray(ks, np.int64).reshape(-1, 3)
    coincide = (ks[:, 0] == ks[:, 1]) | (ks[:, 0] == ks[:, 2]) | (ks[:, 1] == ks[:, 2])
    p, q = cs[ks], cq[ks]  # [m, 3 samples, 3]
    ok = ~coincide
    for a in range(3):
        for b in range(a + 1, 3):
            ds, dt = _edge_len(p[:, a], p[:, b]), _edge_len(q[:, a], q[:, b])
            ok &= ~((ds < dt * edge_ratio) | (dt < ds * edge_ratio))
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cr = _cross(e1, e2)
    ok &= ~(_dot(cr, cr) <= (1e-12 * _dot(e1, e1)) * _dot(e2, e2))
    return coincide, ok


def ransac_scores(cs, cq, seed: int, n_hyp: int, eps: float, edge_ratio: float = 0.9, hyps=None, score: bool = True):
    """scores (-1 = invalid) and the fitted T of every valid hypothesis (dict h -> [3, 4]).  Without hyps: hypotheses 0 .. n_hyp - 1,
    scores[h].  With hyps (any hypothesis numbers, each a pure function of (seed, h)): scores[t] belongs to hyps[t]; n_hyp is not
    used.  The checks before the fit run on all hypotheses at once (sample_checks) and only those that pass are fitted, one by one,
    by horn_fit3.  score = False: the validity alone, 0 in place of the inlier count."""
    cs, cq = np.asarray(cs, np.float64), np.asarray(cq, np.float64)
    hyps = np.arange(n_hyp, dtype=np.int64) if hyps is None else np.asarray(hyps, np.int64).reshape(-1)
    ks = samples(seed, hyps, len(cs)).reshape(-1, 3)
    _, passes = sample_checks(cs, cq, ks, edge_ratio)
    scores = np.full(len(hyps), -1, np.int64)
    fits = {}
    for t in np.flatnonzero(passes):
        p, q = cs[ks[t]], cq[ks[t]]
        T = horn_fit3(p, q)
        if np.any(moved_d2(T, p, q) > eps * eps):
            continue
        scores[t] = int(np.count_nonzero(moved_d2(T, cs, cq) < eps * eps)) if score else 0
        fits[int(hyps[t])] = T
    return scores, fits


# ---- inputs of the edge tests (test_gpu_globreg_edges.py; what they are meant to exercise is checked on the model in test_globreg_cpu.py)
def unit_normals(n: int, seed: int) -> np.ndarray:
    """n random unit vectors."""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def three_planes(n_per: int = 1000, side: float = 17.0, seed: int = 1, noise: float = 0.02) -> np.ndarray:
    """Three noisy orthogonal planes (x = 0, y = 0, z = 0), n_per points on side x side each, coordinates rounded to 2^-8: sums and
    differences of such coordinates (and of shifts by integers) are exact in fp64.  About 3.5 points / m^2 by default."""
    rng = np.random.default_rng(seed)
    parts = []
    for axis in range(3):
        p = rng.uniform(0.0, side, (n_per, 3))
        p[:, axis] = rng.normal(scale=noise, size=n_per)
        parts.append(p)
    return np.round(np.concatenate(parts) * 256.0) / 256.0


def tripled_cloud(n: int = 200, seed: int = 2):
    """n points on a noisy 4 m x 4 m patch, each three times in a row (np.repeat: copies are adjacent in index), and unit normals that
    are the same for the copies of a point."""
    rng = np.random.default_rng(seed)
    p = np.column_stack([rng.uniform(0, 4, n), rng.uniform(0, 4, n), rng.normal(scale=0.05, size=n)])
    return np.repeat(p, 3, axis=0), np.repeat(unit_normals(n, seed + 1), 3, axis=0)


def lattice_cloud(nx: int = 12, ny: int = 12, nz: int = 2) -> np.ndarray:
    """The integer lattice nx x ny x nz: squared distances are small integers, so d2 == radius^2 occurs exactly."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1)
    return g.reshape(-1, 3).astype(np.float64)


def rotation(yaw: float, roll: float = 0.0, pitch: float = 0.0) -> np.ndarray:
    cz, sz, cx, sx, cy, sy = math.cos(yaw), math.sin(yaw), math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return Rz @ Ry @ Rx


def moved_points(T, s) -> np.ndarray:
    """The points s [n, 3] moved by T ([3, 4] or [4, 4]) in the library's order: ((T_r0 x + T_r1 y) + T_r2 z) + T_r3."""
    return np.stack([((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)], axis=1)


def ransac_pair(n_extra: int = 3000, noise: float = 0.06, seed: int = 11):
    """(src, src normals, ref, ref normals, R0, t0): the reference is three planes plus an unrelated cluster 100 m away; the source is
    a noisy copy of the three planes plus another unrelated cluster, moved by (R0, t0).  The clusters only yield wrong feature matches,
    so that most RANSAC samples fail one of the checks."""
    rng = np.random.default_rng(seed + 2)
    a, na = three_planes(seed=seed), unit_normals(3000, seed + 1)
    side, shift = 17.0 * math.sqrt(n_extra / 1000.0), np.array([100.0, 0.0, 0.0])
    ref = np.concatenate([a, three_planes(n_extra, side, seed + 3) + shift])
    nr = np.concatenate([na, unit_normals(3 * n_extra, seed + 4)])
    base = np.concatenate([a + rng.normal(scale=noise, size=a.shape), three_planes(n_extra, side, seed + 5) + shift])
    nb = np.concatenate([na, unit_normals(3 * n_extra, seed + 6)])
    R0, t0 = rotation(1.9, 0.03, 0.02), np.array([25.0, 14.0, -2.0])
    return base @ R0.T + t0, nb @ R0.T, ref, nr, R0, t0
