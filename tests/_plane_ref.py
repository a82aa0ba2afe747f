"""numpy model of the RANSAC plane segmentation (csrc/me_plane.hip; the definition is in include/mapeval_hip.h), with every operation
in the library's order, so that scores, winners and labels can be compared exactly.  Philox, the 64-bit high product and the cross /
dot helpers come from _globreg_ref.py.  segment() is the vectorised model, segment_scalar() a plain restatement of the hypothesis /
score / winner loop in scalar Python (the check of the former on small clouds)."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from _globreg_ref import _cross, _dot, mulhilo64, philox4x64_10

USER_ID = 5  # Philox counter word 1 of me_segment_planes
TILE = 1024  # points of one block tile of k_plane_score (256 lanes x 4 points)
HYP_CHUNK = 256  # hypotheses per block of k_plane_score


def samples(seed: int, h, r: int, m: int) -> np.ndarray:
    """The three sample positions of hypotheses h in round r over m remaining points: counter (h, 5, r, 0), key (seed, 0)."""
    w = philox4x64_10(np.asarray(h, dtype=np.uint64), USER_ID, r, 0, seed, 0)
    return np.stack([mulhilo64(int(m), w[j])[0] for j in range(3)], axis=-1).astype(np.int64)


def _sign(n: np.ndarray) -> np.ndarray:
    flip = (n[..., 2] < 0) | ((n[..., 2] == 0) & (n[..., 1] < 0)) | ((n[..., 2] == 0) & (n[..., 1] == 0) & (n[..., 0] < 0))
    return np.where(flip[..., None], -n, n)


def hypotheses(pts: np.ndarray, seed: int, r: int, H: int):
    """(valid [H], planes [H, 4], k0 [H]) of round r over the remaining points pts [m, 3] (m >= 3)."""
    ks = samples(seed, np.arange(H), r, len(pts)).reshape(-1, 3)
    coincide = (ks[:, 0] == ks[:, 1]) | (ks[:, 0] == ks[:, 2]) | (ks[:, 1] == ks[:, 2])
    p = pts[ks]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cr = _cross(e1, e2)
    cc = _dot(cr, cr)
    valid = ~coincide & ~(cc <= (1e-12 * _dot(e1, e1)) * _dot(e2, e2))
    with np.errstate(divide="ignore", invalid="ignore"):
        n = _sign(cr / np.sqrt(cc)[:, None])
    d = -((n[:, 0] * p[:, 0, 0] + n[:, 1] * p[:, 0, 1]) + n[:, 2] * p[:, 0, 2])
    planes = np.concatenate([n, d[:, None]], axis=1)
    planes[~valid] = (0.0, 0.0, 0.0, np.inf)
    return valid, planes, ks[:, 0]


def residuals(pts: np.ndarray, plane) -> np.ndarray:
    return ((plane[0] * pts[:, 0] + plane[1] * pts[:, 1]) + plane[2] * pts[:, 2]) + plane[3]


def scores_of(pts: np.ndarray, valid, planes, t: float, chunk: int = 64) -> np.ndarray:
    out = np.full(len(planes), -1, np.int64)
    for a in range(0, len(planes), chunk):
        pl = planes[a:a + chunk]
        with np.errstate(invalid="ignore"):
            s = ((pl[:, 0, None] * pts[None, :, 0] + pl[:, 1, None] * pts[None, :, 1]) + pl[:, 2, None] * pts[None, :, 2]) + pl[:, 3, None]
        out[a:a + chunk] = np.count_nonzero(np.abs(s) < t, axis=1)
    out[~np.asarray(valid)] = -1
    return out


def refit_exact(inl: np.ndarray):
    """Least-squares plane of the points: the covariance about the mean formed EXACTLY (rational arithmetic on the binary fractions
    the coordinates are), rounded once per entry, then numpy.linalg.eigh.  Returns (plane, eigenvalues ascending, centroid)."""
    k = len(inl)
    P = [[Fraction(float(v)) for v in row] for row in inl]
    mean = [sum(row[a] for row in P) / k for a in range(3)]
    C = np.array([[float(sum((row[a] - mean[a]) * (row[b] - mean[b]) for row in P) / k) for b in range(3)] for a in range(3)])
    w, V = np.linalg.eigh(C)
    n = _sign(V[:, 0])
    cen = np.array([float(v) for v in mean])
    return np.array([n[0], n[1], n[2], -float(n @ cen)]), w, cen


def segment(xyz, t: float, H: int, P: int = 1, min_inliers: int = 3, seed: int = 0):
    """The model of me_segment_planes with refit = 0 (the refit never changes scores or labels).  Returns a dict: scores [P, H] (-1:
    invalid or round not reached), labels [N], records (count, h, score, plane, k0 = the cloud index of the winner's p0) and info."""
    xyz = np.asarray(xyz, np.float64)
    n = len(xyz)
    labels = np.full(n, -1, np.int32)
    scores = np.full((P, H), -1, np.int64)
    recs = []
    n_valid = rounds = 0
    for r in range(P):
        rounds += 1
        rem = np.flatnonzero(labels < 0)
        if len(rem) < 3:
            break
        pts = xyz[rem]
        valid, planes, k0 = hypotheses(pts, seed, r, H)
        sc = scores_of(pts, valid, planes, t)
        scores[r] = sc
        n_valid += int(valid.sum())
        if not valid.any():
            break
        h = int(np.argmax(sc))  # (the first of the largest: ties to the smallest h)
        if sc[h] < min_inliers:
            break
        inl = np.abs(residuals(pts, planes[h])) < t
        assert int(inl.sum()) == sc[h]
        labels[rem[inl]] = r
        recs.append({"count": int(sc[h]), "h": h, "score": int(sc[h]), "plane": planes[h].copy(), "k0": int(rem[k0[h]])})
    info = {"n_in": n, "n_planes": len(recs), "n_labelled": int((labels >= 0).sum()), "n_valid_hypotheses": n_valid, "rounds": rounds}
    return {"scores": scores, "labels": labels, "records": recs, "info": info}


def segment_scalar(xyz, t: float, H: int, P: int = 1, min_inliers: int = 3, seed: int = 0):
    """The hypothesis / score / winner loop once more, one Python float operation at a time: (scores, labels, winners)."""
    pts_all = [tuple(map(float, p)) for p in np.asarray(xyz, np.float64)]
    n = len(pts_all)
    labels = [-1] * n
    scores = [[-1] * H for _ in range(P)]
    winners = []
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
    for r in range(P):
        rem = [i for i in range(n) if labels[i] < 0]
        m = len(rem)
        if m < 3:
            break
        ks = samples(seed, np.arange(H), r, m).reshape(-1, 3)
        best, best_h, best_plane = -1, -1, None
        for h in range(H):
            k0, k1, k2 = (int(v) for v in ks[h])
            if k0 == k1 or k0 == k2 or k1 == k2:
                continue
            p0, p1, p2 = pts_all[rem[k0]], pts_all[rem[k1]], pts_all[rem[k2]]
            e1 = [p1[a] - p0[a] for a in range(3)]
            e2 = [p2[a] - p0[a] for a in range(3)]
            cr = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
            cc = dot(cr, cr)
            if cc <= (1e-12 * dot(e1, e1)) * dot(e2, e2):
                continue
            L = math.sqrt(cc)
            a, b, c = cr[0] / L, cr[1] / L, cr[2] / L
            if c < 0 or (c == 0 and b < 0) or (c == 0 and b == 0 and a < 0):
                a, b, c = -a, -b, -c
            d = -((a * p0[0] + b * p0[1]) + c * p0[2])
            cnt = 0
            for i in rem:
                x, y, z = pts_all[i]
                if abs(((a * x + b * y) + c * z) + d) < t:
                    cnt += 1
            scores[r][h] = cnt
            if cnt > best:
                best, best_h, best_plane = cnt, h, (a, b, c, d)
        if best_h < 0 or best < min_inliers:
            break
        a, b, c, d = best_plane
        for i in rem:
            x, y, z = pts_all[i]
            if abs(((a * x + b * y) + c * z) + d) < t:
                labels[i] = r
        winners.append(best_h)
    return np.array(scores, np.int64), np.array(labels, np.int32), winners


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def lattice_planes(nz: int = 12, nx: int = 10, ny: int = 8, shuffle_seed: int | None = 3) -> np.ndarray:
    """Noise-free axis-aligned lattice planes with integer coordinates: z = 0 (nz x nz points, x, y in 1 .. nz), x = 0 (nx x nx points,
    y, z in 1 .. nx) and y = 0 (ny x ny points, x, z in 1 .. ny); no point lies on two of them.  nz > nx > ny: the r-th largest is the
    r-th in this list.  Any other plane holds far fewer lattice points than the smallest of the three."""
    def grid(m):
        g = np.stack(np.meshgrid(np.arange(1, m + 1), np.arange(1, m + 1), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
        return g

    a, b, c = grid(nz), grid(nx), grid(ny)
    pts = np.concatenate([np.column_stack([a[:, 0], a[:, 1], np.zeros(len(a))]), np.column_stack([np.zeros(len(b)), b[:, 0], b[:, 1]]),
                          np.column_stack([c[:, 0], np.zeros(len(c)), c[:, 1]])])
    if shuffle_seed is not None:
        pts = pts[np.random.default_rng(shuffle_seed).permutation(len(pts))]
    return pts


def lattice_expected_labels(pts: np.ndarray) -> np.ndarray:
    """The derivable labelling of lattice_planes(): z = 0 -> 0, x = 0 -> 1, y = 0 -> 2."""
    return np.where(pts[:, 2] == 0, 0, np.where(pts[:, 0] == 0, 1, 2)).astype(np.int32)


def collinear(n: int = 50) -> np.ndarray:
    return np.column_stack([np.arange(n) * 0.5, np.arange(n) * 0.25 + 1.0, np.arange(n) * 0.125 - 2.0])
