"""Brute-force numpy model of me_ray.hip: every ray against every triangle, no boxes, no tree.  The
ray-triangle routine is restated operation by operation (numpy rounds every product, sum and quotient on its own, which is what the
library's -ffp-contract=off build does), so t, tri, u, v and the flags are compared with ==."""
import numpy as np

import _perturb_ref as P

HIT, BACKFACE, INVALID = 1, 2, 4
GATE = 2.0 ** -40


def transform(vertices, T):
    """me_mesh_upload's optional transform: h[r] = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3], p = h[:3] / h[3]."""
    v = np.asarray(vertices, np.float64)
    if T is None:
        return v.copy()
    T = np.asarray(T, np.float64).reshape(4, 4)
    if np.array_equal(T, np.eye(4)):
        return v.copy()
    h = [((T[r, 0] * v[:, 0] + T[r, 1] * v[:, 1]) + T[r, 2] * v[:, 2]) + T[r, 3] for r in range(4)]
    return np.stack([h[0] / h[3], h[1] / h[3], h[2] / h[3]], -1)


def corners(vertices, triangles, T=None):
    """(F, 3, 3) corner coordinates in the caller's triangle order."""
    return transform(vertices, T)[np.asarray(triangles, np.int64)]


def normal(tri):
    """n = (B - A) x (C - A) in the component form u1*v2 - u2*v1 (the upload's and the gate's)."""
    u, v = tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :]
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def edge(px, py, qx, qy):
    """The edge function of edge P -> Q seen from the origin of the sheared plane: Qx*Py - Qy*Px."""
    return qx * py - qy * px


def ray_frame(o, d):
    """valid, (kx, ky, kz), (Sx, Sy, Sz), dd per ray."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    a = np.abs(d)
    kz = np.zeros(len(d), np.int64)
    am = a[:, 0].copy()
    for k in (1, 2):
        m = a[:, k] > am
        kz[m] = k
        am[m] = a[m, k]
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    r = np.arange(len(d))
    neg = d[r, kz] < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    with np.errstate(all="ignore"):
        S = np.stack([d[r, kx] / d[r, kz], d[r, ky] / d[r, kz], 1.0 / d[r, kz]], -1)
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (am > 0)
    return valid, np.stack([kx, ky, kz], -1), S, dd


def ray_tri_all(tri, o, d, t_min, t_max):
    """Every ray against every triangle -> hit (R, F) bool, t, u, v, back (R, F).  t_min / t_max: scalars or per-ray arrays."""
    tri = np.asarray(tri, np.float64)
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    R, F = len(o), len(tri)
    t_min = np.broadcast_to(np.asarray(t_min, np.float64), (R,))[:, None]
    t_max = np.broadcast_to(np.asarray(t_max, np.float64), (R,))[:, None]
    valid, K, S, dd = ray_frame(o, d)
    n = normal(tri)
    deg = (n == 0).all(-1)
    r = np.arange(R)
    with np.errstate(all="ignore"):
        c = (n[None, :, 0] * d[:, None, 0] + n[None, :, 1] * d[:, None, 1]) + n[None, :, 2] * d[:, None, 2]
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        graze = c * c < GATE * (nn[None, :] * dd[:, None])
        sh = []
        zs = []
        for corner in range(3):
            p = tri[None, :, corner, :] - o[:, None, :]  # (R, F, 3)  A' = A - o
            pk = [np.take_along_axis(p, np.broadcast_to(K[:, None, j:j + 1], (R, F, 1)), 2)[..., 0] for j in range(3)]
            sh.append((pk[0] - S[:, None, 0] * pk[2], pk[1] - S[:, None, 1] * pk[2]))
            zs.append(S[:, None, 2] * pk[2])
        (Ax, Ay), (Bx, By), (Cx, Cy) = sh
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        T = (U * zs[0] + V * zs[1]) + W * zs[2]
        t = T / det
        hit = valid[:, None] & ~deg[None, :] & ~graze & ~mixed & (det != 0) & (t_min <= t) & (t <= t_max)
        u, v = V / det, W / det
    return hit, t, u, v, det < 0


def cast(tri, o, d, t_min=0.0, t_max=np.inf, chunk=256):
    """Closest hit per ray: the lexicographic minimum of (t, triangle index).  -> dict t, tri, u, v, flags, any and the totals."""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    R = len(o)
    t_min = np.broadcast_to(np.asarray(t_min, np.float64), (R,))
    t_max = np.broadcast_to(np.asarray(t_max, np.float64), (R,))
    out = {"t": np.full(R, np.inf), "tri": np.full(R, -1, np.int32), "u": np.zeros(R), "v": np.zeros(R), "flags": np.zeros(R, np.uint8)}
    valid = ray_frame(o, d)[0]
    for a in range(0, R, chunk):
        s = slice(a, min(R, a + chunk))
        hit, t, u, v, back = ray_tri_all(tri, o[s], d[s], t_min[s], t_max[s])
        th = np.where(hit, t, np.inf)
        best = th.min(1)
        win = np.argmax(hit & (th == best[:, None]), 1)  # the first index among the equal smallest t
        has = hit.any(1)
        r = np.arange(len(best))
        out["t"][s] = np.where(has, t[r, win], np.inf)
        out["tri"][s] = np.where(has, win, -1)
        out["u"][s] = np.where(has, u[r, win], 0.0)
        out["v"][s] = np.where(has, v[r, win], 0.0)
        out["flags"][s] = has * HIT + (has & back[r, win]) * BACKFACE
    out["flags"] = (out["flags"] + (~valid) * INVALID).astype(np.uint8)
    has = (out["flags"] & HIT) != 0
    out["any"] = has
    out.update(n_rays=R, n_hit=int(has.sum()), n_backface=int(((out["flags"] & BACKFACE) != 0).sum()), n_invalid=int((~valid).sum()),
               min_t=float(out["t"][has].min()) if has.any() else np.inf, max_t=float(out["t"][has].max()) if has.any() else -np.inf)
    return out


def any_hit(tri, o, d, t_min=0.0, t_max=np.inf, chunk=256):
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    R = len(o)
    t_min = np.broadcast_to(np.asarray(t_min, np.float64), (R,))
    t_max = np.broadcast_to(np.asarray(t_max, np.float64), (R,))
    res = np.zeros(R, bool)
    for a in range(0, R, chunk):
        s = slice(a, min(R, a + chunk))
        res[s] = ray_tri_all(tri, o[s], d[s], t_min[s], t_max[s])[0].any(1)
    return res


def scan_rays(poses, dirs):
    """Ray p * nd + b: o = the pose's translation, d_w[k] = (R[k][0] dx + R[k][1] dy) + R[k][2] dz."""
    P4 = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
    m, nd = len(P4), len(dirs)
    o = np.repeat(P4[:, :3, 3], nd, axis=0)
    Rm = np.repeat(P4[:, :3, :3], nd, axis=0)
    dl = np.tile(dirs, (m, 1))
    d = np.stack([(Rm[:, k, 0] * dl[:, 0] + Rm[:, k, 1] * dl[:, 1]) + Rm[:, k, 2] * dl[:, 2] for k in range(3)], -1)
    return o, d


def scan(tri, poses, dirs, min_range=0.0, max_range=np.inf, noise_std=0.0, seed=0):
    """-> points (in ray order), ray_id, pose_hits, n_hit, n_backface, and (for the noise tolerance) the noiseless points and z."""
    o, d = scan_rays(poses, dirs)
    m, nd = len(np.asarray(poses).reshape(-1, 16)), len(np.asarray(dirs).reshape(-1, 3))
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    with np.errstate(all="ignore"):
        c = cast(tri, o, d, min_range / ln, max_range / ln)
    has = c["any"]
    ids = np.nonzero(has)[0].astype(np.int64)
    t = c["t"][has]
    clean = o[has] + t[:, None] * d[has]
    z = np.zeros(len(ids))
    if noise_std > 0 and len(ids):
        w = P.philox4x64_10(ids.astype(np.uint64), 6, 0, 0, seed, 0)
        z = P.box_muller(w[0], w[1])[0]
        t = t + (noise_std * z) / ln[has]
    pts = o[has] + t[:, None] * d[has]
    return {"points": pts, "clean": clean, "z": z, "ray_id": ids, "pose_hits": np.bincount(ids // nd, minlength=m).astype(np.int64),
            "n_rays": m * nd, "n_hit": len(ids), "n_backface": c["n_backface"], "len": ln[has], "dir": d[has]}


def visibility(tri, pts, origins, min_range=0.0, max_range=np.inf, tolerance=0.0, first_only=False):
    """-> n_seen, first_seen (cloud order) and the totals of me_cloud_visibility."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    origins = np.asarray(origins, np.float64).reshape(-1, 3)
    n = len(pts)
    n_seen, first = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    in_range_any = np.zeros(n, bool)
    n_tests = 0
    for j, oj in enumerate(origins):
        todo = np.ones(n, bool) if not first_only else first < 0
        d = pts - oj[None, :]
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        with np.errstate(all="ignore"):
            inr = todo & (min_range <= ln) & (ln <= max_range)
            near = inr & (ln <= tolerance)
            castm = inr & ~near
            valid = ray_frame(np.broadcast_to(oj, d.shape), d)[0]
            tests = castm & valid
            occ = np.zeros(n, bool)
            if tests.any():
                occ[tests] = any_hit(tri, np.broadcast_to(oj, d.shape)[tests], d[tests], 0.0, ((ln - tolerance) / ln)[tests])
        n_tests += int(tests.sum())
        seen = near | (tests & ~occ)
        in_range_any |= inr
        first[seen & (first < 0)] = j
        n_seen[seen] += 1
    return {"n_seen": n_seen, "first_seen": first, "n_points": n, "n_visible": int((n_seen > 0).sum()), "n_in_range": int(in_range_any.sum()),
            "n_tests": n_tests}
