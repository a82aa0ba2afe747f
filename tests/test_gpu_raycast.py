"""me_ray.hip on the GPU against the brute-force model (tests/_ray_ref.py): t, tri, u, v and the flags EQUAL on every ray, equal totals,
identical bytes from two calls, any-hit equal to "a closest hit exists" — on one triangle at its edges, across the tree's sizes, on
ties, watertight closed meshes (also at survey coordinates), the grazing gate at one ulp and prune adversaries; the scan, the
visibility with its keep mask, observable_report, and the state rules."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ray_ref as R  # noqa: E402
from cloud_map_evaluation_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

EST, GT = 0, 1
U = 2.0 ** -53
INF = math.inf


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _check(e, corners, o, d, t_min=0.0, t_max=INF):
    """Closest hit == model on every ray and in the totals, two calls give the same bytes, any-hit == "a closest hit exists"."""
    o, d = np.ascontiguousarray(o, np.float64).reshape(-1, 3), np.ascontiguousarray(d, np.float64).reshape(-1, 3)
    ref = R.cast(corners, o, d, t_min, t_max)
    got = e.mesh_raycast(o, d, t_min, t_max)
    for k in ("tri", "flags", "t", "u", "v"):
        bad = np.nonzero(_bits(got[k]) != _bits(ref[k]))[0]
        assert bad.size == 0, (k, bad[:5], got[k][bad[:5]], ref[k][bad[:5]], o[bad[:5]], d[bad[:5]])
    for k in ("n_rays", "n_hit", "n_backface", "n_invalid", "min_t", "max_t"):
        assert got[k] == ref[k], k
    again = e.mesh_raycast(o, d, t_min, t_max)
    for k in ("tri", "flags", "t", "u", "v"):
        assert np.array_equal(_bits(again[k]), _bits(got[k])), k
    occ = e.mesh_raycast(o, d, t_min, t_max, any_hit=True)
    assert np.array_equal((occ["flags"] & R.HIT) != 0, ref["any"])
    assert np.array_equal((occ["flags"] & R.INVALID) != 0, (ref["flags"] & R.INVALID) != 0)
    assert occ["n_hit"] == ref["n_hit"] and (occ["tri"] == -1).all() and np.isinf(occ["t"]).all()
    return ref


def _soup(corners):
    """(F,3,3) corners -> (vertices, triangles) with every triangle its own three vertices."""
    c = np.asarray(corners, np.float64)
    return c.reshape(-1, 3), np.arange(3 * len(c), dtype=np.int32).reshape(-1, 3)


# ---- one triangle -------------------------------------------------------------------------------------------------------------------
TRI1 = np.array([[[0.25, 0.5, 1.0], [2.25, 0.75, 1.5], [0.75, 2.5, 0.5]]])


def _one_triangle_rays():
    A, B, C = TRI1[0]
    rng = np.random.default_rng(5)
    o, d = [], []
    for _ in range(20):  # interior hits from the front (+n side looks down -n) and from the back
        w = rng.dirichlet([1, 1, 1])
        p = w[0] * A + w[1] * B + w[2] * C
        org = p + rng.normal(size=3) * [0.3, 0.3, 0.0] + [0.0, 0.0, rng.choice([-3.0, 3.0])]
        o.append(org), d.append(p - org)
    for _ in range(12):  # misses beside the triangle
        p = A + rng.uniform(1.2, 3.0) * (B - A) + rng.uniform(1.2, 3.0) * (C - A)
        o.append(p + [0.0, 0.0, 4.0]), d.append([0.0, 0.0, -1.0])
    for p in (A, B, C, 0.5 * (A + B), 0.5 * (B + C), 0.5 * (C + A)):  # through each vertex and each edge midpoint, two directions each
        o.append(p + [0.0, 0.0, 2.0]), d.append([0.0, 0.0, -1.0])
        o.append(p + [0.5, -0.25, -2.0]), d.append([-0.5, 0.25, 2.0])
    cen = 0.5 * A + 0.25 * B + 0.25 * C  # (dyadic: exactly on the plane)
    o.append(cen - 2.0 * (B - A)), d.append(B - A)          # in the plane: grazing, a miss
    o.append(cen - 2.0 * (C - A)), d.append(2.0 * (C - A))
    o.append(cen + [0.0, 0.0, 1.0]), d.append([0.0, 0.0, 0.0])  # d = 0: INVALID
    o.append(cen + [0.0, 0.0, 1.0]), d.append([0.0, np.nan, -1.0])
    o.append(cen), d.append([0.0, 0.0, -1.0])               # origin on the triangle, t_min = 0
    o.append(cen), d.append([0.1, 0.2, 1.0])
    o.append(cen + [0.0, 0.0, 1.0]), d.append([0.0, 0.0, 1.0])  # pointing away
    while len(o) < 64:
        o.append(rng.normal(size=3) * 2.0 + [1.0, 1.0, 3.0]), d.append(rng.normal(size=3))
    return np.array(o[:64], np.float64), np.array(d[:64], np.float64)


def test_one_triangle_64_rays():
    o, d = _one_triangle_rays()
    with _engine() as e:
        e.mesh_upload(*_soup(TRI1))
        ref = _check(e, TRI1, o, d)
        assert 20 <= ref["n_hit"] < 64 and 0 < ref["n_backface"] < ref["n_hit"] and ref["n_invalid"] == 2
        hit = (ref["flags"] & R.HIT) != 0
        assert hit[32:44].sum() >= 6  # vertices and edge midpoints: the model decides which side of a rounding each falls on
        assert not hit[44:48].any() and ref["t"][48] == 0.0 and hit[48] and not hit[50]
        # t_max and t_min exactly at a hit, one ulp below and one ulp above
        k = int(np.nonzero(hit & (ref["t"] > 0))[0][0])
        t0 = float(ref["t"][k])
        lo, hi = np.nextafter(t0, 0.0), np.nextafter(t0, INF)
        for t_min, t_max, want in ((0.0, t0, True), (0.0, lo, False), (0.0, hi, True), (t0, INF, True), (lo, INF, True), (hi, INF, False),
                                   (t0, t0, True)):
            r = _check(e, TRI1, o[k:k + 1], d[k:k + 1], t_min, t_max)
            assert bool(r["any"][0]) == want, (t_min, t_max)


# ---- the tree's sizes ---------------------------------------------------------------------------------------------------------------
def _strip(nt, amplitude):
    v, tri = synth.heightfield_mesh((nt + 1) // 2 + 1, 2, 0.5, amplitude, seed=nt)
    return v, tri[:nt]


def _strip_rays(v, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    diam = float(np.linalg.norm(hi - lo))
    cen = 0.5 * (lo + hi)
    kind = np.arange(n) % 6
    tgt = lo + rng.uniform(-0.1, 1.1, (n, 3)) * (hi - lo)
    o = tgt + np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(1.0, 3.0, n)], -1)  # 0: from above
    ob = tgt + np.stack([rng.uniform(-4, 4, n), rng.uniform(-4, 4, n), rng.uniform(0.3, 2.0, n)], -1)         # 1: obliquely
    o[kind == 1] = ob[kind == 1]
    d = tgt - o
    ax = kind == 2                                                                                                # 2: axis-parallel
    axis = rng.integers(0, 3, n)
    oa = tgt.copy()
    oa[np.arange(n), axis] = (lo - 1.0)[axis]
    o[ax] = oa[ax]
    da = np.zeros((n, 3))
    da[np.arange(n), axis] = rng.choice([0.5, 1.0, 3.0], n)
    d[ax] = da[ax]
    neg = ax & (rng.uniform(size=n) < 0.5)  # half of them from the far side, against the axis
    o[neg] = np.where(da[neg] != 0, (hi + 1.0)[None, :], o[neg])
    d[neg] = -da[neg]
    ins = kind == 3                                                                                               # 3: origin inside the box
    o[ins] = (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo))[ins]
    d[ins] = rng.normal(size=(n, 3))[ins]
    far = kind == 4                                                                                               # 4: 1000 diameters away
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    o[far] = (tgt + 1000.0 * max(diam, 1.0) * dirs)[far]
    d[far] = (tgt - o)[far]
    vert = kind == 5                                                                                              # 5: straight down onto the lattice
    o[vert] = (np.round(tgt * 4.0) / 4.0 + [0.0, 0.0, 5.0])[vert]
    d[vert] = [0.0, 0.0, -2.0]
    return o, d


@pytest.mark.parametrize("amplitude", [0.3, 0.0])
@pytest.mark.parametrize("nt", [1, 7, 8, 9, 64, 65, 512, 513])
def test_tree_edges(nt, amplitude):
    v, tri = _strip(nt, amplitude)
    corners = R.corners(v, tri)
    with _engine() as e:
        e.mesh_upload(v, tri)
        assert e.mesh_info()["triangles"] == nt
        for n in (1, 63, 64, 65, 4097):
            o, d = _strip_rays(v, n, seed=1000 * nt + n)
            ref = _check(e, corners, o, d)
            if n == 4097:
                assert 0.2 * n < ref["n_hit"] < n
        o, d = _strip_rays(v, 65, seed=nt)
        _check(e, corners, o, d, 0.25, 1.0)  # a bounded interval: hits before t_min and beyond t_max are none


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def _cube():
    v = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # outward
    tri = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, tri


def _tetra():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


def _edges(tri):
    return sorted({tuple(sorted((int(t[i]), int(t[(i + 1) % 3])))) for t in tri for i in range(3)})


def test_ties_resolve_by_the_smaller_index():
    v, tri = synth.heightfield_mesh(9, 6, 0.5, 0.3, seed=4)
    dup = np.concatenate([tri, tri])[np.random.default_rng(2).permutation(2 * len(tri))]
    with _engine() as e:
        e.mesh_upload(v, dup)
        o, d = _strip_rays(v, 513, seed=8)
        ref = _check(e, R.corners(v, dup), o, d)
        first = {}
        for i, t in enumerate(map(tuple, dup)):
            first.setdefault(t, i)
        hit = ref["tri"] >= 0
        assert hit.sum() > 100 and all(first[tuple(dup[i])] == i for i in ref["tri"][hit])
        # a closed cube and a fan of 6 around one vertex: rays aimed exactly at shared edges and the shared vertex
        cv, ct = _cube()
        cv = cv * 2.0 + [1.0, -1.0, 0.5]
        e.mesh_upload(cv, ct)
        org = np.array([9.0, 7.0, 6.0])
        tg = [cv[a] + s * (cv[b] - cv[a]) for a, b in _edges(ct) for s in (0.0, 0.25, 0.5, 1.0)]
        ref = _check(e, R.corners(cv, ct), np.tile(org, (len(tg), 1)), np.array(tg) - org)
        assert ref["n_hit"] > len(tg) // 2
        ang = 2.0 * np.pi * np.arange(6) / 6.0
        fv = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([np.cos(ang), np.sin(ang), 0.1 * np.cos(3 * ang)], -1)])
        ft = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)], np.int32)
        e.mesh_upload(fv, ft)
        tg = [fv[0]] + [s * fv[1 + k] for k in range(6) for s in (0.25, 0.5, 1.0)]
        for org in (np.array([0.0, 0.0, 4.0]), np.array([0.5, -0.25, 2.0])):
            ref = _check(e, R.corners(fv, ft), np.tile(org, (len(tg), 1)), np.array(tg) - org)
            assert ref["flags"][0] & R.HIT and ref["n_hit"] > len(tg) // 2


# ---- watertight ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [None, (4.0e5, 3.0e6, 100.0)])
@pytest.mark.parametrize("shape", ["cube", "tetra"])
def test_watertight_from_inside(shape, shift):
    v, tri = _cube() if shape == "cube" else _tetra()
    v = v * 3.0 + [0.125, -0.5, 0.75]
    T = None
    if shift is not None:
        T = np.eye(4)
        T[:3, 3] = shift
    w = R.transform(v, T)
    corners = w[tri]
    rng = np.random.default_rng(17)
    inside = w.mean(0) + (0.05 if shape == "tetra" else 0.4) * rng.uniform(-1, 1, 3)
    ed = _edges(tri)
    tg = [p for p in w] + [0.5 * (w[a] + w[b]) for a, b in ed]
    for _ in range(4096):
        a, b = ed[rng.integers(len(ed))]
        tg.append(w[a] + rng.uniform() * (w[b] - w[a]))
    tg = np.array(tg)
    with _engine() as e:
        e.mesh_upload(v, tri, T)
        ref = _check(e, corners, np.tile(inside, (len(tg), 1)), tg - inside)
        assert ref["n_hit"] == ref["n_rays"] == len(tg)
        assert ref["n_backface"] == ref["n_hit"]  # outward winding seen from inside


# ---- the grazing gate ---------------------------------------------------------------------------------------------------------------
def test_grazing_gate_at_one_ulp():
    tri = np.array([[[-4.0, -4.0, 0.0], [4.0, -4.0, 0.0], [0.0, 5.0, 0.0]]])
    nz = float(R.normal(tri)[0, 2])
    dx = 1.0
    # c*c = (nz dz)^2 against 2^-40 (nz^2 (dx^2 + dz^2)), both as the routine rounds them; walk dz over the ulps around the crossing
    def passes(dz):
        return (nz * dz) * (nz * dz) >= R.GATE * ((nz * nz) * ((dx * dx + 0.0) + dz * dz))

    a, b = np.float64(2.0 ** -20).view(np.int64), np.float64(2.0 ** -20 * (1 + 2.0 ** -30)).view(np.int64)
    assert not passes(a.view(np.float64)) and passes(b.view(np.float64))
    while b - a > 1:  # bisection over the doubles in between, by their bit patterns
        m = np.int64((int(a) + int(b)) // 2)
        if passes(m.view(np.float64)):
            b = m
        else:
            a = m
    cand = np.arange(int(a) - 3, int(a) + 5, dtype=np.int64).view(np.float64)
    lhs = (nz * cand) * (nz * cand)
    rhs = R.GATE * ((nz * nz) * ((dx * dx + 0.0) + cand * cand))
    assert (lhs < rhs).any() and (lhs >= rhs).any()
    k = int(np.nonzero(lhs >= rhs)[0][0])  # the first dz that passes the gate; the one below it does not
    assert k > 0 and lhs[k - 1] < rhs[k - 1]
    dzs = np.array([cand[k - 1], cand[k], cand[k + 1]])
    d = np.stack([np.full(3, dx), np.zeros(3), -dzs], -1)
    o = np.array([0.0, 0.0, 0.0]) - 1.0 * d
    o[:, 2] = dzs  # one unit of t above the plane
    with _engine() as e:
        e.mesh_upload(*_soup(tri))
        ref = _check(e, tri, o, d)
        assert ref["any"].tolist() == [False, True, True]  # both outcomes occur, one ulp apart


# ---- prune adversaries --------------------------------------------------------------------------------------------------------------
def test_prune_adversaries():
    v, tri = synth.heightfield_mesh(33, 33, 0.5, 0.2, seed=6)
    # a long thin triangle spanning the whole mesh BEHIND (below) the small ones, and one above them
    ext = np.array([[-1.0, -1.0, -2.0], [17.0, 17.0, -2.0], [17.0, 16.5, -2.0], [-1.0, -1.0, 3.0], [17.0, 17.0, 3.0], [17.0, 16.5, 3.0]])
    v2 = np.concatenate([v, ext])
    tri2 = np.concatenate([tri, np.array([[len(v), len(v) + 1, len(v) + 2], [len(v) + 3, len(v) + 5, len(v) + 4]], np.int32)])
    corners = R.corners(v2, tri2)
    rng = np.random.default_rng(9)
    n = 600
    # the heightfield's diagonal, grazing the corners of many leaf boxes: lattice points along x = y, seen along the diagonal
    s = rng.integers(0, 33, n) * 0.5
    tg = np.stack([s, s, np.zeros(n)], -1)
    o = np.stack([np.full(n, -3.0), np.full(n, -3.0), rng.uniform(0.0, 1.0, n)], -1)
    d = tg - o
    d[:, 0] = d[:, 1]
    o2 = np.stack([rng.uniform(3, 13, n), rng.uniform(3, 13, n), np.full(n, 8.0)], -1)  # from above through the thin triangles
    d2 = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), np.full(n, -1.0)], -1)
    o3 = o2 * [1, 1, -1]                                                                   # from below: the long triangle first
    with _engine() as e:
        e.mesh_upload(v2, tri2)
        _check(e, corners, o, d)
        r2 = _check(e, corners, o2, d2)
        r3 = _check(e, corners, o3, d2 * [1, 1, -1])
        assert r2["n_hit"] == n and r3["n_hit"] == n
        big = len(tri2) - 2
        assert 0 < (r3["tri"] == big).sum() < n and 0 < (r2["tri"] == big + 1).sum() < n


# ---- the scan -----------------------------------------------------------------------------------------------------------------------
def _scene_with_wall():
    v, tri = synth.heightfield_mesh(21, 21, 0.5, 0.15, seed=3)
    wall = np.array([[6.0, 1.0, -1.0], [6.0, 9.0, -1.0], [6.0, 9.0, 4.0], [6.0, 1.0, 4.0]])
    v2 = np.concatenate([v, wall])
    n0 = len(v)
    tri2 = np.concatenate([tri, np.array([[n0, n0 + 1, n0 + 2], [n0, n0 + 2, n0 + 3]], np.int32)])
    return v2, tri2


def _poses():
    a, b, c = 0.3, -0.2, 0.5
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    P = np.tile(np.eye(4), (3, 1, 1))
    P[0, :3, 3] = [3.0, 5.0, 1.5]
    P[1, :3, 3] = [8.0, 4.0, 1.0]
    P[2, :3, :3] = Rz @ Ry @ Rx
    P[2, :3, 3] = [4.5, 6.5, 2.0]
    return P


def test_scan_matches_the_model_in_order():
    v, tri = _scene_with_wall()
    corners = R.corners(v, tri)
    P, dirs = _poses(), synth.lidar_directions(4, 16, -40.0, 10.0)
    M = max(np.abs(v).max(), np.abs(P[:, :3, 3]).max())
    with _engine() as e:
        e.mesh_upload(v, tri)
        e.upload(EST, v)  # the other slot: its cell size is adopted
        ref = R.scan(corners, P, dirs)
        got = e.mesh_scan(GT, P, dirs, fetch=True)
        pts = e.download(GT)
        assert 0 < ref["n_hit"] < ref["n_rays"] == 3 * 64 and e.size(GT) == ref["n_hit"]
        assert np.array_equal(_bits(pts), _bits(ref["points"]))
        assert got["n_hit"] == ref["n_hit"] and got["n_rays"] == ref["n_rays"] and got["n_backface"] == ref["n_backface"]
        assert np.array_equal(got["pose_hits"], ref["pose_hits"]) and np.array_equal(got["ray_id"], ref["ray_id"])
        assert (ref["pose_hits"] > 0).all()
        # the scanned slot indexes, answers a search and lies on its own mesh
        idx, d2 = e.nn1(GT, EST)
        assert len(d2) == ref["n_hit"] and np.isfinite(d2).all()
        pp = e.mesh_distance(GT, fetch=True)[1]
        print("scan against its own mesh: max d / (u M) =", float(np.sqrt(pp["d2"].max()) / (U * M)))
        assert (pp["d2"] < (19 * U * M) ** 2).all()  # 11 u E <= 19 u M
        # min_range / max_range exactly at a hit's range: a bound b with b / len == t of that hit
        k = len(ref["ray_id"]) // 2
        o, d = R.scan_rays(P, dirs)
        r0 = int(ref["ray_id"][k])
        ln = float(ref["len"][k])
        t0 = float(R.cast(corners, o[r0:r0 + 1], d[r0:r0 + 1])["t"][0])
        b = t0 * ln
        for c in (b, np.nextafter(b, 0.0), np.nextafter(b, INF)):
            if c / ln == t0:
                b = c
        assert b / ln == t0
        for kw in (dict(max_range=b), dict(min_range=b), dict(min_range=np.nextafter(b, INF)), dict(max_range=np.nextafter(b, 0.0))):
            rr = R.scan(corners, P, dirs, **kw)
            gg = e.mesh_scan(GT, P, dirs, fetch=True, **kw)
            assert gg["n_hit"] == rr["n_hit"] and np.array_equal(gg["ray_id"], rr["ray_id"]), kw
            assert np.array_equal(_bits(e.download(GT)), _bits(rr["points"])), kw
            if kw in (dict(max_range=b), dict(min_range=b)):
                assert r0 in rr["ray_id"]  # the bound includes the hit exactly at it


def test_scan_noise_and_zero_hits():
    from cloud_map_evaluation_amd.engine import MapEvalError

    v, tri = _scene_with_wall()
    corners = R.corners(v, tri)
    P, dirs = _poses(), synth.lidar_directions(4, 16, -40.0, 10.0)
    sigma = 0.02
    with _engine() as e:
        e.mesh_upload(v, tri)
        ref = R.scan(corners, P, dirs, noise_std=sigma, seed=11)
        got = e.mesh_scan(EST, P, dirs, noise_std=sigma, seed=11, fetch=True)
        a = e.download(EST)
        assert got["n_hit"] == ref["n_hit"] and np.array_equal(got["pose_hits"], ref["pose_hits"]) and np.array_equal(got["ray_id"], ref["ray_id"])
        # the tolerance of tests/test_gpu_perturb.py for the same Box-Muller generator: 1e-12 sigma plus the rounding of the coordinates
        assert (np.abs(a - ref["points"]) <= 1e-12 * sigma + 4 * np.spacing(np.abs(ref["points"]))).all()
        assert np.abs(a - ref["clean"]).max() > 0.1 * sigma
        e.mesh_scan(EST, P, dirs, noise_std=sigma, seed=11)
        assert np.array_equal(_bits(e.download(EST)), _bits(a))  # the same seed: the same bytes
        e.mesh_scan(EST, P, dirs, noise_std=sigma, seed=12)
        b = e.download(EST)
        assert b.shape == a.shape and not np.array_equal(b, a)
        # no hit at all: an empty slot, no fault
        z = e.mesh_scan(EST, P, dirs, min_range=500.0, fetch=True)
        assert z["n_hit"] == 0 and z["pose_hits"].tolist() == [0, 0, 0] and len(z["ray_id"]) == 0 and e.size(EST) == 0
        with pytest.raises(MapEvalError):
            e.mesh_scan_fetch(EST)
        # a pass over the empty slot is refused by name, nothing is indexed or launched over zero points
        with pytest.raises(MapEvalError, match=r"\[-3\] me_cloud_visibility: the slot's cloud is empty"):
            e.cloud_visibility(EST, P[:, :3, 3])
        with pytest.raises(MapEvalError, match=r"\[-3\] me_mesh_distance: the slot's cloud is empty"):
            e.mesh_distance(EST)
        e.upload(GT, v)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.nn1(EST, GT)
        assert e.mesh_scan(EST, P, dirs)["n_hit"] > 0 and e.size(EST) > 0  # and the slot is usable again
        e.upload(EST, v)
        with pytest.raises(MapEvalError, match="me_mesh_scan_fetch"):
            e.mesh_scan_fetch(EST)


# ---- visibility ---------------------------------------------------------------------------------------------------------------------
WALL_V = np.array([[0.0, -2.0, -2.0], [0.0, 2.0, -2.0], [0.0, 2.0, 2.0], [0.0, -2.0, 2.0]])
WALL_T = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def _grid_points():
    y, z = np.meshgrid(np.linspace(-1.5, 1.5, 13), np.linspace(-1.5, 1.5, 11), indexing="ij")
    side = np.stack([np.ones_like(y), y, z], -1).reshape(-1, 3)
    beyond = np.array([[1.0, 30.0, 0.0], [-1.0, -30.0, 0.5], [0.5, 0.0, 40.0]])  # past the wall's rim: seen from both sides
    return np.concatenate([side * [1.0, 1.0, 1.0], side * [-1.0, 1.0, 1.0], beyond])


def test_visibility_wall_counts_mask_and_model():
    pts = _grid_points()
    org = np.array([[-3.0, 0.0, 0.0], [3.0, 0.25, 0.0]])
    corners = R.corners(WALL_V, WALL_T)
    n_side = 13 * 11
    with _engine() as e:
        e.mesh_upload(WALL_V, WALL_T)
        e.upload(GT, pts)
        ref = R.visibility(corners, pts, org)
        tot, pp = e.cloud_visibility(GT, org, fetch=True)
        assert np.array_equal(pp["n_seen"], ref["n_seen"]) and np.array_equal(pp["first_seen"], ref["first_seen"])
        for k in ("n_points", "n_visible", "n_in_range", "n_tests"):
            assert tot[k] == ref[k], k
        # by construction: the +x half is seen from origin 1 only, the -x half from origin 0 only, the three beyond the rim from both
        assert pp["first_seen"][:n_side].tolist() == [1] * n_side and pp["first_seen"][n_side:2 * n_side].tolist() == [0] * n_side
        assert pp["n_seen"][2 * n_side:].tolist() == [2, 2, 2] and tot["n_visible"] == len(pts)
        fo, fp = e.cloud_visibility(GT, org, first_only=True, fetch=True)
        rf = R.visibility(corners, pts, org, first_only=True)
        assert np.array_equal(fp["first_seen"], pp["first_seen"]) and np.array_equal(fp["n_seen"], rf["n_seen"]) and fo["n_tests"] == rf["n_tests"]
        assert fp["n_seen"].max() == 1 and fo["n_tests"] < tot["n_tests"]
        # one origin, a range gate: the keep mask selects exactly the model's visible points, in order
        one = org[:1]
        rv = R.visibility(corners, pts, one, max_range=10.0, min_range=2.2)
        tv, pv = e.cloud_visibility(GT, one, max_range=10.0, min_range=2.2, fetch=True)
        assert np.array_equal(pv["n_seen"], rv["n_seen"]) and tv["n_in_range"] == rv["n_in_range"] and 0 < tv["n_visible"] < tv["n_in_range"] < len(pts)
        assert e.select_kept_into(GT, e, EST) == rv["n_visible"]
        assert np.array_equal(e.download(EST), pts[rv["n_seen"] > 0])


def test_visibility_tolerance_flips_at_one_ulp_behind_the_wall():
    corners = R.corners(WALL_V, WALL_T)
    org = np.array([[-4.0, 0.0, 0.0]])
    tol = 0.25
    # the segment's length 4 + x is what the rule sees: step it by ITS ulps around 4 + tol (x = len - 4 is exact)
    lens = [4.0 + tol]
    for _ in range(6):
        lens.append(np.nextafter(lens[-1], INF))
    lo = 4.0 + tol
    for _ in range(6):
        lo = np.nextafter(lo, 0.0)
        lens.append(lo)
    xs = np.array(sorted(lens)) - 4.0
    pts = np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], -1)  # straight behind the wall at x = 0, around `tol` behind it
    with _engine() as e:
        e.mesh_upload(WALL_V, WALL_T)
        e.upload(GT, pts)
        ref = R.visibility(corners, pts, org, tolerance=tol)
        _, pp = e.cloud_visibility(GT, org, tolerance=tol, fetch=True)
        assert np.array_equal(pp["n_seen"], ref["n_seen"])
        s = ref["n_seen"]
        # one transition, exactly at the tolerance: seen up to one ulp (of the length) short of `tol` behind the wall, hidden from `tol` on
        assert s.tolist() == [1] * 6 + [0] * 7 and xs[6] == tol


def test_visibility_of_samples_on_a_flat_mesh():
    v, tri = synth.heightfield_mesh(12, 9, 0.5, 0.0, seed=1)
    corners = R.corners(v, tri)
    org = np.array([[2.0, 1.5, 6.0], [4.0, 3.0, 9.0]])
    with _engine() as e:
        e.mesh_upload(v, tri)
        e.mesh_sample(GT, 600, seed=5)
        pts = e.download(GT)
        # A sample lies on the surface: its segment ends there with t = 1 (to rounding), and the interval [0, (len - tol) / len] ends at 1
        # for tol = 0 — the point's own triangle is inside the interval, so tol = 0 is ill-posed for exact-surface points.  The smallest
        # tolerance for which the MODEL reports every sample visible is searched on the host; the device must equal the model there
        # and at tol = 0.
        r0 = R.visibility(corners, pts, org)
        _, p0 = e.cloud_visibility(GT, org, fetch=True)
        assert np.array_equal(p0["n_seen"], r0["n_seen"]) and np.array_equal(p0["first_seen"], r0["first_seen"])
        tol = None
        for k in range(52, 20, -1):
            if R.visibility(corners, pts, org, tolerance=2.0 ** -k)["n_visible"] == len(pts):
                tol = 2.0 ** -k
                break
        assert tol is not None and tol <= 2.0 ** -40
        rt = R.visibility(corners, pts, org, tolerance=tol)
        tt, pt = e.cloud_visibility(GT, org, tolerance=tol, fetch=True)
        assert np.array_equal(pt["n_seen"], rt["n_seen"]) and np.array_equal(pt["first_seen"], rt["first_seen"])
        assert tt["n_visible"] == len(pts) and (pt["n_seen"] >= 1).all()  # every sample is seen from some origin


def test_observable_report_two_rooms():
    # two closed rooms side by side; the origins stand in the first: the second room's walls are never seen
    def room(x0):
        cv, ct = _cube()
        return cv * [4.0, 4.0, 3.0] + [x0, 0.0, 0.0], ct

    v1, t1 = room(0.0)
    v2, t2 = room(4.5)
    v, tri = np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)])
    org = np.array([[2.0, 2.0, 1.5], [1.0, 3.0, 1.0]])
    with _engine() as e:
        e.mesh_upload(v1, t1)
        e.mesh_sample(GT, 6000, seed=1)
        a = e.download(GT)
        e.mesh_upload(v2, t2)
        e.mesh_sample(GT, 4000, seed=2)
        b = e.download(GT)
        gt = np.concatenate([a, b])
        est = a[::2] + np.random.default_rng(3).normal(0, 0.005, (len(a[::2]), 3))  # the map covers the first room only
        e.mesh_upload(v, tri)
        e.upload(EST, est)
        e.upload(GT, gt)
        rep = e.observable_report(org, [0.05, 0.5], tolerance=0.01)
        assert rep["visible_share"] == 6000 / 10000 and rep["visibility"]["n_visible"] == 6000
        assert rep["observable"]["gt"]["n_query"] == 6000 and rep["all"]["gt"]["n_query"] == 10000
        assert (rep["observable"]["recall"] >= rep["all"]["recall"]).all() and rep["observable"]["recall"][1] > 0.99 > rep["all"]["recall"][1]
        assert e.size(GT) == 10000 and e.size(EST) == len(est) and np.array_equal(e.download(GT), gt)  # the slots are left as found


# ---- state and arguments ------------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
    from cloud_map_evaluation_amd.engine import MapEvalError

    pts = _grid_points()
    org = np.array([[-3.0, 0.0, 0.0]])
    o, d = np.zeros((2, 3)), np.tile([1.0, 0.0, 0.0], (2, 1))
    P, dirs = _poses(), synth.lidar_directions(2, 4, -10.0, 10.0)
    with _engine() as e:
        for call in (lambda: e.mesh_raycast(o, d), lambda: e.mesh_scan(GT, P, dirs)):
            with pytest.raises(MapEvalError, match=r"\[-3\].*no mesh"):
                call()
        e.upload(GT, pts)
        with pytest.raises(MapEvalError, match=r"\[-3\].*me_cloud_visibility: no mesh"):
            e.cloud_visibility(GT, org)
        e.mesh_upload(WALL_V, WALL_T)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.cloud_visibility(EST, org)  # no cloud in the slot
        with pytest.raises(MapEvalError, match=r"\[-3\].*me_cloud_visibility_fetch"):
            e.visibility_fetch(GT)
        # the twin sees the mesh and the clouds
        tw = e.twin()
        assert tw.mesh_raycast(np.array([[-3.0, 0.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))["t"][0] == 3.0
        # dropped by a re-upload, a re-index (a new cell size through me_mme) and mesh_clear / mesh_upload
        e.cloud_visibility(GT, org)
        e.visibility_fetch(GT)
        e.upload(GT, pts)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.visibility_fetch(GT)
        e.cloud_visibility(GT, org)
        e.mme(GT, 0.7, 3, per_point=False)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.visibility_fetch(GT)
        e.cloud_visibility(GT, org)
        e.mesh_upload(WALL_V, WALL_T)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.visibility_fetch(GT)
        # mesh_distance results of the slot survive a visibility call, and the reverse
        md = e.mesh_distance(GT, fetch=True)[1]
        vis = e.cloud_visibility(GT, org, fetch=True)[1]
        md2 = e.mesh_distance_fetch(GT)
        assert all(np.array_equal(md[k], md2[k], equal_nan=True) for k in md)
        e.mesh_distance(GT)
        vis2 = e.visibility_fetch(GT)
        assert all(np.array_equal(vis[k], vis2[k]) for k in vis)
        e.mesh_clear()
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.visibility_fetch(GT)
        e.mesh_upload(WALL_V, WALL_T)
        # argument errors are named
        for kw, name in ((dict(t_min=-1.0), "t_min"), (dict(t_min=2.0, t_max=1.0), "t_max"), (dict(t_max=math.nan), "t_max"),
                         (dict(t_min=INF), "t_min")):
            with pytest.raises(MapEvalError, match=r"\[-1\] me_mesh_raycast: " + name):
                e.mesh_raycast(o, d, **kw)
        for kw, name in ((dict(min_range=-1.0), "min_range"), (dict(min_range=5.0, max_range=1.0), "max_range"),
                         (dict(noise_std=-0.1), "noise_std"), (dict(noise_std=INF), "noise_std")):
            with pytest.raises(MapEvalError, match=r"\[-1\] me_mesh_scan: " + name):
                e.mesh_scan(EST, P, dirs, **kw)
        with pytest.raises(MapEvalError, match=r"\[-1\] me_mesh_scan: bad slot"):
            e.mesh_scan(2, P, dirs)
        for kw, name in ((dict(min_range=-1.0), "min_range"), (dict(min_range=5.0, max_range=1.0), "max_range"),
                         (dict(tolerance=-0.1), "tolerance"), (dict(tolerance=math.nan), "tolerance")):
            with pytest.raises(MapEvalError, match=r"\[-1\] me_cloud_visibility: " + name):
                e.cloud_visibility(GT, org, **kw)
        with pytest.raises(MapEvalError, match=r"\[-1\] me_cloud_visibility: needs 1 <= n_origins <= 65536"):
            e.cloud_visibility(GT, np.zeros((65537, 3)))
        with pytest.raises(MapEvalError, match=r"\[-1\] me_cloud_visibility: bad slot"):
            e.cloud_visibility(3, org)
