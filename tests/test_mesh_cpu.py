"""The brute-force cloud-to-mesh model (tests/_mesh_ref.py) pinned on statements it did not write: a barycentric lattice of the
triangle, the barycentric coordinates of its own closest point, hand cases; the sampler model's geometry and frequencies; and the
surface: the new entry points are declared, exported and bound.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import _mesh_ref as R
from cloud_map_evaluation_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lattice_min(p, a, b, g, m=200):
    """the smallest distance from p to the points a + (i/m)(b-a) + (j/m)(g-a), i + j <= m"""
    i, j = np.meshgrid(np.arange(m + 1), np.arange(m + 1), indexing="ij")
    keep = i + j <= m
    s, t = i[keep] / m, j[keep] / m
    q = a + s[:, None] * (b - a) + t[:, None] * (g - a)
    return np.sqrt(((q - p) ** 2).sum(1).min())


def test_model_against_a_barycentric_lattice():
    rng = np.random.default_rng(7)
    for _ in range(60):
        a, b, g = rng.normal(size=(3, 3))
        p = rng.normal(size=3) * 1.5
        d2, c, r = R.closest(p, a, b, g)
        d = np.sqrt(d2)
        spacing = max(np.linalg.norm(b - a), np.linalg.norm(g - a), np.linalg.norm(g - b)) / 200
        lat = _lattice_min(p, a, b, g)
        assert d <= lat * (1 + 1e-12) and d >= lat - spacing
        # the region code against the barycentric coordinates of the closest point
        M = np.stack([b - a, g - a], 1)
        (s, t), *_ = np.linalg.lstsq(M, c - a, rcond=None)
        w = np.array([1 - s - t, s, t])
        zero = np.abs(w) < 1e-9
        expect = {(False, False, False): R.FACE, (False, False, True): R.EDGE_AB, (True, False, False): R.EDGE_BC,
                  (False, True, False): R.EDGE_CA, (False, True, True): R.VERT_A, (True, False, True): R.VERT_B,
                  (True, True, False): R.VERT_C}[tuple(zero)]
        assert int(r) == expect and (w > -1e-9).all()


def test_model_is_exact_on_hand_cases():
    a, b, g = np.array([0.0, 0, 0]), np.array([4.0, 0, 0]), np.array([0.0, 4, 0])
    cases = [((1, 1, 3), 9.0, R.FACE, (1, 1, 0)), ((1, 1, 0), 0.0, R.FACE, (1, 1, 0)),          # above the interior, on the plane
             ((2, -3, 0), 9.0, R.EDGE_AB, (2, 0, 0)), ((-3, 2, 4), 25.0, R.EDGE_CA, (0, 2, 0)),  # beyond each edge
             ((3, 3, 0), 2.0, R.EDGE_BC, (2, 2, 0)),
             ((-3, -4, 0), 25.0, R.VERT_A, (0, 0, 0)), ((7, -4, 0), 25.0, R.VERT_B, (4, 0, 0)),  # beyond each vertex
             ((-3, 8, 0), 25.0, R.VERT_C, (0, 4, 0)),
             ((2, 0, 0), 0.0, R.EDGE_AB, (2, 0, 0)), ((4, 0, 0), 0.0, R.VERT_B, (4, 0, 0)),      # on an edge, on a vertex
             ((0, 0, 0), 0.0, R.VERT_A, (0, 0, 0)), ((0, 4, 0), 0.0, R.VERT_C, (0, 4, 0))]
    for p, d2, region, c in cases:
        gd2, gc, gr = R.closest(np.array(p, np.float64), a, b, g)
        assert (float(gd2), int(gr), tuple(gc)) == (d2, region, tuple(float(x) for x in c)), p


def test_model_degenerate_triangles_are_their_segments_and_ties_take_the_lower_index():
    v = np.array([[0.0, 0, 0], [2, 0, 0], [4, 0, 0], [0, 2, 0]])
    tri = np.array([[0, 1, 2], [0, 0, 3], [0, 1, 3], [0, 1, 3]], np.int32)  # collinear, repeated index, and a duplicated proper one
    area, deg = R.areas(v, tri)
    assert deg.tolist() == [True, True, False, False] and area.tolist() == [0.0, 0.0, 2.0, 2.0]
    res = R.distance(np.array([[3.0, 1, 0], [-1, 1, 0], [0.5, 0.5, 1], [5, 0, 0]]), v, tri)
    assert res["d2"].tolist() == [1.0, 1.0, 1.0, 1.0]
    assert res["tri"].tolist() == [0, 1, 2, 0]  # (the duplicate 3 never wins against 2)
    assert res["region"].tolist() == [R.EDGE_BC, R.EDGE_BC, R.FACE, R.VERT_C]
    assert np.isnan(res["signed_d"][[0, 1, 3]]).all() and res["signed_d"][2] == 1.0
    t = R.totals(res, 1.0, [0.5, 1.0])
    assert (t["n_matched"], t["n_face"], t["sum_d"], t["worst_index"], t["n_within"].tolist()) == (4, 1, 4.0, 0, [0, 4])


def _mixed_mesh(seed=3):
    """50 triangles whose areas are exactly spread over 1 ... 100 (each scaled about its first corner to its target), plus two of area
    zero: a repeated vertex index and three collinear corners"""
    rng = np.random.default_rng(seed)
    tv = rng.normal(size=(52, 3, 3))
    target = np.ones(52)
    proper = np.array([k for k in range(52) if k not in (10, 40)])
    target[proper] = np.geomspace(1.0, 100.0, 50)
    area = 0.5 * np.linalg.norm(np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]), axis=1)
    tv = tv[:, :1] + (tv - tv[:, :1]) * np.sqrt(target / area)[:, None, None]
    v = (tv + rng.normal(size=(52, 1, 3)) * 5).reshape(-1, 3)
    tri = np.arange(156, dtype=np.int32).reshape(52, 3)
    tri[10] = [30, 30, 31]
    v[3 * 40:3 * 40 + 3] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
    return v, tri


def test_sampler_model():
    v, tri = _mixed_mesh()
    area, deg = R.areas(v, tri)
    assert deg.sum() == 2 and (~deg).sum() == 50 and area.max() / area[~deg].min() == pytest.approx(100.0, rel=1e-9)
    n = 100_000
    pts, t = R.sample(v, tri, n, seed=11)
    assert not deg[t].any()                                   # zero-area triangles are never drawn
    a, b, g = v[tri[t, 0]], v[tri[t, 1]], v[tri[t, 2]]
    nrm = R.cross(b - a, g - a)
    assert (np.abs(((pts - a) * nrm).sum(1)) / np.linalg.norm(nrm, axis=1) <= 1e-12).all()  # in the plane, to 1e-12
    # inside: barycentric coordinates >= -1e-12
    M = np.stack([b - a, g - a], 2)
    st = np.einsum("nij,nj->ni", np.linalg.pinv(M), pts - a)
    w = np.concatenate([1 - st.sum(1, keepdims=True), st], 1)
    assert (w >= -1e-12).all() and (w <= 1 + 1e-12).all()
    pr = area / area.sum()
    cnt = np.bincount(t, minlength=len(tri))
    sigma = np.sqrt(n * pr * (1 - pr))
    assert (np.abs(cnt - n * pr)[~deg] <= 5 * sigma[~deg]).all()
    again, t2 = R.sample(v, tri, n, seed=11)
    assert np.array_equal(pts, again) and not np.array_equal(pts, R.sample(v, tri, n, seed=12)[0])


def test_heightfield_mesh():
    v, tri = synth.heightfield_mesh(5, 4, 0.5, 0.2, seed=1)
    assert v.shape == (20, 3) and tri.shape == (2 * 4 * 3, 3) and tri.dtype == np.int32
    assert np.abs(v[:, 2]).max() <= 0.2 and v[:, 0].max() == 2.0 and v[:, 1].max() == 1.5
    area, deg = R.areas(v, tri)
    assert not deg.any() and (R.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])[:, 2] > 0).all()  # normals towards +z
    assert set(tri.reshape(-1).tolist()) == set(range(20))


def test_mesh_symbols_are_declared_exported_and_bound():
    names = ["me_mesh_upload", "me_mesh_clear", "me_mesh_info", "me_mesh_distance", "me_mesh_distance_fetch", "me_mesh_sample"]
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mapeval_hip.h")).read()
    for s in names:
        assert s in _lib.SYMBOLS and hasattr(L, s) and f"int {s}(" in hdr
        assert getattr(L, s).argtypes is not None and getattr(L, s).restype is C.c_int
    # int64 / double members only
    assert C.sizeof(_lib.MeshParams) == 8 * (2 + 8)
    assert C.sizeof(_lib.MeshOut) == 8 * (3 + 3 + 1 + 8 + 2)
    assert C.sizeof(_lib.MeshInfoOut) == 8 * (4 + 3 + 3 + 1)
    from cloud_map_evaluation_amd.engine import Engine

    for m in ("mesh_upload", "mesh_info", "mesh_clear", "mesh_distance", "mesh_distance_fetch", "mesh_sample", "mesh_report"):
        assert callable(getattr(Engine, m))
