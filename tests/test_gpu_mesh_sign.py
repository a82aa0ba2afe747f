"""me_mesh_topology / me_mesh_signed_distance on the MI355X against the numpy model of tests/_mesh_sign_ref.py and against the
generalized winding number: topology counts, flags and edge normals EQUAL, vertex normals within the atan2 allowance, signed_d bitwise
equal outside the rounding band of g, totals within 1e-9 of the exact sums of the device's own values, two calls byte-identical, the
state and argument rules, the lifetimes, and a reconstructed sphere.

The band: the device's N_v differs from numpy's by the 1-2 ulp of atan2, so g = dot(p - c, N) may change sign where it is within
2^-40 sqrt(d2) |N| of zero; such points are excluded from the bitwise comparison and their share is capped at 0.1 %."""
import math
import re

import numpy as np
import pytest

import _lifetime as L
import _mesh_ref as R
import _mesh_sign_ref as S
from test_mesh_sign_cpu import CLOSED, case_queries, check_against_winding, cube_diagonals, l_prism_constructed

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a) and a.keys() == b.keys()


def _check_topology(cnt, tf, v, t):
    m = S.topology(v, t)
    assert cnt == m["counts"], (cnt, m["counts"])
    assert np.array_equal(tf["edge_flags"], m["edge_flags"]) and np.array_equal(tf["vertex_flags"], m["vertex_flags"])
    assert tf["edge_normal"].tobytes() == (m["edge_normal"] + 0.0).tobytes(), "edge normals: sqrt, division and ordered sums only"
    bound = ((m["valence"] + 8) * U * m["vertex_sum_ang"])[:, None]
    assert (np.abs(tf["vertex_normal"] - m["vertex_normal"]) <= bound).all()
    return m


def _check_sign(tot, sp, pp, pts, v, t, topo, max_distance=math.inf):
    m = S.signed(pts, v, t, pp, topo)
    # (a point on the mesh, a ZERO feature and a degenerate winner are decided before g is looked at: never in the band)
    band = ~(np.abs(m["g"]) > 2.0 ** -40 * np.sqrt(pp["d2"]) * np.linalg.norm(m["N"], axis=1)) & (pp["d2"] > 0) & ~m["structural"]
    assert band.mean() <= 1e-3, f"{band.sum()} of {len(pts)} points in the rounding band"
    ok = ~band
    assert np.array_equal(sp["signed_d"][ok], m["signed_d"][ok], equal_nan=True)
    assert (np.signbit(sp["signed_d"][ok]) == np.signbit(m["signed_d"][ok])).all()
    assert np.array_equal(sp["flags"][ok], m["flags"][ok])
    assert np.array_equal(np.abs(sp["signed_d"][~np.isnan(sp["signed_d"])]), np.sqrt(pp["d2"])[~np.isnan(sp["signed_d"])])
    want = S.totals(pp["d2"], pp["region"], sp["signed_d"], sp["flags"], max_distance)  # exact sums of the DEVICE's values
    for k in ("n_query", "n_matched", "n_signed", "n_inside", "n_outside", "n_on", "n_unsigned", "n_unreliable", "argmin", "argmax",
              "min_signed", "max_signed"):
        assert tot[k] == want[k], (k, tot[k], want[k])
    assert list(tot["n_by_region"]) == want["n_by_region"]
    for k in ("sum_signed", "sum_abs_signed", "sum_signed2"):
        assert abs(tot[k] - want[k]) <= 1e-9 * (want["sum_abs_signed"] if k == "sum_signed" else abs(want[k])), k
    ns, nm = want["n_signed"], want["n_matched"]
    assert tot["mean_signed"] == (tot["sum_signed"] / ns if ns else 0.0) and tot["mean_abs"] == (tot["sum_abs_signed"] / ns if ns else 0.0)
    assert tot["inside_share"] == (want["n_inside"] / ns if ns else 0.0) and tot["unreliable_share"] == (want["n_unreliable"] / nm if nm else 0.0)
    return m


def _run(pts, v, t, max_distance=math.inf):
    pts = np.ascontiguousarray(pts, np.float64)
    with _engine() as e:
        e.upload(0, pts)
        e.mesh_upload(v, t)
        _, pp = e.mesh_distance(0, fetch=True)
        cnt, tf = e.mesh_topology(fetch=True)
        tot, sp = e.mesh_signed_distance(0, max_distance, fetch=True)
        tot2, sp2 = e.mesh_signed_distance(0, max_distance, fetch=True)  # two calls: identical bytes
        cnt2, tf2 = e.mesh_topology(fetch=True)
        assert _same(tot, tot2) and _same(sp, sp2) and cnt == cnt2 and _same(tf, tf2)
        assert _same(pp, e.mesh_distance_fetch(0)), "the sign pass changed me_mesh_distance's own result"
    topo = _check_topology(cnt, tf, v, t)
    return tot, sp, pp, cnt, _check_sign(tot, sp, pp, pts, v, t, topo, max_distance)


def _on_features(v, t):
    """points exactly on the vertices and on the edge midpoints that fp64 represents exactly on the segment"""
    a = np.asarray(v)[np.asarray(t)]
    return np.vstack([np.asarray(v)[np.unique(t)], ((a[:, 0] + a[:, 1]) / 2.0)])


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_meshes_against_the_model_and_the_winding_number(name):
    v, t, q = case_queries(name)
    tot, sp, pp, cnt, m = _run(q, v, t)
    assert cnt["closed"] and cnt["oriented_manifold"] and tot["n_unreliable"] == 0
    bad = check_against_winding(v, t, q, sp["signed_d"], pp["d2"])
    assert len(bad) == 0, (q[bad[:5]], sp["signed_d"][bad[:5]], pp["region"][bad[:5]])
    assert tot["n_by_region"][1] > 0 and tot["n_by_region"][2] > 0 and tot["n_inside"] > 0 and tot["n_outside"] > 0


def test_cube_on_its_vertices_and_edge_midpoints():
    v, t = S.cube()
    q = np.vstack([_on_features(v, t), cube_diagonals()])
    n_on = len(_on_features(v, t))
    tot, sp, pp, cnt, _ = _run(q, v, t)
    assert (pp["d2"][:n_on] == 0).all() and (sp["flags"][:n_on] == S.ON).all()
    assert (sp["signed_d"][:n_on] == 0).all() and not np.signbit(sp["signed_d"][:n_on]).any()
    assert tot["n_on"] == n_on and (sp["signed_d"][n_on:] > 0).all() and (pp["region"][n_on:] != 0).all()


def test_l_prism_where_face_normals_disagree():
    """inside the L on the planes of the two faces that meet in the re-entrant edge: the two face normals give g = 0 and g < 0; the
    pseudo-normal names the inside, as the winding number does"""
    v, t = S.l_prism()
    q = l_prism_constructed()
    tot, sp, pp, cnt, m = _run(q, v, t)
    n = S.faces(v, t)[0]
    topo = S.topology(v, t)
    shown = 0
    for i in np.flatnonzero((pp["region"] >= 1) & (pp["region"] <= 3)):
        eid = topo["eid"][pp["tri"][i], pp["region"][i] - 1]
        g = [float(np.dot(q[i] - pp["closest"][i], n[k])) for k in np.flatnonzero((topo["eid"] == eid).any(axis=1))]
        assert len(g) == 2
        if np.sign(g[0]) != np.sign(g[1]):
            shown += 1
            assert sp["signed_d"][i] < 0 and S.winding(q[i:i + 1], v, t)[0] > 0.5
    assert shown >= 1
    assert (sp["signed_d"] < 0).all() and len(check_against_winding(v, t, q, sp["signed_d"], pp["d2"])) == 0


OPEN = {
    "one_triangle": lambda: (np.array([[0.0, 0, 0], [4, 0, 0], [0, 4, 0]]), np.array([[0, 1, 2]], np.int32)),
    "inconsistent_pair": S.inconsistent_pair,
    "fin_of_5": S.fin,
    "fan_of_70": lambda: S.fan(70),
    "duplicated_triangle": lambda: (S.cube()[0], np.vstack([S.cube()[1], S.cube()[1][3:4]]).astype(np.int32)),
    "unreferenced_vertices": lambda: (np.vstack([[[7.0, 7, 7]], S.cube()[0], [[9.0, 9, 9]]]), (S.cube()[1] + 1).astype(np.int32)),
    "vertex_named_twice": lambda: (S.cube()[0], np.vstack([S.cube()[1], [[0, 0, 5]]]).astype(np.int32)),
}


@pytest.mark.parametrize("name", sorted(OPEN))
def test_open_and_broken_meshes_against_the_model(name):
    v, t = OPEN[name]()
    q = np.vstack([S.queries(v, t, 300, seed=len(name)), _on_features(v, t)])
    tot, sp, pp, cnt, m = _run(q, v, t)
    if name == "one_triangle":
        assert cnt["n_boundary_edges"] == 3 and not cnt["closed"]
        off_face = pp["region"] != 0
        assert ((sp["flags"][off_face] & S.UNRELIABLE) != 0).all() and ((sp["flags"][~off_face] & S.UNRELIABLE) == 0).all()
    if name == "fan_of_70":
        assert cnt["n_edges"] == 140 and (pp["region"] >= 4).any()
    if name == "fin_of_5":
        assert cnt["n_nonmanifold_edges"] == 1
    if name == "inconsistent_pair":
        assert cnt["n_inconsistent_edges"] == 1 and not cnt["oriented_manifold"]
    if name == "duplicated_triangle":
        assert cnt["n_nonmanifold_edges"] == 3 and tot["n_unreliable"] > 0
    if name == "unreferenced_vertices":
        assert cnt["n_unreferenced_vertices"] == 2 and cnt["n_zero_vertices"] == 2 and cnt["closed"]
    if name == "vertex_named_twice":
        assert cnt["n_edges"] == 18 and cnt["closed"]


@pytest.mark.parametrize("nt", [1, 8, 9, 4097])
def test_triangle_counts_and_cloud_sizes(nt):
    """the first nt triangles of a subdivided octahedron (closed at 8, cut open at 1, 9 and 4097) against 1 ... 4097 queries"""
    v, t = S.surface_prefix(nt)
    assert len(t) == nt
    for nq in ((1, 63, 64, 65, 4097) if nt < 4097 else (257, 4097)):
        q = S.queries(v, t, nq, seed=nt + nq)
        tot, sp, pp, cnt, _ = _run(q, v, t, max_distance=0.75)
        assert tot["n_query"] == nq and cnt["closed"] == (nt == 8)
        if nt == 8:
            assert cnt["oriented_manifold"] and cnt["n_edges"] == 12
            assert len(check_against_winding(v, t, q, sp["signed_d"], pp["d2"])) == 0


def test_state_and_argument_errors():
    from cloud_map_evaluation_amd.engine import MapEvalError

    v, t = S.cube()
    with _engine() as e:
        e.upload(0, S.queries(v, t, 50, 1))
        for call in (lambda: e.mesh_topology(), lambda: e.mesh_signed_distance(0)):
            with pytest.raises(MapEvalError, match=r"\[-3\]"):  # no mesh
                call()
        e.mesh_upload(v, t)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):  # no mesh-distance result
            e.mesh_signed_distance(0)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.mesh_signed_distance(1)  # no cloud
        e.mesh_distance(0)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.mesh_signed_fetch(0)  # not run yet
        for bad in (-1.0, math.nan):
            with pytest.raises(MapEvalError, match=r"\[-1\]"):
                e.mesh_signed_distance(0, bad)
        for slot in (-1, 2):
            with pytest.raises(MapEvalError, match=r"\[-1\]"):
                e.mesh_signed_distance(slot)
        gated = e.mesh_signed_distance(0, 0.0)
        assert gated["n_matched"] == 0 and gated["argmin"] == -1 and gated["argmax"] == -1 and gated["sum_abs_signed"] == 0.0
        assert e.mesh_signed_distance(0)["n_matched"] == 50


def test_lifetimes_follow_the_mesh_distance_result():
    """per disturber of tests/_lifetime.py and side: the signed result is gone exactly where the table drops (or rewrites) the
    mesh-distance result, and keeps its bytes elsewhere; a new mesh_distance and reconstruct_install drop it"""
    from cloud_map_evaluation_amd.engine import MapEvalError

    def state(e):
        try:
            return e.mesh_signed_fetch(0), None
        except MapEvalError as ex:
            return None, str(ex)

    bad = []
    for dname, D in L.DISTURBERS.items():
        for side in L.SIDES:
            want = L.EXPECT[("mesh_distance", dname, side)][0]
            with _engine() as e:
                L.base(e)
                e.mesh_distance(0)
                e.mesh_signed_distance(0)
                before, _ = state(e)
                md = e.mesh_distance_fetch(0)
                D["act"](e, 0 if side == "own" else 1)
                after, err = state(e)
                if want == L.KEEP:
                    if after is None or not _same(before, after) or not _same(md, e.mesh_distance_fetch(0)):
                        bad.append((dname, side, want, err))
                elif after is not None or not re.search(r"\[-3\]", err):
                    bad.append((dname, side, want, err))
    assert not bad, bad
    with _engine() as e:
        L.base(e)
        e.mesh_distance(0)
        e.mesh_signed_distance(0)
        e.mesh_distance(1)  # the other slot's own result: nothing happens to this one
        e.mesh_signed_distance(1)
        assert state(e)[0] is not None
        e.mesh_distance(0)  # a new mesh distance on the slot
        assert state(e)[0] is None and re.search(r"\[-3\]", state(e)[1])
        assert e.mesh_signed_fetch(1) is not None
        e.mesh_signed_distance(0)
        e.reconstruct(1, 0.1, radius=L.R_FAR, min_k=4, band=0, fetch=False)
        e.reconstruct_install()
        assert state(e)[0] is None and re.search(r"\[-3\]", state(e)[1])


def test_reconstructed_sphere_has_the_analytic_sign():
    rng = np.random.default_rng(3)
    n = rng.normal(size=(6000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    radius, voxel = 1.0, 0.1
    q = rng.uniform(-1.6, 1.6, size=(3000, 3))
    with _engine() as e:
        e.upload(0, q)
        e.upload(1, radius * n)
        e.set_normals(1, n)  # outward
        rec = e.reconstruct(1, voxel, install=True, fetch=False)
        cnt = e.mesh_topology()
        e.mesh_distance(0)
        tot, sp = e.mesh_signed_distance(0, fetch=True)
    print("reconstructed sphere:", {k: rec[k] for k in rec if np.isscalar(rec[k])}, cnt, {k: tot[k] for k in tot if k.startswith("n_")})
    r = np.linalg.norm(q, axis=1)
    far = np.abs(r - radius) > 2 * voxel
    assert far.sum() > 1000
    with np.errstate(invalid="ignore"):
        ok = np.where(r < radius, sp["signed_d"] < 0, sp["signed_d"] > 0)
    assert ok[far].all(), (np.flatnonzero(far & ~ok)[:5], cnt)


def test_mesh_report_signed_block():
    v, t = S.torus()
    q = S.queries(v, t, 500, seed=11, inflate=0.2)
    with _engine() as e:
        e.upload(0, q)
        e.mesh_upload(v, t)
        plain = e.mesh_report([0.1, 0.3])
        rep = e.mesh_report([0.1, 0.3], signed=True)
        tot, sp = e.mesh_signed_distance(0, fetch=True)
    assert "signed" not in plain and all(np.asarray(plain[k]).tobytes() == np.asarray(rep[k]).tobytes() for k in plain)
    sg = rep["signed"]
    assert all(np.asarray(sg[k]).tobytes() == np.asarray(tot[k]).tobytes() for k in tot)
    assert sg["topology"]["closed"] and sg["topology"]["oriented_manifold"]
    s = np.sort(sp["signed_d"][~np.isnan(sp["signed_d"])])
    assert (s < 0).any() and (s > 0).any()
    assert np.array_equal(sg["quantile_signed"], s[sg["rank"]]), "exact nearest-rank quantiles over the signed points"
