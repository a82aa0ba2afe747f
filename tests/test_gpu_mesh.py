"""me_mesh_upload / me_mesh_distance / me_mesh_sample on the MI355X against the brute-force model of tests/_mesh_ref.py: d2, triangle,
region and closest point EQUAL on every point (the model restates the device's arithmetic), counts equal, sums within 1e-9 of the
exact sum of the device's own values, two calls byte-identical; the tree's level edges, ties across shared edges near the origin and
at survey coordinates, duplicates, degenerate triangles, far queries, the gate at one ulp, the state rules, the sampler bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import _mesh_ref as R
from cloud_map_evaluation_amd import _lib, synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _check(tot, pp, pts, v, tri, max_distance=math.inf, thresholds=(), model=None):
    m = R.distance(pts, v, tri) if model is None else model
    for k in ("d2", "tri", "region", "closest"):
        assert np.array_equal(pp[k], m[k]), k
    assert np.array_equal(np.isnan(pp["signed_d"]), pp["region"] != R.FACE)
    assert np.array_equal(pp["signed_d"], m["signed_d"], equal_nan=True)
    t = R.totals(pp, max_distance, thresholds)  # the exact sums of the DEVICE's per-point values
    for k in ("n_query", "n_matched", "n_face", "worst_index", "max"):
        assert tot[k] == t[k], k
    assert np.array_equal(tot["n_within"], t["n_within"])
    for k in ("sum_d", "sum_d2", "sum_signed", "sum_abs_signed"):  # (a signed sum may cancel: its scale is the sum of the magnitudes)
        assert abs(tot[k] - t[k]) <= 1e-9 * (t["sum_abs_signed"] if k == "sum_signed" else abs(t[k])), k
    return m


def _run(pts, v, tri, max_distance=math.inf, thresholds=(), model=None, T=None):
    with _engine() as e:
        e.upload(0, pts)
        e.mesh_upload(v, tri, T)
        tot, pp = e.mesh_distance(0, max_distance, thresholds, fetch=True)
        tot2, pp2 = e.mesh_distance(0, max_distance, thresholds, fetch=True)  # two calls: identical bytes
        assert all(np.asarray(tot[k]).tobytes() == np.asarray(tot2[k]).tobytes() for k in tot)
        assert all(pp[k].tobytes() == pp2[k].tobytes() for k in pp)
        info = e.mesh_info()
    return tot, pp, info, _check(tot, pp, pts, v, tri, max_distance, thresholds, model)


def test_one_triangle_all_seven_regions():
    v = np.array([[0.0, 0, 0], [4, 0, 0], [0, 4, 0]])
    tri = np.array([[0, 1, 2]], np.int32)
    rng = np.random.default_rng(1)
    pts = np.concatenate([rng.uniform(-6, 10, (52, 3)),
                          [[1, 1, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0], [0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, 3], [1, 2, -0.5], [2, -3, 0],
                           [7, -4, 0], [-3, 8, 0]]])
    assert len(pts) == 64
    tot, pp, info, m = _run(pts, v, tri, thresholds=[0.0, 1.0, 3.0])
    assert set(pp["region"].tolist()) == set(range(7)) and (pp["d2"][52:59] == 0.0).all()
    assert (info["triangles"], info["degenerate"], info["depth"], info["area"]) == (1, 0, 1, 8.0)
    assert pp["signed_d"][59] == 3.0 and pp["signed_d"][60] == -0.5 and tot["n_within"][0] == 7


@pytest.mark.parametrize("nt", [1, 7, 8, 9, 64, 65, 512, 513])
def test_tree_level_edges_and_query_counts(nt):
    """strips of a heightfield with 1 ... 513 triangles (the levels of the 8-ary tree fill and spill) against 1 ... 4097 queries"""
    v, tri = synth.heightfield_mesh(nt // 2 + 2, 2, 0.25, 0.2, seed=nt)
    tri = np.ascontiguousarray(tri[:nt])
    depth = 1 + sum(1 for k in (8, 64, 512) if nt > k)
    rng = np.random.default_rng(nt)
    for nq in (1, 63, 64, 65, 4097):
        pts = np.stack([rng.uniform(-0.5, v[:, 0].max() + 0.5, nq), rng.uniform(-0.5, 0.75, nq), rng.uniform(-0.6, 0.6, nq)], 1)
        tot, pp, info, _ = _run(np.ascontiguousarray(pts), v, tri, max_distance=0.4, thresholds=[0.1, 0.25])
        assert info["depth"] == depth and info["triangles"] == nt and tot["n_query"] == nq


def _cube():
    v = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # outward winding
    tri = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, tri


def test_closed_cube_signs():
    v, tri = _cube()
    nrm = R.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    assert (np.einsum("ij,ij->i", nrm, v[tri].mean(1)) > 0).all()  # every normal points out of the cube
    rng = np.random.default_rng(5)
    inside, outside = rng.uniform(-0.95, 0.95, (1000, 3)), rng.uniform(-3, 3, (1000, 3))
    outside = outside[np.abs(outside).max(1) > 1.05]
    with _engine() as e:
        e.mesh_upload(v, tri)
        for pts, sign in ((inside, -1), (np.ascontiguousarray(outside), 1)):
            e.upload(0, pts)
            tot, pp = e.mesh_distance(0, fetch=True)
            m = _check(tot, pp, pts, v, tri)
            assert tot["face_share"] == (m["region"] == R.FACE).mean() > 0
            assert sign * tot["signed_mean"] > 0 and (sign * pp["signed_d"][pp["region"] == R.FACE] >= 0).all()
            assert tot["signed_mean_abs"] == pytest.approx(abs(tot["signed_mean"]), rel=1e-12)


@pytest.fixture(scope="module")
def field():
    v, tri = synth.heightfield_mesh(40, 40, 0.5, 0.6, seed=2)
    rng = np.random.default_rng(8)
    # queries at and around vertices and along edges, within +-3 steps: shared features of 2-6 triangles
    at = v[rng.integers(0, len(v), 900)] + np.outer(rng.integers(-3, 4, 900) * 0.5, [0.0, 0.0, 1.0])
    mid = 0.5 * (v[tri[:600, 0]] + v[tri[:600, 1]]) + rng.normal(0, 0.4, (600, 1)) * [0.0, 0.0, 1.0]
    free = np.stack([rng.uniform(-1.5, 21, 500), rng.uniform(-1.5, 21, 500), rng.uniform(-1.5, 1.5, 500)], 1)
    pts = np.ascontiguousarray(np.concatenate([at, mid, free]))
    return v, tri, pts, R.distance(pts, v, tri)


def test_heightfield_ties_across_shared_edges(field):
    v, tri, pts, model = field
    assert len(tri) == 3042
    tot, pp, info, m = _run(pts, v, tri, thresholds=[0.05, 0.5], model=model)
    assert info["depth"] == 4 and set(m["region"].tolist()) == set(range(7))
    # the tie rule is exercised: a good part of the closest features are edges and vertices, and many queries have a second triangle
    # at the bitwise-same distance (both are properties of the queries, counted on the model)
    assert (m["region"] != R.FACE).mean() > 0.3
    a, b, g = (v[tri][None, :, k] for k in range(3))
    dd = R.closest(pts[:200, None, :], a, b, g)[0]
    assert ((dd == dd.min(1, keepdims=True)).sum(1) > 1).mean() > 0.3


def test_heightfield_at_survey_coordinates(field):
    """the same mesh and queries moved by (1100, -1100, 1100) m: the pruning margin at large coordinate magnitude"""
    v, tri, pts, _ = field
    off = np.array([1100.0, -1100.0, 1100.0])
    _run(np.ascontiguousarray(pts + off), np.ascontiguousarray(v + off), tri)


def test_transform_is_the_uploads(field):
    v, tri, pts, _ = field
    T = np.array([[0.0, -1, 0, 3], [1, 0, 0, -2], [0, 0, 1, 0.5], [0, 0, 0, 1]])
    with _engine() as e:
        e.upload(1, v, T=T)
        vt = e.download(1)
    tot, pp, info, _ = _run(pts[:300], v, tri[:400], T=T, model=R.distance(pts[:300], vt, tri[:400]))
    assert np.array_equal(info["bbox_lo"], vt[np.unique(tri[:400])].min(0))


def test_duplicated_triangles_lower_index_wins():
    v, tri = synth.heightfield_mesh(9, 9, 0.5, 0.3, seed=4)
    rng = np.random.default_rng(9)
    order = rng.permutation(len(tri))
    both = np.ascontiguousarray(np.concatenate([tri[order], tri]))  # every triangle twice, the copies far apart in the list
    pts = np.stack([rng.uniform(-0.5, 4.5, 1500), rng.uniform(-0.5, 4.5, 1500), rng.uniform(-0.5, 0.5, 1500)], 1)
    tot, pp, info, m = _run(pts, v, both)
    assert (pp["tri"] < len(tri)).all() and info["triangles"] == 2 * len(tri)  # (the model's equality has checked which one)


def test_degenerate_triangles_are_segments():
    v = np.array([[0.0, 0, 0], [2, 0, 0], [4, 0, 0], [0, 2, 1], [np.nan, 0, 0], [5, 5, 5]])
    tri = np.array([[0, 1, 2], [0, 0, 3], [3, 3, 3]], np.int32)  # collinear; a repeated index; a single point
    rng = np.random.default_rng(10)
    pts = rng.uniform(-3, 7, (700, 3))
    tot, pp, info, m = _run(pts, v, tri)  # (vertex 4 is NaN and unreferenced: accepted)
    assert (info["degenerate"], info["area"], info["vertices"]) == (3, 0.0, 6)
    assert (pp["region"] != R.FACE).all() and tot["n_face"] == 0

    def seg(p, a, b):
        t = np.clip(((p - a) @ (b - a)) / ((b - a) @ (b - a)), 0, 1)
        return np.linalg.norm(p - (a + t[:, None] * (b - a)), axis=1)

    d = np.minimum(seg(pts, v[0], v[2]), seg(pts, v[0], v[3]))
    assert np.allclose(np.sqrt(pp["d2"]), d, rtol=1e-12, atol=0)
    with _engine() as e:
        with pytest.raises(Exception, match="non-finite"):
            e.mesh_upload(v, np.array([[0, 1, 4]], np.int32))
        with pytest.raises(Exception, match="outside"):
            e.mesh_upload(v, np.array([[0, 1, 6]], np.int32))
        with pytest.raises(Exception, match="n_triangles"):
            e.mesh_upload(v, np.zeros((0, 3), np.int32))
        e.mesh_upload(v, tri)
        with pytest.raises(Exception, match="area"):
            e.mesh_sample(1, 10)


def test_queries_a_thousand_diameters_away(field):
    v, tri, _, _ = field
    rng = np.random.default_rng(11)
    d = rng.normal(size=(300, 3))
    pts = v.mean(0) + 1000.0 * 30.0 * d / np.linalg.norm(d, axis=1)[:, None]
    _run(np.ascontiguousarray(pts), v, tri)


def test_gate_at_one_ulp():
    v = np.array([[-1.0, -1, 0], [3, -1, 0], [-1, 3, 0]])
    tri = np.array([[0, 1, 2]], np.int32)
    pts = np.array([[0.25, 0.25, 0.5], [0.5, 0.25, np.nextafter(0.5, 1.0)]])
    tot, pp, _, _ = _run(pts, v, tri, max_distance=0.5)
    assert pp["d2"].tolist() == [0.25, np.nextafter(0.5, 1.0) ** 2] and (tot["n_matched"], tot["worst_index"], tot["max"]) == (1, 0, 0.5)
    tot, pp, _, _ = _run(pts, v, tri, thresholds=[0.5])
    assert tot["n_matched"] == 2 and tot["n_within"].tolist() == [1] and tot["worst_index"] == 1
    tot, _, _, _ = _run(pts, v, tri, max_distance=0.0)
    assert (tot["n_matched"], tot["worst_index"], tot["mean"]) == (0, -1, 0.0)


def test_state_and_errors():
    v, tri = synth.heightfield_mesh(12, 12, 0.5, 0.3, seed=6)
    rng = np.random.default_rng(12)
    pts = np.stack([rng.uniform(0, 5.5, 3000), rng.uniform(0, 5.5, 3000), rng.uniform(-0.3, 0.3, 3000)], 1)
    other = pts[:2000] + 0.01
    state = "\\[-3\\]"
    with _engine() as e:
        with pytest.raises(Exception, match=state):
            e.mesh_info()
        e.upload(0, pts, cell_size=0.2)
        with pytest.raises(Exception, match=state):  # no mesh
            e.mesh_distance(0)
        e.mesh_upload(v, tri)
        with pytest.raises(Exception, match=state):  # no cloud in slot 1, no result in slot 0
            e.mesh_distance(1)
        with pytest.raises(Exception, match=state):
            e.mesh_distance_fetch(0)
        tot, pp = e.mesh_distance(0, fetch=True)
        e.upload(1, other, cell_size=0.2)  # the other slot's upload, a search and an MME leave the result alone
        e.nn1(0, 1)
        e.mme(0, 0.2, 5)
        again = e.mesh_distance_fetch(0)
        assert all(pp[k].tobytes() == again[k].tobytes() for k in pp)
        t = e.twin()  # a twin sees the mesh and the result
        assert t.mesh_info()["triangles"] == len(tri)
        t2, p2 = t.mesh_distance(0, fetch=True)
        assert all(pp[k].tobytes() == p2[k].tobytes() for k in pp) and t2["sum_d"] == tot["sum_d"]
        # dropped by a new upload of the query slot, by a new mesh and by mesh_clear
        e.upload(0, pts, cell_size=0.2)
        with pytest.raises(Exception, match=state):
            e.mesh_distance_fetch(0)
        e.mesh_distance(0)
        e.mesh_upload(v, tri)
        with pytest.raises(Exception, match=state):
            e.mesh_distance_fetch(0)
        e.mesh_distance(0)
        e.mesh_distance_fetch(0)
        e.mesh_clear()
        with pytest.raises(Exception, match=state):
            e.mesh_distance_fetch(0)
        with pytest.raises(Exception, match=state):
            e.mesh_distance(0)
        e.mesh_upload(v, tri)
        arg = "\\[-1\\]"
        for kw in ({"max_distance": -1.0}, {"max_distance": math.nan}, {"thresholds": [-0.1]}, {"thresholds": [math.inf]},
                   {"thresholds": [math.nan]}, {"thresholds": [0.1] * 9}):
            with pytest.raises(Exception, match=arg):
                e.mesh_distance(0, **kw)
        p, o = _lib.MeshParams(), _lib.MeshOut()
        p.max_distance = 1.0
        assert e._L.me_mesh_distance(e._ctx, 2, C.byref(p), C.byref(o)) == -1
        assert e._L.me_mesh_distance(e._ctx, 0, None, C.byref(o)) == -1 and e._L.me_mesh_distance(e._ctx, 0, C.byref(p), None) == -1
        p.n_thresholds = 9
        assert e._L.me_mesh_distance(e._ctx, 0, C.byref(p), C.byref(o)) == -1
        with pytest.raises(Exception, match=arg):
            e.mesh_sample(1, 0)
        e.set_shard(0, 2)
        with pytest.raises(Exception, match=arg):
            e.mesh_distance(0)


def test_mesh_sample_bit_for_bit_and_on_its_own_mesh():
    v, tri = synth.heightfield_mesh(30, 25, 0.5, 0.6, seed=13)
    n = 10007
    with _engine() as e:
        e.mesh_upload(v, tri)
        assert e.mesh_sample(1, n, seed=77) == n
        got = e.download(1)
        want, _ = R.sample(v, tri, n, 77)
        assert np.array_equal(got, want)
        assert e.mesh_info()["area"] == np.cumsum(R.areas(v, tri)[0])[-1]
        e.upload(0, want[:3000] + [0.0, 0.0, 0.01])
        idx, d2 = e.nn1(0, 1)  # the sampled slot indexes and answers a search
        assert (d2 <= 0.01 ** 2 * (1 + 1e-9)).all() and (d2 > 0).all()
        tot, pp = e.mesh_distance(1, fetch=True)
        extent = np.abs(v).max()  # the scale of the sampler's and the routine's roundings
        assert (pp["d2"] < (8 * U * extent) ** 2).all()
        e.mesh_sample(1, 100, seed=78)
        assert e.size(1) == 100 and not np.array_equal(e.download(1), want[:100])


def test_mesh_report():
    v, tri = synth.heightfield_mesh(40, 40, 0.5, 0.6, seed=2)
    n = 20000
    pts = R.sample(v, tri, n, 5)[0] + np.random.default_rng(14).normal(0, 0.02, (n, 3))
    ths, qs = [0.01, 0.03, 0.1], (0.5, 0.9, 0.99, 1.0)
    with _engine() as e:
        e.upload(0, pts)
        e.mesh_upload(v, tri)
        rep = e.mesh_report(ths, qs, sample_points=15000, seed=3, max_distance=0.05)
        d2 = e.mesh_distance_fetch(0)["d2"]
        d = np.sort(np.sqrt(d2[d2 <= 0.05 * 0.05]))
        assert rep["n_matched"] == len(d) < n
        assert np.array_equal(rep["quantile_d"], d[[max(0, math.ceil(q * len(d)) - 1) for q in qs]])
        assert rep["max"] == d[-1] == rep["quantile_d"][-1] and rep["mean"] == pytest.approx(d.mean(), rel=1e-12)
        assert np.array_equal(e.download(1), R.sample(v, tri, 15000, 3)[0])
        s = rep["sampled"]
        for k in range(len(ths)):
            prf = e.fscore(s["est"]["n_within"][k], s["est"]["n_used"], s["gt"]["n_within"][k], s["gt"]["n_used"])
            assert (s["precision"][k], s["recall"][k], s["fscore"][k]) == prf
        assert 0 < s["recall"][0] < s["recall"][-1] <= 1 and 0 < rep["face_share"] <= 1
