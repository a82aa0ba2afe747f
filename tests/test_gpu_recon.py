"""me_reconstruct end to end on the MI355X: the device mesh equals the model's extraction (tests/_recon_ref.py) of the device's OWN
fetched field, exactly — rounding order in the field cannot enter and no node is excluded; a sphere is closed with V - E + T = 2 and
lies where the construction says; a plane patch has boundary only at the rim of the active set; install equals upload of the fetched
arrays; the state and argument errors."""
import math

import numpy as np
import pytest

import _recon_ref as rr

pytestmark = pytest.mark.gpu


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _against_own_field(e, d, h, points, band):
    nd = e.reconstruct_nodes()
    _, act, _ = rr.lattice(points, h, band)
    m = rr.isosurface(nd["node_ijk"], nd["f"], nd["valid"], h, cells=set(act))
    assert d["n_cells_extracted"] == m["n_cells_extracted"]
    assert d["n_vertices"] == len(m["vertices"]) and d["n_triangles"] == len(m["triangles"])
    dv = {tuple(k): v.tobytes() for k, v in zip(d["vertex_edge"].tolist(), d["vertices"])}
    mv = {tuple(k): v.tobytes() for k, v in zip(m["vertex_edge"].tolist(), m["vertices"])}
    assert dv == mv
    assert rr.oriented_set(d["vertex_edge"], d["triangles"]) == rr.oriented_set(m["vertex_edge"], m["triangles"])
    return nd


@pytest.fixture(scope="module")
def sphere():
    rng = np.random.default_rng(2024)
    u = rng.normal(size=(20000, 3))
    n = u / np.sqrt((u * u).sum(1))[:, None]
    jitter = 0.004
    p = n * (1.0 + rng.uniform(-jitter, jitter, (20000, 1)))
    return p, n, jitter


def test_sphere_is_closed_and_equals_the_model_on_the_device_field(sphere):
    p, n, jitter = sphere
    h, band = 0.1, 1
    with _engine() as e:
        e.upload(0, p)
        e.set_normals(0, n)
        d = e.reconstruct(0, h, band=band)
        d2 = e.reconstruct(0, h, band=band)
        assert all(np.asarray(d[k]).tobytes() == np.asarray(d2[k]).tobytes() for k in d)
        _against_own_field(e, d, h, p, band)
    assert d["n_triangles"] > 2000
    assert rr.boundary_edges(d["triangles"]) == []
    assert rr.euler_characteristic(d["n_vertices"], d["triangles"]) == 2
    r = np.sqrt((d["vertices"] ** 2).sum(1))
    assert np.abs(r - 1.0).max() <= (band + 1) * math.sqrt(3.0) * h + jitter  # a vertex lies in an active cell
    print(f"sphere: V={d['n_vertices']} T={d['n_triangles']} max |r - 1| = {np.abs(r - 1.0).max():.4f}, mean {np.abs(r - 1.0).mean():.5f}")
    # outward winding: (B - A) x (C - A) along the radius on every triangle with an area
    v, t = d["vertices"], d["triangles"]
    nn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    c = (v[t[:, 0]] + v[t[:, 1]] + v[t[:, 2]]) / 3.0
    assert ((nn * c).sum(1) >= 0).all()


def test_plane_patch_has_boundary_only_at_the_rim_of_the_active_set():
    rng = np.random.default_rng(77)
    m = 6000
    p = np.column_stack([rng.random(m) * 3.0, rng.random(m) * 2.0, 0.437 + rng.uniform(-0.003, 0.003, m)])
    n = np.tile([0.0, 0.0, 1.0], (m, 1))
    h, band = 0.125, 1
    with _engine() as e:
        e.upload(0, p)
        e.set_normals(0, n)
        d = e.reconstruct(0, h, band=band)
        _against_own_field(e, d, h, p, band)
    assert d["n_triangles"] > 500
    assert np.abs(d["vertices"][:, 2] - 0.437).max() < 0.01
    _, act, _ = rr.lattice(p, h, band)
    act = set(act)
    ve = d["vertex_edge"]
    for a, b in rr.boundary_edges(d["triangles"]):
        # both vertices of a boundary edge lie on lattice edges of a rim cell: a cell with a missing neighbour in the active set
        i, j, k = ve[a][:3].tolist()
        near = [(i + dx, j + dy, k + dz) for dx in (-1, 0) for dy in (-1, 0) for dz in (-1, 0)]
        rim = [c for c in near if c in act and any((c[0] + ex, c[1] + ey, c[2]) not in act for ex in (-1, 0, 1) for ey in (-1, 0, 1))]
        assert rim, (a, b)


def test_install_equals_upload_of_the_fetched_arrays(sphere):
    p, n, _ = sphere
    q = p[:3000] * 1.02
    with _engine() as e:
        e.upload(0, p)
        e.set_normals(0, n)
        e.upload(1, q)
        d = e.reconstruct(0, 0.1, install=True)
        info_a = e.mesh_info()
        tot_a, pp_a = e.mesh_distance(1, fetch=True)
        e.mesh_upload(d["vertices"], d["triangles"])
        info_b = e.mesh_info()
        tot_b, pp_b = e.mesh_distance(1, fetch=True)
    assert info_a["triangles"] == d["n_triangles"] and info_a["degenerate"] == d["n_degenerate"]
    assert all(np.asarray(info_a[k]).tobytes() == np.asarray(info_b[k]).tobytes() for k in info_a)
    assert all(np.asarray(tot_a[k]).tobytes() == np.asarray(tot_b[k]).tobytes() for k in tot_a)
    assert all(pp_a[k].tobytes() == pp_b[k].tobytes() for k in pp_a)
    assert tot_a["signed_mean"] > 0  # the query lies outside the sphere: signed_d > 0 outside


def test_state_and_argument_errors():
    from cloud_map_evaluation_amd.engine import MapEvalError

    rng = np.random.default_rng(1)
    p = rng.random((100, 3))
    n = np.tile([0.0, 0.0, 1.0], (100, 1))
    with _engine() as e:
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.reconstruct(0, 0.1)  # no cloud
        e.upload(0, p)
        with pytest.raises(MapEvalError, match=r"\[-3\].*normals"):
            e.reconstruct(0, 0.1)
        e.set_normals(0, n)
        with pytest.raises(MapEvalError, match=r"\[-1\].*radius"):
            e.reconstruct(0, 0.1, radius=0.05)
        with pytest.raises(MapEvalError, match=r"\[-1\].*band"):
            e.reconstruct(0, 0.1, band=3)
        with pytest.raises(MapEvalError, match=r"\[-1\].*min_k"):
            e.reconstruct(0, 0.1, min_k=0)
        with pytest.raises(MapEvalError, match=r"\[-1\].*voxel"):
            e.reconstruct(0, float("nan"))
        with pytest.raises(MapEvalError, match=r"\[-1\].*2\^21"):
            e.reconstruct(0, 1e-8, radius=1e-8)
        d = e.reconstruct(0, 0.1, min_k=1000)  # no valid node: zeros, not an error
        assert d["n_valid_nodes"] == 0 and d["n_cells_extracted"] == 0 and d["n_triangles"] == 0 and d["triangles"].shape == (0, 3)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.reconstruct_install()
        assert len(e.reconstruct_nodes()["f"]) == d["n_nodes"]
    with _engine() as e:
        e.set_slab(0, 0.0, 0.5, 0.1)
        e.upload(0, p)
        with pytest.raises(MapEvalError, match=r"\[-1\].*single GPU"):
            e.reconstruct(0, 0.1)
