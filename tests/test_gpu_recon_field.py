"""The IMLS field of me_reconstruct on the MI355X against the model of tests/_recon_ref.py: the node set, k and validity EQUAL on
every node, |f - f_model| <= (2k + 4) 2^-53 R on every valid node (the derivation: _recon_ref.field_bound)."""
import numpy as np
import pytest

import _recon_ref as rr

pytestmark = pytest.mark.gpu


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _cloud(n, seed, centre=(0.0, 0.0, 0.0), box=1.0):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * box + np.array(centre)
    v = rng.normal(size=(n, 3))
    return p, v / np.sqrt((v * v).sum(1))[:, None]


def _check(e, p, nrm, h, R, min_k, band, slot=0):
    e.upload(slot, p)
    e.set_normals(slot, nrm)
    c = e.reconstruct(slot, h, R, min_k, band, fetch=False)
    nd = e.reconstruct_nodes()
    c2 = e.reconstruct(slot, h, R, min_k, band, fetch=False)
    nd2 = e.reconstruct_nodes()
    assert c == c2 and all(nd[k].tobytes() == nd2[k].tobytes() for k in nd)  # two calls: identical bytes
    m = rr.field(p, nrm, h, R, min_k, band)
    assert c["n_occupied_cells"] == len(m["occupied"]) and c["n_active_cells"] == len(m["active"])
    assert c["n_nodes"] == len(m["node_ijk"]) == len(nd["node_ijk"])
    order = np.lexsort((nd["node_ijk"][:, 2], nd["node_ijk"][:, 1], nd["node_ijk"][:, 0]))  # the model's order: ascending (i, j, k)
    assert np.array_equal(nd["node_ijk"][order], m["node_ijk"])
    k, valid, f = nd["k"][order], nd["valid"][order], nd["f"][order]
    assert np.array_equal(k, m["k"])
    assert np.array_equal(valid, m["valid"])
    assert c["n_valid_nodes"] == int(valid.sum()) and c["sum_k"] == int(k.sum())
    assert (f[~valid] == 0.0).all()
    err = np.abs(f - m["f"])[valid]
    bound = rr.field_bound(k[valid], R)
    if valid.any():
        print(f"n={len(p)} nodes={len(k)} valid={int(valid.sum())} max k={int(k.max())} max err/bound={float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    return c, {"node_ijk": nd["node_ijk"][order], "k": k, "valid": valid, "f": f}, m


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_field_equals_the_model_at_the_wave_edges(n):
    p, nrm = _cloud(n, n)
    with _engine() as e:
        c, nd, m = _check(e, p, nrm, 0.2, 0.3, 1 if n < 100 else 8, 1)
    assert c["n_valid_nodes"] > 0


def test_a_point_at_exactly_the_radius_is_excluded():
    # one point at the origin, h = 0.5, R = 1.5: the nodes (3,0,0) and (2,2,1) are at d2 = 2.25 = R*R exactly, (2,2,0) at d2 = 2
    p = np.zeros((1, 3))
    nrm = np.array([[0.0, 0.0, 1.0]])
    with _engine() as e:
        c, nd, m = _check(e, p, nrm, 0.5, 1.5, 1, 2)
    at = {tuple(r): n for n, r in enumerate(nd["node_ijk"].tolist())}
    assert nd["k"][at[(3, 0, 0)]] == 0 and nd["k"][at[(2, 2, 1)]] == 0 and not nd["valid"][at[(3, 0, 0)]]
    assert nd["k"][at[(2, 2, 0)]] == 1 and nd["valid"][at[(2, 2, 0)]]
    assert nd["f"][at[(1, 1, 1)]] == 0.5 and nd["f"][at[(0, 0, -1)]] == -0.5  # f = n . (x - p)


def test_min_k_is_met_exactly_or_missed_by_one():
    p, nrm = _cloud(300, 7)
    m = rr.field(p, nrm, 0.25, 0.4, 1, 1)
    K = int(np.sort(m["k"])[len(m["k"]) // 2])
    assert K >= 2
    with _engine() as e:
        _, a, _ = _check(e, p, nrm, 0.25, 0.4, K, 1)
        _, b, _ = _check(e, p, nrm, 0.25, 0.4, K + 1, 1)
    at = a["k"] == K
    assert at.any() and a["valid"][at].all() and not b["valid"][at].any()


def test_zero_and_non_finite_normals_are_skipped_and_not_counted():
    p, nrm = _cloud(500, 9)
    nrm[::3] = 0.0
    nrm[1, 0] = np.nan
    nrm[4, 2] = np.inf
    with _engine() as e:
        c, nd, m = _check(e, p, nrm, 0.2, 0.35, 4, 1)
        full = rr.field(p, _cloud(500, 9)[1], 0.2, 0.35, 4, 1)
    assert nd["k"].sum() < full["k"].sum() and np.isfinite(nd["f"]).all()


def test_survey_coordinates():
    p, nrm = _cloud(1500, 21, centre=(4.0e5, -3.0e5, 50.0), box=2.0)
    with _engine() as e:
        c, nd, m = _check(e, p, nrm, 0.25, 0.5, 6, 1)
    assert c["n_valid_nodes"] > 100


@pytest.mark.parametrize("band", [0, 1, 2])
def test_the_node_set_of_every_band(band):
    rng = np.random.default_rng(band)
    # two clusters one empty cell apart and a lone point: with band 0 the cell between the clusters has all 8 corners and is not active
    p = np.concatenate([rng.random((40, 3)) * 0.3 + [-0.3, 0, 0], rng.random((40, 3)) * 0.3 + [0.3, 0, 0], [[-2.05, 1.31, 0.77]]])
    v = rng.normal(size=(81, 3))
    nrm = v / np.sqrt((v * v).sum(1))[:, None]
    with _engine() as e:
        c, nd, m = _check(e, p, nrm, 0.3, 0.6, 2, band)
        d = e.reconstruct(0, 0.3, 0.6, 2, band)
        nodes = e.reconstruct_nodes()
    mm = rr.isosurface(nodes["node_ijk"], nodes["f"], nodes["valid"], 0.3, cells=set(m["active"]))
    assert d["n_cells_extracted"] == mm["n_cells_extracted"]
    assert rr.oriented_set(d["vertex_edge"], d["triangles"]) == rr.oriented_set(mm["vertex_edge"], mm["triangles"])


def test_the_other_slot_is_untouched():
    p, nrm = _cloud(200, 31)
    q, qn = _cloud(333, 32, centre=(5.0, 5.0, 5.0))
    with _engine() as e:
        e.upload(1, q)
        e.set_normals(1, qn)
        _check(e, p, nrm, 0.2, 0.3, 3, 1, slot=0)
        assert np.array_equal(e.download(1), q) and np.array_equal(e.get_normals(1), qn) and e.size(1) == 333
        assert np.array_equal(e.download(0), p) and np.array_equal(e.get_normals(0), nrm)
