"""me_isosurface on the MI355X against the model of tests/_recon_ref.py, EXACTLY: after matching vertices through vertex_edge the
vertex coordinates are bit-equal and the sets of oriented triangles are equal; two calls return identical bytes."""
import numpy as np
import pytest

import _recon_ref as rr

pytestmark = pytest.mark.gpu


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _run(e, ijk, f, valid, h):
    d = e.isosurface(ijk, f, valid, h)
    d2 = e.isosurface(ijk, f, valid, h)
    for k in d:
        assert np.asarray(d[k]).tobytes() == np.asarray(d2[k]).tobytes(), k
    m = rr.isosurface(ijk, f, valid, h)
    assert d["n_nodes"] == len(ijk) and d["n_valid_nodes"] == int(np.count_nonzero(valid))
    assert d["n_cells_extracted"] == m["n_cells_extracted"]
    assert d["n_vertices"] == len(m["vertices"]) and d["n_triangles"] == len(m["triangles"])
    dv = {tuple(k): v.tobytes() for k, v in zip(d["vertex_edge"].tolist(), d["vertices"])}
    mv = {tuple(k): v.tobytes() for k, v in zip(m["vertex_edge"].tolist(), m["vertices"])}
    assert len(dv) == d["n_vertices"]
    assert dv == mv  # the same edges carry a vertex, at bit-equal coordinates
    assert rr.oriented_set(d["vertex_edge"], d["triangles"]) == rr.oriented_set(m["vertex_edge"], m["triangles"])
    if d["n_triangles"]:
        v, t = d["vertices"], d["triangles"]
        n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
        assert d["n_degenerate"] == int((n == 0).all(axis=1).sum())
    return d


def _block(lo, hi):
    g = range(lo, hi + 1)
    return np.array([(i, j, k) for i in g for j in g for k in g], np.int32)


def test_the_256_patterns_of_one_cell_with_mixed_magnitudes():
    ijk = _block(0, 1)
    rng = np.random.default_rng(11)
    ok = np.ones(8, bool)
    with _engine() as e:
        for pattern in range(256):
            mag = 10.0 ** rng.uniform(-6, 3, 8)
            f = np.where([(pattern >> b) & 1 for b in range(8)], -mag, mag)
            d = _run(e, ijk, f, ok, 0.37)
            assert (d["n_triangles"] == 0) == (pattern in (0, 255))


def test_zero_negative_zero_and_equal_magnitudes_hit_both_ends_of_the_clamp():
    ijk = _block(0, 1)
    ok = np.ones(8, bool)
    x0 = ijk[:, 0] == 0
    with _engine() as e:
        d = _run(e, ijk, np.where(x0, -1.0, 0.0), ok, 2.0)  # outside end exactly 0, inside origin: t = 1
        assert d["n_triangles"] > 0 and (d["vertices"][:, 0] == 2.0).all() and d["n_degenerate"] > 0
        d = _run(e, ijk, np.where(x0, -0.0, -3.0), ok, 2.0)  # -0.0 is outside and the origin: t = -0.0
        assert d["n_triangles"] > 0 and (d["vertices"][:, 0] == 0.0).all()
        d = _run(e, ijk, np.where(x0, 0.0, -3.0), ok, 2.0)
        assert d["n_triangles"] > 0 and (d["vertices"][:, 0] == 0.0).all()
        d = _run(e, ijk, np.where(x0, -2.5, 2.5), ok, 2.0)  # equal magnitudes: t = 0.5 exactly
        assert (d["vertices"][:, 0] == 1.0).all()
        d = _run(e, ijk, np.where(ijk.sum(1) == 0, -1.0, 0.0), ok, 1.0)  # one inside corner, all three vertices at t = 1: kept
        assert d["n_triangles"] == 6 and d["n_degenerate"] == 0
        f = np.zeros(8)
        f[7] = -1.0  # the inside corner is the END of every edge: t = 0 / (0 + 1) = 0, all vertices at their origins
        d = _run(e, ijk, f, ok, 1.0)
        assert d["n_triangles"] == 6
        assert _run(e, ijk, np.zeros(8), ok, 1.0)["n_triangles"] == 0
        assert _run(e, ijk, np.full(8, -0.0), ok, 1.0)["n_triangles"] == 0


def test_an_invalid_or_absent_corner_gives_no_cell_and_no_stray_vertex():
    ijk = _block(0, 2)
    f = np.where(ijk[:, 0] == 0, -1.0, 1.0)
    with _engine() as e:
        full = _run(e, ijk, f, np.ones(27, bool), 1.0)
        assert full["n_cells_extracted"] == 8
        ok = np.ones(27, bool)
        ok[13] = False  # the centre node: a corner of all 8 cells
        d = _run(e, ijk, f, ok, 1.0)
        assert d["n_cells_extracted"] == 0 and d["n_vertices"] == 0 and d["n_triangles"] == 0
        keep = np.arange(27) != 13  # the same node absent
        d = _run(e, ijk[keep], f[keep], np.ones(26, bool), 1.0)
        assert d["n_cells_extracted"] == 0 and d["n_vertices"] == 0
        ok = np.ones(27, bool)
        ok[26] = False  # the corner (2,2,2): only its cell goes
        d = _run(e, ijk, f, ok, 1.0)
        assert d["n_cells_extracted"] == 7
        bad = f.copy()
        bad[26] = np.nan  # a non-finite f on an INVALID node is ignored
        assert _run(e, ijk, bad, ok, 1.0)["n_cells_extracted"] == 7


def test_duplicates_non_finite_values_and_state_errors():
    from cloud_map_evaluation_amd.engine import MapEvalError

    ijk = _block(0, 1)
    f = np.where(ijk[:, 0] == 0, -1.0, 1.0)
    with _engine() as e:
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e._recon_fetch({"n_vertices": 0, "n_triangles": 0})
        with pytest.raises(MapEvalError, match=r"\[-1\].*more than once"):
            e.isosurface(np.concatenate([ijk, ijk[3:4]]), np.append(f, 1.0), np.ones(9, bool), 1.0)
        with pytest.raises(MapEvalError, match=r"\[-1\].*non-finite"):
            e.isosurface(ijk, np.where(np.arange(8) == 2, np.inf, f), np.ones(8, bool), 1.0)
        with pytest.raises(MapEvalError, match=r"\[-1\].*voxel"):
            e.isosurface(ijk, f, np.ones(8, bool), 0.0)
        wide = ijk.copy()
        wide[7, 0] = 1 << 21
        with pytest.raises(MapEvalError, match=r"\[-1\].*2\^21"):
            e.isosurface(wide, f, np.ones(8, bool), 1.0)
        d = e.isosurface(ijk, f, np.ones(8, bool), 1.0)
        assert d["n_triangles"] > 0
        with pytest.raises(MapEvalError, match=r"\[-3\]"):  # me_isosurface keeps no node field
            e.reconstruct_nodes()
        e.set_shard(0, 2)
        with pytest.raises(MapEvalError, match=r"\[-1\].*single GPU"):
            e.isosurface(ijk, f, np.ones(8, bool), 1.0)


def test_one_node_and_no_node_give_an_empty_result():
    with _engine() as e:
        for n in (1, 0):
            d = e.isosurface(np.zeros((n, 3), np.int32), np.full(n, -1.0), np.ones(n, bool), 1.0)
            assert d["n_nodes"] == n and d["n_cells_extracted"] == 0 and d["n_vertices"] == 0 and d["n_triangles"] == 0
            assert d["vertices"].shape == (0, 3) and d["triangles"].shape == (0, 3)


@pytest.mark.parametrize("origin,h", [((-1, -1, -1), 0.25), ((1000000 - 1, -1000000 - 1, 4000), 0.05)])
def test_a_block_of_cells_across_negative_indices_and_at_survey_coordinates(origin, h):
    ijk = _block(0, 2) + np.array(origin, np.int32)
    rng = np.random.default_rng(3)
    with _engine() as e:
        for _ in range(4):
            f = rng.normal(size=27)
            d = _run(e, ijk, f, np.ones(27, bool), h)
            assert d["n_cells_extracted"] == 8 and d["n_triangles"] > 0
        perm = rng.permutation(27)  # the caller's node order does not matter
        a = e.isosurface(ijk, f, np.ones(27, bool), h)
        b = e.isosurface(ijk[perm], f[perm], np.ones(27, bool), h)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.mark.parametrize("name,chi", [("sphere", 2), ("torus", 0)])
def test_closed_fields_are_closed_with_the_right_euler_characteristic(name, chi):
    ijk, f = rr.sphere_field() if name == "sphere" else rr.torus_field()
    with _engine() as e:
        d = _run(e, ijk, f, np.ones(len(ijk), bool), 1.0)
    assert d["n_cells_extracted"] == 16 ** 3 and d["n_triangles"] > 100
    assert rr.boundary_edges(d["triangles"]) == []
    assert rr.euler_characteristic(d["n_vertices"], d["triangles"]) == chi
