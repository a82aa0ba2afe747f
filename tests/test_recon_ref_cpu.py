"""The reconstruction model (tests/_recon_ref.py) against itself: the marching-tetrahedra case table is closed, the Kuhn cut matches
across cell faces, and the winding follows +grad f.  No GPU."""
import numpy as np
import pytest

import _recon_ref as rr


def _block27():
    g = (-1, 0, 1, 2)
    return np.array([(i, j, k) for i in g for j in g for k in g], np.int32)


def test_all_256_patterns_of_a_cell_give_closed_surfaces():
    """The 8 corners of the cell (0,0,0) take every sign pattern, the nodes around them are outside: the zero set of the 3x3x3-cell
    block is closed — every directed edge has its reverse exactly once.  (All-outside: no triangle at all.)"""
    ijk = _block27()
    centre = [n for n, p in enumerate(ijk.tolist()) if all(0 <= c <= 1 for c in p)]
    assert len(centre) == 8
    rng = np.random.default_rng(5)
    for pattern in range(256):
        f = 0.25 + rng.random(len(ijk))
        for b, n in enumerate(centre):
            if (pattern >> b) & 1:
                f[n] = -(0.25 + rng.random())
        m = rr.isosurface(ijk, f, np.ones(len(ijk), bool), 0.5)
        assert m["n_cells_extracted"] == 27
        if pattern == 0:
            assert len(m["triangles"]) == 0 and len(m["vertices"]) == 0
            continue
        assert rr.boundary_edges(m["triangles"]) == [], pattern
        assert len({tuple(r) for r in m["vertex_edge"].tolist()}) == len(m["vertices"])


def _outward(m, grad):
    v, t = m["vertices"], m["triangles"]
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    n = np.cross(b - a, c - a)
    g = grad((a + b + c) / 3.0)
    return (n * g).sum(1), np.sqrt((n * n).sum(1)) * np.sqrt((g * g).sum(1))


@pytest.mark.parametrize("name,chi", [("sphere", 2), ("torus", 0)])
def test_closed_fields_have_the_right_euler_characteristic_and_winding(name, chi):
    centre = np.array((8.1, 7.9, 8.2))
    if name == "sphere":
        ijk, f = rr.sphere_field()
        grad = lambda p: p - centre
    else:
        ijk, f = rr.torus_field()

        def grad(p):
            d = p - centre
            rho = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
            g = np.empty_like(d)
            g[:, 0] = (rho - 4.6) * d[:, 0] / rho
            g[:, 1] = (rho - 4.6) * d[:, 1] / rho
            g[:, 2] = d[:, 2]
            return g
    m = rr.isosurface(ijk, f, np.ones(len(ijk), bool), 1.0)
    assert len(m["triangles"]) > 100
    assert rr.boundary_edges(m["triangles"]) == []
    assert rr.euler_characteristic(len(m["vertices"]), m["triangles"]) == chi
    dot, scale = _outward(m, grad)
    assert (dot >= 0).all()
    # a triangle with a real area points along +grad f (the cut is coarse: within 60 degrees)
    big = scale > 1e-9
    assert (dot[big] > 0.5 * scale[big]).mean() > 0.95 and (dot[big] > 0).all()


def test_invalid_and_absent_corners_give_no_cell_and_no_vertex():
    g = (0, 1)
    ijk = np.array([(i, j, k) for i in g for j in g for k in g], np.int32)
    f = np.where(ijk[:, 0] == 0, -1.0, 1.0)
    ok = np.ones(8, bool)
    assert len(rr.isosurface(ijk, f, ok, 1.0)["triangles"]) > 0
    bad = ok.copy()
    bad[3] = False
    m = rr.isosurface(ijk, f, bad, 1.0)
    assert m["n_cells_extracted"] == 0 and len(m["vertices"]) == 0 and len(m["triangles"]) == 0
    m = rr.isosurface(ijk[:7], f[:7], ok[:7], 1.0)
    assert m["n_cells_extracted"] == 0 and len(m["vertices"]) == 0


def test_zero_and_negative_zero_are_outside_and_clamp_both_ends():
    g = (0, 1)
    ijk = np.array([(i, j, k) for i in g for j in g for k in g], np.int32)
    f = np.where(ijk[:, 0] == 0, -1.0, 0.0)  # the outside end is exactly 0: t = 1 from the inside origin
    m = rr.isosurface(ijk, f, np.ones(8, bool), 2.0)
    assert len(m["triangles"]) > 0 and (m["vertices"][:, 0] == 2.0).all()
    f = np.where(ijk[:, 0] == 0, -0.0, -3.0)  # -0.0 is outside and the origin: t = -0.0 / 3 = -0.0, kept as it is
    m = rr.isosurface(ijk, f, np.ones(8, bool), 2.0)
    assert len(m["triangles"]) > 0 and (m["vertices"][:, 0] == 0.0).all()


def test_field_of_a_plane_is_the_signed_height():
    rng = np.random.default_rng(2)
    p = np.column_stack([rng.random(600) * 2, rng.random(600) * 2, np.full(600, 0.52)])
    n = np.tile([0.0, 0.0, 1.0], (600, 1))
    fm = rr.field(p, n, 0.25, 0.75, 5, 1)
    z = fm["node_ijk"][:, 2] * 0.25
    v = fm["valid"]
    assert v.sum() > 50
    assert np.abs(fm["f"][v] - (z[v] - 0.52)).max() < 1e-12
    n[::2] = 0.0  # zero normals are skipped and not counted
    fz = rr.field(p, n, 0.25, 0.75, 5, 1)
    assert (fz["k"] <= fm["k"]).all() and fz["k"].sum() < fm["k"].sum()
    assert (fz["node_ijk"] == fm["node_ijk"]).all()
