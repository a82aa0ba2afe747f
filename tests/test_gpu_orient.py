"""me_orient_normals end to end on the MI355X, on the torus of tests/test_orient_cpu.py — a scene that no single viewpoint sees from
outside: unoriented radius normals are made outward everywhere, and the reconstruction, torn by the bounding-box viewpoint, lies on
the surface once the orientation is propagated."""
import numpy as np
import pytest

import _orient_ref as R
from test_orient_cpu import TORUS_K, TORUS_N, TORUS_SEED

pytestmark = pytest.mark.gpu

NORMAL_RADIUS, H = 0.1, 0.05  # ~24 neighbours per normal at this density; the voxel of the reconstruction


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


@pytest.fixture(scope="module")
def torus():
    xyz, true, _ = R.torus(TORUS_N, TORUS_SEED)
    return xyz, true


def test_torus_radius_normals_become_outward(torus):
    xyz, true = torus
    with _engine() as e:
        e.upload(0, xyz, cell_size=NORMAL_RADIUS)
        e.radius_normals(0, NORMAL_RADIUS, 5, viewpoint=None)
        raw = e.get_normals(0)
        d = e.orient_normals(0, TORUS_K, fetch=True)
        out = e.get_normals(0)
    valid = np.any(raw != 0, axis=1)
    assert d["n_valid"] == valid.sum() > 0.99 * TORUS_N and d["n_inconsistent_edges"] == 0 and d["n_components"] == 1
    assert np.all(R.dot3(out[valid], true[valid]) > 0)
    m = R.orient(xyz, raw, TORUS_K)  # the model on the normals the device had
    assert np.array_equal(d["flipped"], m["flipped"]) and np.array_equal(d["component"], m["component"])
    assert {f: d[f] for f in R.FIELDS} == {f: m[f] for f in R.FIELDS}
    assert out.tobytes() == m["normals"].tobytes()


def test_bounding_box_viewpoint_tears_the_mesh_and_propagation_mends_it(torus):
    xyz, true = torus
    centre = 0.5 * (xyz.min(0) + xyz.max(0))
    with _engine() as e:
        e.upload(0, xyz, cell_size=NORMAL_RADIUS)
        e.radius_normals(0, NORMAL_RADIUS, 5, viewpoint=centre)
        n = e.get_normals(0)
        wrong = np.mean(R.dot3(n, true) < 0)
        print(f"share of inward normals with the bounding-box viewpoint: {wrong:.3f}")
        assert wrong > 0.10  # (the outer half of the tube faces away from the centre)
        torn = e.reconstruct(0, H)
        mended = e.reconstruct(0, H, orient_k=TORUS_K)
        assert np.all(R.dot3(e.get_normals(0), true) >= 0)
    d_torn, d_mended = R.torus_distance(torn["vertices"]), R.torus_distance(mended["vertices"])
    print(f"vertex distance to the torus, voxel {H}: torn max {d_torn.max():.4f}, mended max {d_mended.max():.4f}")
    assert mended["n_triangles"] > 10_000 and d_mended.max() <= H
    assert d_torn.max() > H
