"""me_orient_normals on the MI355X at its edges: every output EQUALS the numpy model (tests/_orient_ref.py) — flipped, component and
every me_orient_out field — and the returned normals are bit-equal to +- the input.  The normals go in through set_normals, so that
the model and the device see the same bits."""
import ctypes as C

import numpy as np
import pytest

import _orient_ref as R

pytestmark = pytest.mark.gpu
Z = (0.0, 0.0, 1.0)


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _device(e, xyz, nrm, k, direction=Z, inward=False, slot=0):
    e.upload(slot, xyz)
    e.set_normals(slot, nrm)
    d = e.orient_normals(slot, k, direction, inward, fetch=True)
    d["normals"] = e.get_normals(slot)
    return d


def _equal(d, xyz, nrm, k, direction=Z, inward=False):
    m = R.orient(xyz, nrm, k, direction, inward)
    got = {f: d[f] for f in R.FIELDS}
    assert got == {f: m[f] for f in R.FIELDS}
    assert np.array_equal(d["component"], m["component"]) and d["component"].dtype == np.int32
    assert np.array_equal(d["flipped"], m["flipped"]) and d["flipped"].dtype == np.bool_
    nrm = np.ascontiguousarray(nrm, np.float64)
    assert d["normals"].tobytes() == np.where(m["flipped"][:, None], -nrm, nrm).tobytes()
    return m


def _check(xyz, nrm, k, direction=Z, inward=False):
    with _engine() as e:
        return _equal(_device(e, xyz, nrm, k, direction, inward), xyz, nrm, k, direction, inward)


@pytest.mark.parametrize("n,k", [(1, 3), (2, 3), (3, 1), (3, 5), (7, 7), (8, 7)])
def test_tiny_clouds_and_padded_lists(n, k):  # N = 1, 2, 3; N = k and N = k + 1: the lists are padded with -1
    rng = np.random.default_rng(100 + n)
    m = _check(rng.random((n, 3)), _unit(rng, n), k)
    assert m["n_components"] == 1 and m["n_tree_edges"] == n - 1


@pytest.mark.parametrize("n", [63, 64, 65, 4097])
def test_random_clouds_with_random_normals(n):
    rng = np.random.default_rng(n)
    m = _check(rng.random((n, 3)), _unit(rng, n), 12)
    assert m["n_graph_edges"] > 6 * n


def test_identical_normals_order_by_index_alone():
    rng = np.random.default_rng(7)
    m = _check(rng.random((700, 3)), np.tile([0.6, 0.0, -0.8], (700, 1)), 6)  # every |c| is the same value: (lo, hi) decides
    assert m["n_flipped"] == m["n_valid"] == 700 and m["n_inconsistent_edges"] == 0  # every root points down and is turned, every c > 0


def test_cube_faces_with_axis_normals():  # c is exactly 0 (or -0.0) across the edges of the cube
    rng = np.random.default_rng(8)
    pts, nrm = [], []
    for ax in range(3):
        for side in (0.0, 1.0):
            p = rng.random((150, 3))
            p[:, ax] = side
            v = np.zeros((150, 3))
            v[:, ax] = rng.choice([-1.0, 1.0], 150)
            pts.append(p)
            nrm.append(v)
    xyz, nrm = np.concatenate(pts), np.concatenate(nrm)
    m = _check(xyz, nrm, 10)
    lo, hi, c, _ = R.graph_edges(xyz, nrm, 10)
    assert np.count_nonzero(c == 0) > 50 and m["n_graph_edges"] == len(lo)


@pytest.mark.parametrize("k", [1, 2])
def test_collinear_points_a_tree_as_deep_as_the_cloud(k):
    n = 4097
    xyz = np.stack([np.arange(n) * 0.25, np.zeros(n), np.zeros(n)], axis=1)
    nrm = np.zeros((n, 3))
    nrm[:, 2] = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    m = _check(xyz, nrm, k)
    assert m["n_components"] == 1 and m["n_tree_edges"] == n - 1 and m["n_flipped"] == n // 2
    # the same line with weights that grow along it: every point hooks to its successor in the first round
    t = np.arange(n) * (0.5 * np.pi / n)
    nrm = np.stack([np.sin(t * t), np.zeros(n), np.cos(t * t)], axis=1) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)[:, None]
    _check(xyz, nrm, k)


def test_blocks_of_coincident_points():  # 50 duplicates > k + 1: a point may be missing from its own list
    rng = np.random.default_rng(9)
    xyz = np.repeat(rng.random((20, 3)) * 4.0, 50, axis=0)
    _check(xyz, _unit(rng, 1000), 12)


def test_invalid_normals_take_no_part():
    rng = np.random.default_rng(10)
    n = 2000
    xyz, nrm = rng.random((n, 3)), _unit(rng, n)
    bad = rng.random(n) < 0.1
    nrm[bad] = 0.0
    nrm[np.flatnonzero(bad)[:5]] = -0.0  # (-0.0 is 0)
    with _engine() as e:
        d = _device(e, xyz, nrm, 8)
        m = _equal(d, xyz, nrm, 8)
    assert m["n_valid"] == n - bad.sum() and np.all(d["component"][bad] == -1) and not d["flipped"][bad].any()
    assert d["normals"][bad].tobytes() == nrm[bad].tobytes()


@pytest.mark.parametrize("n_clusters", [2, 64])
def test_well_separated_clusters(n_clusters):
    rng = np.random.default_rng(n_clusters)
    centres = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)[:n_clusters] * 100.0
    xyz = (centres[:, None, :] + rng.random((n_clusters, 40, 3))).reshape(-1, 3)
    perm = rng.permutation(len(xyz))  # components are numbered by their lowest member, not by position in space
    m = _check(xyz[perm], _unit(rng, len(xyz)), 8)
    assert m["n_components"] == n_clusters and m["largest_component"] == 40


def test_root_tie_oblique_direction_and_inward():
    rng = np.random.default_rng(12)
    xyz = rng.random((300, 3))
    xyz[[17, 250], 2] = 5.0  # two points share the top projection: the root is 17
    nrm = _unit(rng, 300)
    m = _check(xyz, nrm, 10)
    assert m["roots"] == [17]
    for direction, inward in (((0.3, -1.7, 0.9), False), ((0.3, -1.7, 0.9), True), (Z, True), ((0.0, -2.0, 0.0), False)):
        _check(xyz, nrm, 10, direction, inward)


@pytest.mark.parametrize("k", [1, 39])
def test_smallest_and_largest_k(k):
    rng = np.random.default_rng(k)
    _check(rng.random((500, 3)), _unit(rng, 500), k)


def test_repeatable_and_idempotent():
    xyz, true, nrm = R.torus(3000, 3)
    outs = []
    with _engine() as e:
        for _ in range(2):
            outs.append(_device(e, xyz, nrm, 12))
        again = e.orient_normals(0, 12, fetch=True)  # on the oriented cloud: nothing left to flip
        assert again["n_flipped"] == 0 and not again["flipped"].any() and again["n_inconsistent_edges"] == outs[0]["n_inconsistent_edges"]
        assert np.array_equal(again["component"], outs[0]["component"])
        assert e.get_normals(0).tobytes() == outs[0]["normals"].tobytes()
    with _engine() as e:
        outs.append(_device(e, xyz, nrm, 12, slot=1))
    for o in outs[1:]:
        assert all(np.asarray(o[k]).tobytes() == np.asarray(outs[0][k]).tobytes() for k in outs[0])
    _equal(outs[0], xyz, nrm, 12)


def test_everything_else_resident_stays():
    rng = np.random.default_rng(13)
    a, b = rng.random((3000, 3)), rng.random((2500, 3))
    with _engine() as e:
        e.upload(0, a, cell_size=0.1)
        e.upload(1, b, cell_size=0.1)
        e.set_normals(0, _unit(rng, 3000))
        e.gicp_covariances(0, 1e-3)
        e.nn1(0, 1, fetch=False)
        e.mme(0, 0.1, 5)
        before = (e.nn_fetch(0), e.mme_fetch(0), e.download(0), e.download(1))
        d = e.orient_normals(0, 12)
        assert d["n_flipped"] > 0
        after = (e.nn_fetch(0), e.mme_fetch(0), e.download(0), e.download(1))
        for x, y in zip(before, after):
            xs, ys = (x, y) if isinstance(x, tuple) else ((x,), (y,))
            assert all(p.tobytes() == q.tobytes() for p, q in zip(xs, ys))
        from cloud_map_evaluation_amd.engine import MapEvalError

        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.get_covariances(0)  # made from the old normals: dropped, as set_normals drops them
        assert e.orient_fetch(0)["flipped"].sum() == d["n_flipped"]


def test_errors():
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import MapEvalError

    rng = np.random.default_rng(14)
    p, n = rng.random((100, 3)), _unit(rng, 100)

    def fails(code, fn, *a, **kw):
        with pytest.raises(MapEvalError, match=rf"\[{code}\]"):
            fn(*a, **kw)

    ARG, STATE = -1, -3
    with _engine() as e:
        fails(STATE, e.orient_normals, 0)  # no cloud
        fails(STATE, e.orient_fetch, 0)
        e.upload(0, p)
        fails(STATE, e.orient_normals, 0)  # no normals
        e.set_normals(0, n)
        fails(STATE, e.orient_fetch, 0)  # no result yet
        for slot in (-1, 2):
            fails(ARG, e.orient_normals, slot)
            fails(ARG, e.orient_fetch, slot)
        for k in (0, -1, 40):
            fails(ARG, e.orient_normals, 0, k)
        for d in ((0.0, 0.0, 0.0), (0.0, -0.0, 0.0), (float("nan"), 0.0, 1.0), (0.0, float("inf"), 1.0)):
            fails(ARG, e.orient_normals, 0, 12, d)
        prm, out = _lib.OrientParams(), _lib.OrientOut()
        prm.direction[2], prm.k = 1.0, 12
        assert e._L.me_orient_normals(e._ctx, 0, None, C.byref(out)) == ARG
        assert e._L.me_orient_normals(e._ctx, 0, C.byref(prm), None) == ARG
        assert e._L.me_orient_normals(e._ctx, 0, C.byref(prm), C.byref(out)) == 0 and out.n == 100 and out.n_valid == 100
        assert e.orient_fetch(0)["component"].shape == (100,)
        e.set_normals(0, n)  # the normals are replaced: the result is gone
        fails(STATE, e.orient_fetch, 0)
        e.orient_normals(0, 5)
        e.upload(0, p)  # the points are replaced
        fails(STATE, e.orient_fetch, 0)
        e.set_normals(0, n)
        e.set_shard(0, 2)
        fails(ARG, e.orient_normals, 0)
        e.set_shard(0, 1)
        assert e.orient_normals(0)["n"] == 100
    with _engine() as e:
        e.set_slab(0, 0.0, 0.5, 0.1)
        e.upload(0, p)
        fails(ARG, e.orient_normals, 0)
