"""me_nn_surface_error / me_nn_surface_fetch on the MI355X (csrc/me_surface.hip) against the numpy model (tests/_surface_ref.py).

Given the device's own fetched normals and its bit-exact 1-NN idx / d2, the model is the header's expressions in the same order: e
and c per point are expected BIT-IDENTICAL, every count exact, max_e / argmax exact; the sums agree with math.fsum within
n 2^-52 relative (any summation order of n non-negative terms)."""
import math

import numpy as np
import pytest

import _surface_ref as R

pytestmark = pytest.mark.gpu

_CACHE = {}


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _clouds(n_e, n_g):
    """a noisy wavy sheet sampled twice (N_e != N_g), with normals on both that are NOT unit length in places and zero in others"""
    key = (n_e, n_g)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 + n_e)

        def sheet(n, noise):
            u = rng.uniform(0, 2.0, (n, 2))
            z = 0.05 * np.sin(3 * u[:, 0]) + noise * rng.standard_normal(n)
            return np.ascontiguousarray(np.concatenate([u, z[:, None]], 1))

        def normals(p, zero_every):
            nrm = np.stack([-0.15 * np.cos(3 * p[:, 0]), np.zeros(len(p)), np.ones(len(p))], 1)
            nrm /= np.linalg.norm(nrm, axis=1)[:, None]
            nrm[::3] *= 1.25  # used as stored, not re-normalised
            nrm[::zero_every] = 0.0
            return np.ascontiguousarray(nrm)

        est, gt = sheet(n_e, 0.01), sheet(n_g, 0.002)
        _CACHE[key] = (est, gt, normals(est, 11), normals(gt, 7))
    return _CACHE[key]


def _setup(e, n_e, n_g, query_normals=True):
    est, gt, ne, ng = _clouds(n_e, n_g)
    e.upload(0, est)
    e.upload(1, gt)
    e.set_normals(1, ng)
    if query_normals:
        e.set_normals(0, ne)
    idx, d2 = e.nn1(0, 1)
    return est, gt, (ne if query_normals else None), ng, idx, d2


def _compare(dev, e_dev, c_dev, model, n):
    e_m, c_m, o = model
    assert e_dev.tobytes() == e_m.tobytes(), f"{np.count_nonzero(e_dev != e_m)} plane distances differ"
    assert c_dev.tobytes() == c_m.tobytes(), f"{np.count_nonzero(c_dev != c_m)} cosines differ"
    for key in ("n_query", "n_used", "n_normal_used", "max_e", "argmax"):
        assert dev[key] == o[key], key
    for key in ("n_within", "n_angle"):
        assert np.array_equal(dev[key], o[key]), key
    tol = n * 2.0 ** -52
    for key in ("sum_e", "sum_e2", "sum_t2", "sum_c"):
        assert math.isclose(dev[key], o[key], rel_tol=tol, abs_tol=0.0) or dev[key] == o[key], (key, dev[key], o[key])
    for a, b in zip(dev["sum_e2_within"], o["sum_e2_within"]):
        assert math.isclose(a, b, rel_tol=tol, abs_tol=0.0) or a == b


@pytest.mark.parametrize("n_e,n_g", [(3000, 4097), (1, 257)])
@pytest.mark.parametrize("gate,gate_mode", [(-1.0, 0), (0.0004, 0), (0.02, 1)])
def test_against_the_model(n_e, n_g, gate, gate_mode):
    taus, angs = (0.001, 0.005, 0.02, 0.1), (5.0, 10.0, 20.0)
    with _engine() as e:
        est, gt, ne, ng, idx, d2 = _setup(e, n_e, n_g)
        dev, e_dev, c_dev = e.nn_surface_error(0, taus, angs, gate, gate_mode, fetch=True)
        idx2, d22 = e.nn_fetch(0)
        twice = e.nn_surface_error(0, taus, angs, gate, gate_mode)
    assert np.array_equal(idx, idx2) and d2.tobytes() == d22.tobytes()  # the 1-NN result is left untouched
    assert all(np.array_equal(dev[k], twice[k]) for k in dev)  # bit-identical from run to run
    model = R.surface_error(est, gt, idx, d2, ng, ne, taus, dev["cos_min"], gate, gate_mode)
    _compare(dev, e_dev, c_dev, model, n_e)
    assert dev["cos_min"].tolist() == [math.cos(a * (math.pi / 180.0)) for a in angs]
    if n_e > 1 and gate < 0:
        assert 0 < dev["n_used"] < n_e and 0 < dev["n_normal_used"] < dev["n_used"]  # zero rows on both sides are in play
        zero_ref = np.all(ng[idx] == 0.0, axis=1)
        assert zero_ref.any() and np.all(e_dev[zero_ref] == -1.0) and np.all(e_dev[~zero_ref] >= 0.0)


def test_without_query_normals():
    taus = (0.005, 0.02)
    with _engine() as e:
        est, gt, ne, ng, idx, d2 = _setup(e, 3000, 4097)
        with_n = e.nn_surface_error(0, taus, (10.0,))
    with _engine() as e:
        est, gt, none, ng, idx, d2 = _setup(e, 3000, 4097, query_normals=False)
        dev, e_dev, c_dev = e.nn_surface_error(0, taus, (10.0,), fetch=True)
    assert dev["n_normal_used"] == 0 and dev["sum_c"] == 0.0 and dev["n_angle"].tolist() == [0] and np.all(c_dev == -1.0)
    for key in ("n_used", "sum_e", "sum_e2", "sum_t2", "max_e", "argmax"):
        assert dev[key] == with_n[key], key
    assert np.array_equal(dev["n_within"], with_n["n_within"])
    _compare(dev, e_dev, c_dev, R.surface_error(est, gt, idx, d2, ng, None, taus, dev["cos_min"]), 3000)


def test_thresholds_equal_to_a_value_are_inclusive():
    from cloud_map_evaluation_amd import _lib
    import ctypes as C

    with _engine() as e:
        est, gt, ne, ng, idx, d2 = _setup(e, 3000, 4097)
        _, e_dev, c_dev = e.nn_surface_error(0, fetch=True)
        tau = float(np.sort(e_dev[e_dev >= 0])[1234])
        cm = float(np.sort(c_dev[(c_dev >= 0) & (c_dev <= 1)])[321])
        p = _lib.SurfaceParams()
        p.gate, p.gate_mode, p.n_thresholds, p.n_angles = -1.0, 0, 2, 2
        p.tau[0], p.tau[1] = tau, np.nextafter(tau, 0.0)
        p.cos_min[0], p.cos_min[1] = cm, np.nextafter(cm, 2.0)
        o = _lib.SurfaceOut()
        e._ck(e._L.me_nn_surface_error(e._ctx, 0, C.byref(p), C.byref(o)))
    used, nused = e_dev >= 0, c_dev >= 0
    assert o.n_within[0] == int((used & (e_dev <= tau)).sum()) and o.n_within[0] - o.n_within[1] == int((e_dev == tau).sum()) >= 1
    assert o.n_angle[0] == int((nused & (c_dev >= cm)).sum()) and o.n_angle[0] - o.n_angle[1] == int((c_dev == cm).sum()) >= 1


def test_max_ties_go_to_the_smallest_index():
    gt = np.array([[0.0, 0, 0], [5.0, 0, 0], [10.0, 0, 0]])
    est = np.array([[10.0, 0.25, 0.5], [0.0, 0.1, 0.25], [5.0, -0.25, -0.5], [0.0, 0, -0.5], [5.0, 0.0, 0.125]])
    nrm = np.tile([0.0, 0.0, 1.0], (3, 1))
    with _engine() as e:
        e.upload(0, est)
        e.upload(1, gt)
        e.set_normals(1, nrm)
        idx, d2 = e.nn1(0, 1)
        dev, e_dev, c_dev = e.nn_surface_error(0, (0.25,), fetch=True)
    assert idx.tolist() == [2, 0, 1, 0, 1] and e_dev.tolist() == [0.5, 0.25, 0.5, 0.5, 0.125]  # fetch order = cloud order
    assert (dev["max_e"], dev["argmax"], dev["n_used"], dev["n_within"].tolist()) == (0.5, 0, 5, [2])
    assert dev["sum_e2_within"].tolist() == [0.25 * 0.25 + 0.125 * 0.125] and np.all(c_dev == -1.0)


def test_empty_used_set_and_state_errors():
    from cloud_map_evaluation_amd.engine import MapEvalError

    with _engine() as e:
        est, gt, ne, ng = _clouds(3000, 4097)
        e.upload(0, est)
        e.upload(1, gt)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):  # no 1-NN result
            e.nn_surface_error(0)
        e.nn1(0, 1, fetch=False)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):  # no reference normals
            e.nn_surface_error(0)
        with pytest.raises(MapEvalError, match=r"\[-3\]"):  # nothing to fetch yet
            e.nn_surface_fetch(0)
        e.set_normals(1, np.zeros_like(gt))  # every reference normal is the zero vector: no pair is used
        dev, e_dev, c_dev = e.nn_surface_error(0, (0.01,), (10.0,), fetch=True)
        assert dev["n_query"] == 3000 and np.all(e_dev == -1.0) and np.all(c_dev == -1.0)
        for key in ("n_used", "n_normal_used", "sum_e", "sum_e2", "sum_t2", "sum_c", "max_e"):
            assert dev[key] == 0, key
        assert dev["argmax"] == -1 and dev["n_within"].tolist() == [0] and dev["sum_e2_within"].tolist() == [0.0] and dev["n_angle"].tolist() == [0]
        e.nn1(0, 1, fetch=False)  # a new 1-NN result discards the per-point arrays
        with pytest.raises(MapEvalError, match=r"\[-3\]"):
            e.nn_surface_fetch(0)
        with pytest.raises(MapEvalError, match=r"\[-1\]"):
            e.nn_surface_error(0, (-0.5,))


def test_a_result_without_neighbour_indices_has_no_used_pair():
    """me_set_nn_result places distances only (nn_idx = -1): the kernel's 0 <= j < n_ref guard leaves every pair unused"""
    est, gt, ne, ng = _clouds(3000, 4097)
    with _engine() as e:
        e.upload(0, est)
        e.upload(1, gt)
        e.set_normals(1, ng)
        _, d2 = e.nn1(0, 1)
        e.set_nn_result(0, 1, d2)
        dev, e_dev, c_dev = e.nn_surface_error(0, (0.01,), (10.0,), fetch=True)
    assert dev["n_query"] == 3000 and dev["n_used"] == 0 and dev["argmax"] == -1 and dev["sum_e"] == 0.0
    assert np.all(e_dev == -1.0) and np.all(c_dev == -1.0)


def test_slab_and_shard_modes_are_refused():
    from cloud_map_evaluation_amd.engine import MapEvalError

    est, gt, ne, ng = _clouds(3000, 4097)
    with _engine() as e:
        e.upload(0, est)
        e.upload(1, gt)
        e.set_normals(1, ng)
        e.nn1(0, 1, fetch=False)
        e.set_shard(0, 2)
        for call in (lambda: e.nn_surface_error(0), lambda: e.nn_surface_fetch(0), lambda: e.radius_normals(0, 0.1)):
            with pytest.raises(MapEvalError, match=r"\[-1\]"):
                call()
        e.set_shard(0, 1)
        assert e.nn_surface_error(0)["n_query"] == 3000
    with _engine() as e:
        e.set_slab(0, 0.0, 1.0, 0.1)
        e.upload(0, est)
        for call in (lambda: e.nn_surface_error(0), lambda: e.radius_normals(0, 0.1)):
            with pytest.raises(MapEvalError, match=r"\[-1\]"):
                call()


def test_surface_report_quantiles_and_both_directions():
    taus, probs = (0.005, 0.02), (0.0, 0.5, 0.9, 0.99, 1.0)
    with _engine() as e:
        est, gt, ne, ng = _clouds(3000, 4097)
        e.upload(0, est, cell_size=0.1)
        e.upload(1, gt, cell_size=0.1)
        e.radius_normals(0, 0.1, 5)  # normals first (they may rebuild the index), then the searches
        e.radius_normals(1, 0.1, 5)
        n0, n1 = e.get_normals(0), e.get_normals(1)
        i01, d01 = e.nn1(0, 1)
        i10, d10 = e.nn1(1, 0)
        rep = e.surface_report(taus, (5.0, 10.0, 20.0), probs)
    for name, q, r, idx, d2, nr, nq in (("est", est, gt, i01, d01, n1, n0), ("gt", gt, est, i10, d10, n0, n1)):
        d = rep[name]
        e_m, c_m, o = R.surface_error(q, r, idx, d2, nr, nq, taus, d["cos_min"])
        assert d["n_used"] == o["n_used"] > 0 and np.array_equal(d["n_within"], o["n_within"]) and np.array_equal(d["n_angle"], o["n_angle"])
        srt = np.sort(e_m[e_m >= 0])
        ranks = [R.nearest_rank(p, o["n_used"]) for p in probs]
        assert d["rank"].tolist() == ranks and d["quantile_e"].tolist() == srt[ranks].tolist()
        assert d["quantile_e"][-1] == d["max_e"] == srt[-1]
        assert d["mean_e"] == d["sum_e"] / d["n_used"] and d["rms_e"] == math.sqrt(d["sum_e2"] / d["n_used"])
        assert d["mean_c"] == d["sum_c"] / d["n_normal_used"]
        assert d["plane_rmse"].tolist() == [math.sqrt(s / m) if m else 0.0 for s, m in zip(d["sum_e2_within"], d["n_within"])]
        # the point of the feature: on a sampled surface the distance to the local plane is well below the distance to the nearest sample
        assert d["mean_e"] < 0.8 * float(np.mean(np.sqrt(d2)))
    assert rep["plane_chamfer"] == rep["est"]["mean_e"] + rep["gt"]["mean_e"]
