"""me_mom / me_mom_fetch on the MI355X (csrc/me_mom.hip) against the numpy model (tests/_mom_ref.py).

(a) The model fed the device's OWN fetched inputs — the eigenvalues and validity bytes of me_local_geometry, the labels and records
    of me_segment_planes: everything integer, the axis bytes, min / max / lower / upper / median and mom_median are exact; the sums lie
    within (count - 1) 2^-53 sum.
(b) End to end against the pure numpy pipeline (_plane_ref.segment + _localgeom_ref.local_geometry): labels and axes exact, each axis
    median within 8 k_max 2^-53 r^2 — the device's eigenvalue bound (_localgeom_ref.eig_bound) at the largest neighbour count of the
    contributing points: a median moves by at most the largest per-point change when the contributing set is the same, and the test
    asserts that it is (no l1 inside the bound, equal validity).
(c) State handling, (d) zero, one and two axes, and an axis without a valid point."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _globreg_ref as G  # noqa: E402
import _localgeom_ref as L  # noqa: E402
import _mom_ref as M  # noqa: E402
import _plane_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

RADIUS, MIN_K = 1.5, 5
PLANE = dict(distance_threshold=0.06, num_iterations=300, max_planes=8, min_inliers=150, refit=True, seed=4)
CP, CO = M.cosines(10.0, 10.0)
INT_FIELDS = ("direction", "n_planes", "n_points", "n_valid")
EXACT_FIELDS = ("min", "max", "lower", "upper", "median")


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


_cache = {}


def _scene(kind: str) -> np.ndarray:
    if kind not in _cache:
        if kind == "planes":
            p = G.three_planes(1400, seed=5)
            p = np.ascontiguousarray(p[np.random.default_rng(9).permutation(len(p))][:4099])
        else:
            p = M.box_room(600, 8.0, seed=3)
        p.setflags(write=False)
        _cache[kind] = p
    return _cache[kind]


def _same(dev, model):
    assert (dev["n_axes"], dev["n_directions"]) == (model["n_axes"], model["n_directions"])
    for d, m in zip(dev["axes"], model["axes"]):
        assert [d[f] for f in INT_FIELDS] == [m[f] for f in INT_FIELDS]
        assert np.array_equal(d["rep"], m["rep"])
        for f in EXACT_FIELDS:
            assert M.bits(d[f]) == M.bits(m[f]), (f, d[f], m[f])
        assert abs(d["sum_l3"] - m["sum_l3"]) <= M.sum_bound(m["n_valid"], m["sum_l3"])
    assert M.bits(dev["mom_median"]) == M.bits(model["mom_median"])
    mean_bound = sum(M.sum_bound(m["n_valid"], m["sum_l3"]) / max(1, m["n_valid"]) + 2 * M.EPS * m["sum_l3"] / max(1, m["n_valid"])
                     for m in model["axes"])
    assert abs(dev["mom_mean"] - model["mom_mean"]) <= mean_bound + len(model["axes"]) * M.EPS * model["mom_mean"]


def _model_from_device(e, slot, min_axis_points):
    _, eig, k, valid = e.local_geometry(slot, RADIUS, MIN_K, fetch=True)
    planes, labels = e.plane_fetch(slot)
    return M.mom(eig[:, 2], valid, labels, planes, CP, CO, min_axis_points), (eig, k, valid, planes, labels)


@pytest.mark.parametrize("kind,want_axes", [("planes", 3), ("box", 3)])
def test_exact_against_the_model_on_the_devices_own_inputs(kind, want_axes):
    xyz = _scene(kind)
    with _engine() as e:
        e.upload(0, xyz)
        e.segment_planes(0, **PLANE)
        (model, axis_m), (eig, k, valid, planes, labels) = _model_from_device(e, 0, 100)
        dev, axis = e.mom(0, min_axis_points=100, fetch=True)
    assert model["n_axes"] == want_axes and all(a["n_valid"] > 100 for a in model["axes"])
    if kind == "box":  # seven planes, four directions: the oblique one is orthogonal to one wall pair only and is left out
        assert len(planes) == 7 and model["n_directions"] == 4 and all(a["n_planes"] == 2 for a in model["axes"])
    _same(dev, model)
    assert axis.dtype == np.int8 and np.array_equal(axis, axis_m)
    # the axis byte says exactly which points were used
    for a, d in enumerate(dev["axes"]):
        assert int((axis == a).sum()) == d["n_valid"] <= d["n_points"]
    assert dev["mom_median"] == sum(d["median"] for d in dev["axes"]) and all(d["median"] == (d["lower"] + d["upper"]) / 2 for d in dev["axes"])


def test_end_to_end_against_the_numpy_pipeline():
    xyz = _scene("planes")
    t, H, P, min_inl, seed = 0.06, 300, 4, 150, 4
    seg = R.segment(xyz, t, H, P, min_inl, seed)
    eig_m, k_m, valid_m = L.local_geometry(xyz, RADIUS, MIN_K)
    with _engine() as e:
        e.upload(0, xyz)
        info, planes, labels, _ = e.segment_planes(0, t, H, P, min_inl, refit=False, seed=seed, fetch=True)
        _, eig, k, valid = e.local_geometry(0, RADIUS, MIN_K, fetch=True)
        dev, axis = e.mom(0, min_axis_points=100, fetch=True)
    assert np.array_equal(labels, seg["labels"]) and len(planes) == len(seg["records"]) == 3
    assert all(np.array_equal(p["plane"], m["plane"]) and p["count"] == m["count"] for p, m in zip(planes, seg["records"]))
    # the contributing set is the same: equal neighbour counts, no l1 inside the eigenvalue bound, hence equal validity
    assert np.array_equal(k, k_m)
    assert not np.any((k_m >= MIN_K) & (eig_m[:, 0] <= L.eig_bound(k_m, RADIUS)))
    assert np.array_equal(valid.astype(bool), valid_m)
    model, axis_m = M.mom(eig_m[:, 2], valid_m, seg["labels"], seg["records"], CP, CO, 100)
    assert np.array_equal(axis, axis_m) and dev["n_axes"] == model["n_axes"] == 3
    for a, (d, m) in enumerate(zip(dev["axes"], model["axes"])):
        assert [d[f] for f in INT_FIELDS] == [m[f] for f in INT_FIELDS] and np.array_equal(d["rep"], m["rep"])
        bound = float(L.eig_bound(k_m[axis_m == a].max(), RADIUS))
        print(f"axis {a}: median {d['median']:.17g} model {m['median']:.17g} diff {abs(d['median'] - m['median']):.3g} bound {bound:.3g}")
        assert abs(d["median"] - m["median"]) <= bound
    assert abs(dev["mom_median"] - model["mom_median"]) <= 3 * float(L.eig_bound(k_m[axis_m >= 0].max(), RADIUS))


def test_state_handling():
    from cloud_map_evaluation_amd.engine import MapEvalError

    xyz = _scene("planes")
    with _engine() as e:
        e.upload(0, xyz)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e.mom(0)
        e.local_geometry(0, RADIUS, MIN_K)
        with pytest.raises(MapEvalError, match=r"^\[-3\].*plane"):
            e.mom(0)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e._ck(e._L.me_mom_fetch(e._ctx, 0, 0))
        e.upload(0, xyz)
        e.segment_planes(0, **PLANE)
        with pytest.raises(MapEvalError, match=r"^\[-3\].*eigenvalues"):
            e.mom(0)
        # local geometry after the planes ...
        e.local_geometry(0, RADIUS, MIN_K)
        a, axis_a = e.mom(0, min_axis_points=100, fetch=True)
        # ... and the planes after local geometry: the same output
        e.upload(1, xyz)
        e.local_geometry(1, RADIUS, MIN_K)
        e.segment_planes(1, **PLANE)
        b, axis_b = e.mom(1, min_axis_points=100, fetch=True)
        assert a["n_axes"] == 3 and np.array_equal(axis_a, axis_b)
        _same(a, b)
        assert all(x["sum_l3"] == y["sum_l3"] for x, y in zip(a["axes"], b["axes"])) and a["mom_mean"] == b["mom_mean"]
        # Engine.mom runs a missing stage when it has its arguments, and only then
        e.upload(1, xyz)
        c = e.mom(1, radius=RADIUS, min_k=MIN_K, min_axis_points=100, plane_kwargs=PLANE)
        _same(c, a)
        e.timers_enable(True)
        e.timers_reset()
        _same(e.mom(1, radius=RADIUS, min_k=MIN_K, min_axis_points=100, plane_kwargs=PLANE), a)
        assert e.timer("local_geom")[1] == 0 and e.timer("plane_score")[1] == 0 and e.timer("group_select")[1] > 0 and e.timer("mom")[1] > 0
        e.timers_enable(False)
        # a later segment_planes with other parameters changes the result accordingly, and drops the axis bytes until me_mom runs again
        e.segment_planes(0, 0.06, 300, 2, 150, refit=True, seed=4)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e._ck(e._L.me_mom_fetch(e._ctx, 0, 0))
        (model, axis_m), _ = _model_from_device(e, 0, 100)
        two, axis_two = e.mom(0, min_axis_points=100, fetch=True)
        assert two["n_axes"] == 2 and np.array_equal(axis_two, axis_m)
        _same(two, model)
        # a later local_geometry drops them too
        e.local_geometry(0, RADIUS, MIN_K + 1)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e._ck(e._L.me_mom_fetch(e._ctx, 0, 0))
        e.mom(0, min_axis_points=100)
        # a transform discards both inputs
        T = np.eye(4)
        T[0, 3] = 0.25
        e.transform_cloud(0, T)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e.mom(0)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e._ck(e._L.me_mom_fetch(e._ctx, 0, 0))
        # bad parameters
        for kw in (dict(parallel_deg=50.0, orthogonal_deg=50.0), dict(min_axis_points=0), dict(orthogonal_deg=-1.0), dict(parallel_deg=91.0)):
            with pytest.raises(MapEvalError, match=r"^\[-1\]"):
                e.mom(1, **kw)


def test_zero_one_and_two_axes_and_an_axis_without_a_valid_point():
    full = _scene("planes")
    rng = np.random.default_rng(2)
    line = np.zeros((300, 3))
    line[:, 0] = np.round(rng.uniform(0, 17, 300) * 256) / 256
    with _engine() as e:
        # no plane at all: collinear points
        e.upload(0, line)
        e.local_geometry(0, RADIUS, MIN_K)
        info, planes = e.segment_planes(0, **PLANE)
        assert info["n_planes"] == 0
        res, axis = e.mom(0, min_axis_points=100, fetch=True)
        assert (res["n_axes"], res["n_directions"], res["mom_median"], res["mom_mean"], res["axes"]) == (0, 0, 0.0, 0.0, []) and np.all(axis == -1)
        # planes, but no direction with enough points
        e.upload(0, full)
        e.local_geometry(0, RADIUS, MIN_K)
        e.segment_planes(0, **PLANE)
        res, axis = e.mom(0, min_axis_points=10_000, fetch=True)
        assert res["n_axes"] == 0 and res["n_directions"] == 3 and res["mom_median"] == 0.0 and np.all(axis == -1)
        # one and two planes
        for max_planes in (1, 2):
            e.segment_planes(0, **dict(PLANE, max_planes=max_planes))
            (model, axis_m), _ = _model_from_device(e, 0, 100)
            res, axis = e.mom(0, min_axis_points=100, fetch=True)
            assert res["n_axes"] == max_planes and np.array_equal(axis, axis_m)
            _same(res, model)
        # no point has min_k neighbours: two axes, neither with a valid point
        e.local_geometry(0, RADIUS, 100_000)
        res, axis = e.mom(0, min_axis_points=100, fetch=True)
        assert res["n_axes"] == 2 and np.all(axis == -1) and res["mom_median"] == 0.0 and res["mom_mean"] == 0.0
        for d in res["axes"]:
            assert d["n_valid"] == 0 and d["n_points"] > 1000 and all(d[f] == 0.0 for f in EXACT_FIELDS + ("sum_l3",))
