"""me_mom_select_axes (host arithmetic, no device) against tests/_mom_ref.py, and the model against itself.  No GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mom_ref as M  # noqa: E402

from cloud_map_evaluation_amd import _lib  # noqa: E402
from cloud_map_evaluation_amd.engine import Engine, MapEvalError  # noqa: E402

X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
CP, CO = M.cosines(10.0, 10.0)


def _unit(yaw_deg, pitch_deg=0.0):
    a, b = math.radians(yaw_deg), math.radians(pitch_deg)
    return (math.cos(a) * math.cos(b), math.sin(a) * math.cos(b), math.sin(b))


def _planes(normals, counts):
    return [{"plane": np.array(list(n) + [0.5 * r]), "count": int(c)} for r, (n, c) in enumerate(zip(normals, counts))]


def _both(normals, counts, cp=CP, co=CO, min_pts=100):
    """library == vectorised model == scalar model, exactly; returns the library's answer"""
    dirs, axes = Engine.mom_select_axes(_planes(normals, counts), min_axis_points=min_pts, cos_parallel=cp, cos_orthogonal=co)
    dv, av = M.select_axes(normals, counts, cp, co, min_pts)
    ds, as_ = M.select_axes_scalar(normals, counts, cp, co, min_pts)
    assert np.array_equal(dv, ds) and M.same_axes(av, as_)
    assert np.array_equal(dirs, dv) and M.same_axes(axes, av), (dirs, axes, dv, av)
    return dirs, axes


def _chosen(axes):
    return [a["direction"] for a in axes["axes"]]


def test_scalar_equals_vectorised_on_random_plane_sets():
    rng = np.random.default_rng(7)
    for trial in range(60):
        P = int(rng.integers(0, 25))
        base = rng.normal(size=(4, 3))
        N = base[rng.integers(0, 4, P)] + rng.normal(scale=0.08, size=(P, 3))
        N /= np.linalg.norm(N, axis=1)[:, None] if P else 1.0
        counts = rng.integers(1, 400, P)
        cp, co = M.cosines(float(rng.uniform(2, 30)), float(rng.uniform(2, 30)))
        _both([tuple(n) for n in N], counts, cp, co, int(rng.integers(1, 500)))


def test_box_room_six_planes_three_directions():
    flip = lambda n: tuple(-v for v in n)  # noqa: E731
    dirs, axes = _both([Z, X, flip(Z), Y, flip(X), flip(Y)], [900, 400, 800, 300, 350, 250])
    assert list(dirs) == [0, 1, 0, 2, 1, 2] and axes["n_directions"] == 3 and _chosen(axes) == [0, 1, 2]
    assert [a["weight"] for a in axes["axes"]] == [1700, 750, 550] and [a["n_planes"] for a in axes["axes"]] == [2, 2, 2]
    assert [tuple(a["rep"]) for a in axes["axes"]] == [Z, X, Y]


def test_two_walls_a_floor_and_a_45_degree_plane():
    dirs, axes = _both([Z, _unit(0, 45), X, Y], [1000, 5000, 600, 500])
    # the oblique plane is the largest direction, but orthogonal only to y: the triple wins over any pair with it
    assert list(dirs) == [0, 1, 2, 3] and _chosen(axes) == [0, 2, 3]


def test_only_two_orthogonal_directions():
    dirs, axes = _both([X, _unit(3), Y, _unit(40)], [500, 100, 300, 900])
    assert list(dirs) == [0, 0, 1, 2] and axes["n_axes"] == 2 and _chosen(axes) == [0, 1]
    assert axes["axes"][0]["weight"] == 600 and axes["axes"][0]["n_planes"] == 2


def test_one_plane_and_no_plane():
    dirs, axes = _both([_unit(20, 30)], [150])
    assert list(dirs) == [0] and axes["n_axes"] == 1 and axes["axes"][0]["weight"] == 150
    dirs, axes = _both([_unit(20, 30)], [99])
    assert axes["n_axes"] == 0 and axes["n_directions"] == 1 and axes["axes"] == []
    dirs, axes = _both([], [])
    assert len(dirs) == 0 and axes == {"n_axes": 0, "n_directions": 0, "axes": []}


def test_a_direction_below_min_axis_points_is_not_eligible():
    dirs, axes = _both([X, Y, Z], [500, 99, 400])
    assert _chosen(axes) == [0, 2]
    dirs, axes = _both([X, Y, Z, (0.0, -1.0, 0.0)], [500, 99, 400, 1])  # the second y plane lifts its direction to the bound
    assert list(dirs) == [0, 1, 2, 1] and _chosen(axes) == [0, 1, 2] and axes["axes"][1]["weight"] == 100


def test_min_w_tie_goes_to_the_larger_sum_then_to_the_smaller_tuple():
    # four directions in one plane: (x, y) and the pair rotated by 45 degrees; no triple exists
    N = [X, Y, _unit(45), _unit(135)]
    assert _chosen(_both(N, [100, 500, 100, 700])[1]) == [2, 3]  # min W 100 both, sums 600 < 800
    assert _chosen(_both(N, [100, 500, 100, 500])[1]) == [0, 1]  # full tie: the lexicographically smaller tuple
    assert _chosen(_both(N, [100, 500, 101, 102])[1]) == [2, 3]  # min W decides before the sum
    # single axes: the same rule
    assert _chosen(_both([X, _unit(30)], [200, 200])[1]) == [0]
    assert _chosen(_both([X, _unit(30)], [200, 201])[1]) == [1]


def test_both_thresholds_are_inclusive():
    # dot((1, 0, 0), (a, b, 0)) = (1 * a + 0 * b) + 0 * 0 = a, exactly
    n = (0.6, 0.8, 0.0)
    dirs, _ = _both([X, n], [100, 100], cp=0.6, co=0.1)
    assert list(dirs) == [0, 0]
    dirs, _ = _both([X, n], [100, 100], cp=float(np.nextafter(0.6, 1.0)), co=0.1)
    assert list(dirs) == [0, 1]
    m = (0.25, math.sqrt(1 - 0.0625), 0.0)
    assert _both([X, m], [100, 100], cp=0.9, co=0.25)[1]["n_axes"] == 2
    assert _both([X, m], [100, 100], cp=0.9, co=float(np.nextafter(0.25, 0.0)))[1]["n_axes"] == 1
    # the sign of the normal does not matter: |dot|
    assert list(_both([X, (-0.6, -0.8, 0.0)], [100, 100], cp=0.6, co=0.1)[0]) == [0, 0]
    assert _both([X, (-0.25, m[1], 0.0)], [100, 100], cp=0.9, co=0.25)[1]["n_axes"] == 2


def test_a_plane_joins_the_first_matching_direction_not_the_best():
    cp, co = M.cosines(15.0, 10.0)
    dirs, axes = _both([X, _unit(20), _unit(12)], [100, 100, 100], cp=cp, co=co)
    assert list(dirs) == [0, 1, 0]  # 12 degrees from direction 0, 8 from direction 1
    # ... and the representative stays the founder's normal: a fourth plane 14 degrees past the third does not chain on
    dirs, _ = _both([X, _unit(12), _unit(26)], [100, 100, 100], cp=cp, co=co)
    assert list(dirs) == [0, 0, 1]


def test_argument_errors():
    L = _lib.load()
    recs = (_lib.PlaneRecord * 65)()
    dirs = np.zeros(65, np.int32)
    ax = _lib.MomAxes()

    def call(cp, co, mp, n=1, planes=recs, d=dirs, a=ax):
        prm = _lib.MomParams(cp, co, mp)
        return L.me_mom_select_axes(C.addressof(planes) if planes is not None else 0, n, C.byref(prm), d.ctypes.data if d is not None else 0,
                                    C.byref(a) if a is not None else None)

    assert call(0.9, 0.1, 1) == 0 and call(1.0, 0.0, 1, 64) == 0 and call(0.9, 0.1, 1, 0, None, None) == 0
    for bad in ((0.9, 0.9, 1), (0.1, 0.9, 1), (1.0000001, 0.1, 1), (0.9, -0.1, 1), (0.9, 0.1, 0), (float("nan"), 0.1, 1), (0.9, float("nan"), 1)):
        assert call(*bad) == _lib.ME_ERR_ARG, bad
    assert call(0.9, 0.1, 1, 65) == _lib.ME_ERR_ARG and call(0.9, 0.1, 1, -1) == _lib.ME_ERR_ARG
    assert call(0.9, 0.1, 1, 1, None) == _lib.ME_ERR_ARG and call(0.9, 0.1, 1, 1, recs, None) == _lib.ME_ERR_ARG
    assert call(0.9, 0.1, 1, 1, recs, dirs, None) == _lib.ME_ERR_ARG
    assert L.me_mom_select_axes(C.addressof(recs), 1, None, dirs.ctypes.data, C.byref(ax)) == _lib.ME_ERR_ARG
    with pytest.raises(MapEvalError):
        Engine.mom_select_axes([], parallel_deg=50.0, orthogonal_deg=50.0)


def test_order_statistics_model_on_hand_cases():
    v = np.array([3.0, -0.0, 1.0, 2.0, 0.0, 5.0, 4.0])
    g = np.array([0, 1, 0, 0, 1, -1, 2])
    s = M.order_stats(v, g, 4)
    assert list(s["count"]) == [3, 2, 1, 0] and list(s["lower"]) == [2.0, 0.0, 4.0, 0.0] and list(s["upper"]) == [2.0, 0.0, 4.0, 0.0]
    assert not np.signbit(s["min"][1]) and list(s["sum"]) == [6.0, 0.0, 4.0, 0.0] and list(s["max"]) == [3.0, 0.0, 4.0, 0.0]
    s = M.order_stats([4.0, 1.0, 3.0, 2.0], [0, 0, 0, 0], 1)
    assert (s["lower"][0], s["upper"][0], s["median"][0]) == (2.0, 3.0, 2.5)
    # the key order is the numeric order on non-negative doubles, denormals included
    x = np.abs(np.random.default_rng(1).normal(size=1000)) * 10.0 ** np.random.default_rng(2).integers(-320, 300, 1000).astype(float)
    assert np.array_equal(np.sort(M.keys_of(x)).view(np.float64), np.sort(x))
