"""me_voxel_deformation without a GPU: the numpy model of pass 3 (tests/_deform_ref.py) against an independent Kabsch fit and the
residuals summed over the points; the entry points are declared, exported and bound."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import _deform_ref as ref  # noqa: E402
from _globreg_ref import rotation  # noqa: E402

VS = 1.0


def _voxel(seed: int, n: int = 120, noise: float = 0.0):
    """n well-spread points of the voxel (0, 0, 0), moved by a small rigid motion (+ noise): a, b about the voxel centre."""
    rng = np.random.default_rng(seed)
    p = 0.05 + 0.9 * rng.random((n, 3))
    R0 = rotation(*(math.radians(x) for x in rng.uniform(-2.0, 2.0, 3)))
    q = (p - 0.5) @ R0.T + 0.5 + rng.uniform(-0.01, 0.01, 3) + noise * rng.standard_normal((n, 3))
    return p, q, R0


def _model(p, q, min_pairs=30, min_spread=VS / 20):
    d2 = ((p - q) ** 2).sum(1)
    s = ref.voxel_sums(p, q, d2, np.ones(len(p), bool), VS)
    assert len(s["keys"]) == 1 and s["n_pairs"][0] == len(p)
    return s, ref.fit(len(p), s["sums"][0], min_pairs, min_spread)


@pytest.mark.parametrize("seed", range(8))
def test_model_rotation_against_kabsch(seed):
    p, q, R0 = _voxel(seed, noise=0.002)
    s, (fl, t0, u, R, e0, et, eR) = _model(p, q)
    assert fl == ref.FIT | ref.ROT_OK
    K = ref.kabsch(p - 0.5, q - 0.5)
    assert np.abs(np.reshape(R, (3, 3)) - K).max() <= 1e-9
    # u = bbar - R abar, the fit's displacement at the voxel centre
    a, b = p - 0.5, q - 0.5
    assert np.abs(np.array(u) - (b.mean(0) - K @ a.mean(0))).max() <= 1e-9
    assert np.abs(np.array(t0) - (b.mean(0) - a.mean(0))).max() <= 1e-12


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("noise", [0.0, 0.003])
def test_residuals_from_moments_against_the_points(seed, noise):
    p, q, _ = _voxel(100 + seed, noise=noise)
    n = len(p)
    s, (fl, t0, u, R, e0, et, eR) = _model(p, q)
    a, b = p - 0.5, q - 0.5
    dt, dR = ref.direct_residuals(a, b, R)
    bound = 64 * n * 2.0 ** -53 * (1.5 * VS + 0.1) ** 2  # the bound the GPU tests hold the device to (max_distance 0.1 here)
    assert abs(et - dt) <= bound and abs(eR - dR) <= bound
    assert abs(e0 - math.fsum(((p - q) ** 2).sum(1).tolist())) <= n * 2.0 ** -52 * e0
    assert eR <= et + bound <= e0 + 2 * bound  # a rigid fit explains at least what its translation does
    if noise == 0.0:
        assert eR <= bound  # an exact rigid motion leaves nothing


def test_flags_and_degenerate_sources():
    rng = np.random.default_rng(3)
    line = 0.5 + np.outer(np.linspace(-0.4, 0.4, 40), [1.0, 0.5, 0.25])
    for p in (line, np.full((40, 3), 0.25)):
        q = p + [0.001, 0.0, 0.002]
        _, (fl, t0, u, R, e0, et, eR) = _model(p, q)
        assert fl == ref.FIT and R == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0] and u == t0 and eR == et
    p = 0.1 + 0.8 * rng.random((29, 3))
    _, (fl, *_rest) = _model(p, p + 0.001)
    assert fl == 0
    p = 0.1 + 0.8 * rng.random((30, 3))
    _, (fl, *_rest) = _model(p, p + 0.001)
    assert fl == ref.FIT | ref.ROT_OK
    assert ref.fit(0, np.zeros(23), 30, 0.05) == (0, [0.0] * 3, [0.0] * 3, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], 0.0, 0.0, 0.0)


def test_pair_predicate():
    d2 = np.array([-1.0, 0.0, 0.25, np.nextafter(0.25, 0.0), 0.2, 0.2, np.nan])
    idx = np.array([0, 1, 2, 3, -1, 5, 0])
    assert ref.pair_mask(d2, idx, 5, 0.5).tolist() == [False, True, False, True, False, False, False]
    assert ref.pair_mask(d2, idx, 6, math.inf).tolist() == [False, True, True, True, False, True, False]


def test_totals_in_order_equal_plain_sums_to_rounding():
    rng = np.random.default_rng(5)
    V = 700
    n = rng.integers(0, 90, V)
    fl = np.where(n >= 30, ref.FIT | ref.ROT_OK, 0).astype(np.uint8)
    t0 = 0.01 * rng.standard_normal((V, 3))
    e0, et, eR = rng.random(V), 0.5 * rng.random(V), 0.25 * rng.random(V)
    t = ref.totals(n, fl, t0, e0, et, eR)
    assert t["n_pairs"] == n.sum() and t["n_fit"] == (n >= 30).sum() and t["n_with_pairs"] == (n > 0).sum()
    assert math.isclose(t["sum_e0"], math.fsum(e0), rel_tol=1e-13)
    assert math.isclose(t["sum_e_R"], math.fsum(eR[n >= 30]), rel_tol=1e-13)
    tn = np.linalg.norm(t0, axis=1)
    assert math.isclose(t["sum_n_t0"], math.fsum(n * tn), rel_tol=1e-13)
    assert t["max_row"] == int(np.argmax(np.where(n >= 30, tn, -1.0)))


def test_entry_points_are_declared_exported_and_bound():
    """fails on a tree without the feature"""
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import Engine

    hdr = open(os.path.join(ROOT, "include", "mapeval_hip.h")).read()
    assert "int me_voxel_deformation(me_ctx *ctx, int query_slot, double voxel_size, double max_distance, int min_pairs, double min_spread," in hdr
    assert "int me_voxel_deformation_fetch(me_ctx *ctx, int query_slot," in hdr
    for s in ("me_voxel_deformation", "me_voxel_deformation_fetch"):
        assert s in _lib.SYMBOLS
    L = _lib.load()
    assert L.me_voxel_deformation.restype is ctypes.c_int and len(L.me_voxel_deformation.argtypes) == 7
    assert L.me_voxel_deformation_fetch.restype is ctypes.c_int and len(L.me_voxel_deformation_fetch.argtypes) == 11
    assert ctypes.sizeof(_lib.DeformSummary) == 8 * 6 + 16 + 8 * 7
    assert callable(getattr(Engine, "deformation_field", None)) and callable(getattr(Engine, "deformation_fetch", None))


def test_rotation_angle_is_the_documented_formula():
    from cloud_map_evaluation_amd.engine import rotation_angle

    for deg in (0.0, 0.2, 30.0, 179.0):
        R = rotation(math.radians(deg))
        assert abs(float(rotation_angle(R.reshape(1, 9))[0]) - math.radians(deg)) <= 1e-12
    assert rotation_angle(np.eye(3).reshape(1, 9))[0] == 0.0
