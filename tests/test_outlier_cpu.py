"""CPU checks of the outlier filters' numpy restatement (tests/_outlier_ref.py) against the O(n^2) definitions — duplicates, n < k,
k = 1, n = 1, ties at the k-th distance, points exactly at the radius — and of the C ABI binding of me_outlier_info."""
import ctypes as C
import math

import numpy as np
import pytest

import _outlier_ref as R


def _clouds():
    rng = np.random.default_rng(11)
    base = rng.random((60, 3))
    g = np.arange(5, dtype=np.float64) * 0.25
    return {
        "random": rng.random((200, 3)),
        "dup": np.concatenate([base, base[:20], np.repeat(base[:1], 8, axis=0)]),
        "n_lt_k": rng.random((9, 3)),
        "n1": rng.random((1, 3)),
        "lattice": np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3),
    }


@pytest.mark.parametrize("name", list(_clouds()))
@pytest.mark.parametrize("k", [1, 2, 7, 20, 40])
def test_sor_avg_equals_brute_force(name, k):
    xyz = _clouds()[name]
    assert np.array_equal(R.sor_avg(xyz, k), R.brute_sor_avg(xyz, k))


def test_sor_consequences():
    c = _clouds()
    avg, keep, _ = R.sor(c["random"], 1, 2.0)
    assert not keep.any() and np.all(avg == 0)  # k = 1: every point's only neighbour is itself
    _, keep, (mean, std, thr) = R.sor(c["n1"], 5, 2.0)
    assert not keep.any() and math.isnan(thr)  # n = 1: std = 0 / 0
    avg, keep, _ = R.sor(c["dup"], 9, 2.0)
    assert np.all(avg[-8:] == 0) and not keep[-8:].any()  # ten copies of one point: all nine neighbours at d2 = 0
    avg, keep, (mean, std, thr) = R.sor(c["random"], 20, 1.0)
    assert mean == np.sum(avg[avg > 0]) / len(avg)  # Open3D divides by every point
    assert np.array_equal(keep, (avg > 0) & (avg < thr))


@pytest.mark.parametrize("name", list(_clouds()))
@pytest.mark.parametrize("radius", [0.05, 0.25, 0.3])
def test_ror_counts_equal_brute_force(name, radius):
    xyz = _clouds()[name]
    assert np.array_equal(R.ror_counts(xyz, radius), R.brute_ror_counts(xyz, radius))


def test_ror_is_strict_at_the_radius():
    xyz = np.stack([np.arange(10) * 0.25, np.zeros(10), np.zeros(10)], 1)  # d2 == 0.0625 == 0.25^2 exactly
    c = R.ror_counts(xyz, 0.25)
    assert np.all(c == 1)
    assert not R.ror(xyz, 1, 0.25)[1].any() and R.ror(xyz, 0, 0.25)[1].all()


def test_outlier_info_binding():
    from cloud_map_evaluation_amd import _lib

    assert C.sizeof(_lib.OutlierInfo) == 48
    assert [f for f, _ in _lib.OutlierInfo._fields_] == ["n_in", "n_kept", "n_fallback", "mean", "std_dev", "threshold"]
    for s in ("me_statistical_outlier", "me_radius_outlier", "me_outlier_select_into"):
        assert s in _lib.SYMBOLS
