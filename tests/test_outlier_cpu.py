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


_TREE_N = [1, 255, 256, 257, 4097, 256 * 1024 + 1]


@pytest.mark.parametrize("n", _TREE_N)
def test_device_tree_sum_against_fsum(n):
    """Any order of n positive terms is within (n - 1) 2^-53 sum of the exact sum; both passes of the statistics."""
    rng = np.random.default_rng(n)
    v = rng.random(n) + 2.0 ** -20
    for vals in (v, (v - v.mean()) ** 2):
        s, exact = R.device_tree_sum(vals), math.fsum(vals)
        assert abs(s - exact) <= (n - 1) * 2.0 ** -53 * exact, (n, s, exact)
    mean, std, thr = R.sor_stats_device(v, 1.5)
    assert mean == R.device_tree_sum(v) / n
    if n > 1:
        d = v - mean
        assert std == math.sqrt(R.device_tree_sum(d * d) / (n - 1)) and thr == mean + 1.5 * std
        m0, _, _ = R.sor_stats(v, 1.5)  # the serial definition: the same mean up to the summation order
        assert abs(mean - m0) <= (n - 1) * 2.0 ** -53 * m0
    else:
        assert math.isnan(std) and math.isnan(thr)


@pytest.mark.parametrize("n", _TREE_N)
def test_device_tree_sum_exact_on_powers_of_two(n):
    """Powers of two in [1, 2^20]: every partial sum is an integer below 2^53, so every order gives the same bits."""
    rng = np.random.default_rng(1000 + n)
    v = np.ldexp(1.0, rng.integers(0, 21, n))
    assert R.device_tree_sum(v) == math.fsum(v) == float(np.sum(v))
    v[rng.random(n) < 0.3] = 0.0  # entries the kernel skips (avg == 0)
    mean, _, _ = R.sor_stats_device(v, 1.0)
    assert mean == math.fsum(v) / n


def test_sor_launch_shape():
    assert R.sor_launch(1) == (1, 256) and R.sor_launch(256) == (1, 256) and R.sor_launch(257) == (2, 256)
    assert R.sor_launch(256 * 1024) == (1024, 256)
    nb, per = R.sor_launch(256 * 1024 + 1)  # per steps up: the trailing blocks own no point
    assert (nb, per) == (1024, 512) and (256 * 1024 + 1 + per - 1) // per == 513
    assert R.sor_launch(5_000_000) == (1024, 5120)


@pytest.mark.parametrize("n", [2, 64, 1000])
def test_equal_values_give_a_threshold_equal_to_them(n):
    mean, std, thr = R.sor_stats_device(np.full(n, 0.125), 2.0)
    assert (mean, std, thr) == (0.125, 0.0, 0.125)
    assert not R.sor_keep(np.full(n, 0.125), thr).any()  # strict <: equality with the threshold drops the point


def test_brute_force_chunks_agree_with_one_block():
    xyz = np.random.default_rng(5).random((700, 3))  # (more than two chunks of rows)
    d2 = np.sort(R.d2_exact(xyz[:, None, :], xyz[None, :, :]), axis=1)
    for k in (1, 12, 40):
        ref = np.array([sum((math.sqrt(v) for v in row[:k]), 0.0) / k for row in d2])
        assert np.array_equal(R.brute_sor_avg(xyz, k), ref)
    assert np.array_equal(R.brute_ror_counts(xyz, 0.1), np.count_nonzero(d2 < 0.1 * 0.1, axis=1))
    assert np.array_equal(R.brute_sor_avg(xyz[:5], 9), R.brute_sor_avg(xyz[:5], 5))  # n < k: the n points there are


def test_outlier_info_binding():
    from cloud_map_evaluation_amd import _lib

    assert C.sizeof(_lib.OutlierInfo) == 48
    assert [f for f, _ in _lib.OutlierInfo._fields_] == ["n_in", "n_kept", "n_fallback", "mean", "std_dev", "threshold"]
    for s in ("me_statistical_outlier", "me_radius_outlier", "me_outlier_select_into"):
        assert s in _lib.SYMBOLS
