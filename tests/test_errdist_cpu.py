"""The error-distribution metrics without a GPU: the numpy model (tests/_errdist_ref.py) against hand-worked cases, and the library's
host arithmetic (me_fscore_finalize, me_sqrt_threshold, the struct layouts) against the model."""
import ctypes as C
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _errdist_ref as R  # noqa: E402

from cloud_map_evaluation_amd import _lib  # noqa: E402


def test_nearest_rank_at_the_ends_and_where_p_n_is_integral():
    assert R.nearest_rank(0.0, 10) == 0          # ceil(0) - 1 = -1 -> clamped
    assert R.nearest_rank(1.0, 10) == 9
    assert R.nearest_rank(0.5, 10) == 4          # p n = 5 exactly: the 5th smallest
    assert R.nearest_rank(0.5, 11) == 5          # ceil(5.5) - 1
    assert R.nearest_rank(0.25, 8) == 1
    assert R.nearest_rank(0.9, 1) == 0 and R.nearest_rank(0.0, 1) == 0
    assert R.nearest_rank(0.5, 0) == -1
    # 0.1 * 10 rounds to 1.0 in fp64, 0.07 * 100 to 7.000000000000001: the formula is taken as written
    assert R.nearest_rank(0.1, 10) == 0 and R.nearest_rank(0.07, 100) == int(math.ceil(0.07 * 100.0)) - 1 == 7


def test_model_rank_select_by_hand():
    v = np.array([3.0, -0.0, 1.0, 7.0, 1.0, 5.0])
    r = R.rank_select(v, [0, 5, 2, 2, 1])
    assert r["count"] == 6 and r["sum"] == 17.0 and r["min"] == 0.0 and not np.signbit(r["min"]) and r["max"] == 7.0
    assert list(r["value"]) == [0.0, 7.0, 1.0, 1.0, 1.0]
    r = R.rank_select(v, [0, 1], use=[1, 0, 0, 1, 0, 0])
    assert r["count"] == 2 and list(r["value"]) == [3.0, 7.0]
    assert R.rank_select(v, [], use=np.zeros(6))["count"] == 0


def test_threshold_edge_exactly_at_t2max_and_one_ulp_above():
    for t in (0.2, 0.1, 0.08, 0.05, 0.01, 1.0, 0.3):
        x = R.t2max(t)
        assert math.sqrt(x) <= t < math.sqrt(np.nextafter(x, np.inf))
        up = float(np.nextafter(x, np.inf))
        d = R.error_distribution([x, up, 0.0], thresholds=[t], bins=2, bin_width=t)
        assert list(d["n_within"]) == [2]            # 0 and t2max count, one ulp above does not
        assert list(d["hist"]) == [2, 1] and d["n_overflow"] == 0  # ... and falls into the next bin
        d = R.error_distribution([x, up, 0.0], bins=1, bin_width=t)
        assert list(d["hist"]) == [2] and d["n_overflow"] == 1


def test_model_distribution_by_hand():
    d2 = np.array([4.0, 0.25, 9.0, -1.0, 9.0, 1.0])
    d = R.error_distribution(d2, quantiles=[0.0, 0.5, 1.0], thresholds=[1.0, 2.5])
    assert (d["n_query"], d["n_used"], d["argmax"]) == (5, 5, 2)
    assert list(d["rank"]) == [0, 2, 4] and list(d["quantile_d2"]) == [0.25, 4.0, 9.0] and list(d["quantile_d"]) == [0.5, 2.0, 3.0]
    assert (d["min_d"], d["max_d"], d["sum_d"], d["sum_d2"]) == (0.5, 3.0, 9.5, 23.25)
    assert list(d["n_within"]) == [2, 3]
    g = R.error_distribution(d2, quantiles=[0.5], gate=2.0, gate_mode=R.GATE_LT_SQUARED)   # d2 < 4
    assert (g["n_used"], g["argmax"]) == (2, 5) and list(g["quantile_d2"]) == [0.25]
    g = R.error_distribution(d2, quantiles=[0.5], gate=4.0, gate_mode=R.GATE_LE_UNSQUARED)  # d2 <= 4 (the gate is compared as given)
    assert (g["n_used"], g["argmax"]) == (3, 0)
    e = R.error_distribution(d2, quantiles=[0.5], gate=0.0, gate_mode=R.GATE_LT_SQUARED)
    assert (e["n_used"], e["argmax"], list(e["rank"]), list(e["quantile_d2"])) == (0, -1, [-1], [0.0])


def test_fscore_finalize_against_hand_arithmetic():
    L = _lib.load()
    cases = [(30, 40, 10, 20), (0, 40, 0, 20), (5, 0, 3, 10), (5, 10, 3, 0), (0, 0, 0, 0), (7, 7, 9, 9), (1, 3, 2, 7)]
    for a, b, c, d in cases:
        prf = (C.c_double * 3)()
        L.me_fscore_finalize(a, b, c, d, C.byref(prf))
        assert tuple(prf) == R.fscore(a, b, c, d), (a, b, c, d)
    prf = (C.c_double * 3)()
    L.me_fscore_finalize(30, 40, 10, 20, C.byref(prf))
    assert tuple(prf) == (0.75, 0.5, 2 * 0.75 * 0.5 / 1.25)
    L.me_fscore_finalize(5, 0, 3, 10, C.byref(prf))
    assert tuple(prf) == (0.0, 0.3, 0.0)


def test_struct_sizes_follow_the_header():
    assert C.sizeof(_lib.RankStats) == 8 * (4 + 16)
    assert C.sizeof(_lib.ErrDistParams) == 8 + 4 + 4 + 16 * 8 + 8 + 8 * 8 + 8 + 8   # the two lone int32 are padded to 8
    assert C.sizeof(_lib.ErrDistOut) == 8 * (2 + 4 + 1 + 16 + 32 + 8 + 1)
    assert (_lib.ME_RANK_MAX, _lib.ME_ERRDIST_MAX_THRESHOLDS, _lib.ME_ERRDIST_MAX_BINS) == (R.RANK_MAX, R.MAX_THRESHOLDS, R.MAX_BINS)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mapeval_hip.h")).read()
    for name, val in (("ME_RANK_MAX", 16), ("ME_ERRDIST_MAX_THRESHOLDS", 8), ("ME_ERRDIST_MAX_BINS", 4096)):
        assert f"#define {name} {val}\n" in hdr


def test_sqrt_threshold_equals_the_model():
    L = _lib.load()
    rng = np.random.default_rng(17)
    ts = np.concatenate([[0.2, 0.1, 0.08, 0.05, 0.01, 0.0, 1.0, 2.5], rng.random(10_000) * 2.0 ** rng.integers(-30, 12, 10_000)])
    for t in ts:
        assert L.me_sqrt_threshold(float(t)) == R.t2max(float(t)), t
    assert L.me_sqrt_threshold(-1.0) == -1.0 and L.me_sqrt_threshold(float("nan")) == -1.0
