"""me_group_order_stats on the MI355X (csrc/me_mom.hip) against the numpy model (tests/_mom_ref.py).

count, min, max, lower and upper are compared EXACTLY, as bit patterns: they are elements of the input.  The sum is compared within
the derived bound (count - 1) 2^-53 sum, which holds for any order of adding non-negative terms; the model's sum is math.fsum's.
One block of k_gs_stat holds M.TILE = 2048 entries; the block partials are reduced in M.STAGE = 256 chunks, so above TILE * STAGE
entries a chunk holds two partials; k_gs_hist walks M.SLICE = 16 groups per launch and strides above 256 * M.HIST_BLOCKS entries."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mom_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
TWO_LEVEL = M.TILE * M.STAGE + 1  # the first size at which a chunk of the block-order reduction holds more than one partial
GROUPS = [1, 3, 64]
KINDS = ["random", "equal", "low_bit", "top_digit", "zeros", "denormals", "duplicates"]


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    with Engine(0) as e:
        yield e


def _f64(keys) -> np.ndarray:
    return np.asarray(keys, np.uint64).view(np.float64)


def _values(kind: str, n: int, rng) -> np.ndarray:
    if kind == "random":  # magnitudes over many binades, a tenth of the entries repeated
        v = rng.random(n) * 2.0 ** rng.integers(-40, 40, n)
        if n > 4:
            v[rng.integers(0, n, n // 10)] = v[rng.integers(0, n, n // 10)]
        return v
    if kind == "equal":
        return np.full(n, 0.375)
    if kind == "low_bit":  # two values that differ in the lowest key bit: no pass before the last tells them apart
        return np.where(rng.random(n) < 0.5, 1.0, np.nextafter(1.0, 2.0))
    if kind == "top_digit":  # keys that differ only in the top eight bits: the first pass decides everything
        return _f64((rng.integers(0, 0x7E, n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x000123456789AB))  # (below 2^978: the sums stay finite)
    if kind == "zeros":  # +0.0, -0.0 and a few positive values
        return rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 2.0 ** -1074, 1.5]), n)
    if kind == "denormals":
        return _f64(rng.integers(1, 1000, n).astype(np.uint64))
    if kind == "duplicates":  # most entries equal the median value
        return np.where(rng.random(n) < 0.6, 0.5, rng.random(n))
    raise ValueError(kind)


def _check(e, values, groups, n_groups):
    dev = e.group_order_stats(values, groups, n_groups)
    ref = M.order_stats(values, groups, n_groups)
    assert np.array_equal(dev["count"], ref["count"])
    for f in ("min", "max", "lower", "upper", "median"):
        assert np.array_equal(M.bits(dev[f]), M.bits(ref[f])), (f, dev[f], ref[f])
    err, bound = np.abs(dev["sum"] - ref["sum"]), M.sum_bound(ref["count"], ref["sum"])
    assert np.all(err <= bound), (err.max(), bound[np.argmax(err)])
    return dev


@pytest.mark.parametrize("n", SIZES)
def test_every_kind_of_value_at_the_tile_edges(eng, n):
    rng = np.random.default_rng(1000 + n)
    for n_groups in GROUPS:
        for kind in KINDS:
            _check(eng, _values(kind, n, rng), rng.integers(-1, n_groups, n), n_groups)


@pytest.mark.parametrize("n_groups", GROUPS)
def test_second_reduction_level_and_striding_blocks(eng, n_groups):
    n = TWO_LEVEL
    assert n > 256 * M.HIST_BLOCKS
    rng = np.random.default_rng(n_groups)
    dev = _check(eng, _values("random", n, rng), rng.integers(-1, n_groups, n), n_groups)
    assert dev["count"].sum() > n // 2
    # one group holds everything beyond the first tile: its sum crosses every chunk
    g = np.zeros(n, np.int32)
    g[:M.TILE] = rng.integers(-1, n_groups, M.TILE)
    _check(eng, _values("duplicates", n, rng), g, n_groups)


@pytest.mark.parametrize("n", [1, M.TILE - 1, M.TILE, M.TILE + 1, TWO_LEVEL])
def test_sums_are_added_in_the_fixed_order(eng, n):
    """Every group's sum, bit for bit, against M.group_sums_in_order: the eight entries of a thread, the block tree, the STAGE chunk
    blocks (two partials in the first chunk at TWO_LEVEL) and the final block.  The values span 80 binades: another order shows."""
    rng = np.random.default_rng(9000 + n)
    for n_groups in GROUPS:
        v, g = _values("random", n, rng), rng.integers(-1, n_groups, n)
        assert n < 64 or (g == -1).any()
        dev = eng.group_order_stats(v, g, n_groups)
        ref = M.group_sums_in_order(v, g, n_groups)
        assert np.array_equal(dev["count"], np.bincount(g[g >= 0], minlength=n_groups))
        assert np.array_equal(M.bits(dev["sum"]), M.bits(ref)), (n, n_groups, dev["sum"], ref)


def test_group_shapes_empty_single_even_odd_and_all_ignored(eng):
    rng = np.random.default_rng(5)
    counts = {0: 0, 1: 1, 2: 2, 3: 3, 4: 1000, 5: 1001, 7: 64, 8: 65}  # group 6 and 9 .. 11 stay empty too
    g = np.concatenate([np.full(c, k) for k, c in counts.items()] + [np.full(500, -1)])
    g = g[rng.permutation(len(g))]
    dev = _check(eng, rng.random(len(g)), g, 12)
    assert [int(dev["count"][k]) for k in range(12)] == [counts.get(k, 0) for k in range(12)]
    for k in (0, 6, 9, 11):
        assert all(dev[f][k] == 0 and not np.signbit(dev[f][k]) for f in ("sum", "min", "max", "lower", "upper"))
    assert dev["lower"][1] == dev["upper"][1] == dev["min"][1] == dev["max"][1] == dev["sum"][1]
    assert dev["lower"][2] == dev["min"][2] and dev["upper"][2] == dev["max"][2] and dev["lower"][2] != dev["upper"][2]
    dev = _check(eng, rng.random(777), np.full(777, -1), 3)
    assert not dev["count"].any()
    # the value of an ignored entry is not looked at
    dev = _check(eng, np.array([1.0, 2.0, 3.0]), np.array([0, 0, 0]), 1)
    assert eng.group_order_stats([1.0, -5.0, np.nan, 3.0, np.inf], [0, -1, -1, 0, -1], 1)["median"][0] == 2.0


def test_lower_and_upper_straddle_a_digit_boundary(eng):
    """An even count whose two middle keys end one digit and begin the next, at each of the eight digit positions: the two ranks share
    every pass above the boundary and part there."""
    rng = np.random.default_rng(8)
    for p in range(8):
        upper = np.uint64(0x3F5A5A5A5A5A5A5A) & ~np.uint64((1 << (8 * p)) - 1)  # digit p is the last non-zero one: ... 5A 00 .. 00
        lower = upper - np.uint64(1)                                           # ... 59 FF .. FF (p = 0: the neighbour in the last digit)
        below = lower - rng.integers(0, 1000, 40).astype(np.uint64)
        above = upper + rng.integers(0, 1000, 40).astype(np.uint64)
        keys = np.concatenate([below, above, [lower, upper]])
        v = _f64(keys[rng.permutation(len(keys))])
        dev = _check(eng, v, np.zeros(len(v), np.int32), 1)
        assert M.bits(dev["lower"])[0] == lower and M.bits(dev["upper"])[0] == upper
        # the same in the third of three groups, with an odd group beside it
        g = np.concatenate([np.full(len(v), 2), np.full(33, 1)])
        _check(eng, np.concatenate([v, rng.random(33)]), g, 3)


def test_heavy_duplicates_at_the_median(eng):
    rng = np.random.default_rng(11)
    for n_dup, n_lo, n_hi in ((1000, 10, 10), (1000, 499, 501), (1000, 999, 1), (2, 1000, 1000), (1001, 1000, 0)):
        v = np.concatenate([np.full(n_dup, 0.5), rng.random(n_lo) * 0.5, 0.5 + 2.0 ** -53 + rng.random(n_hi)])
        _check(eng, v[rng.permutation(len(v))], np.zeros(len(v), np.int32), 1)


def test_bit_identical_across_calls_and_contexts(eng):
    from cloud_map_evaluation_amd.engine import Engine

    rng = np.random.default_rng(3)
    n = 3 * M.TILE + 17
    v, g = _values("random", n, rng), rng.integers(-1, 5, n)
    a, b = eng.group_order_stats(v, g, 5), eng.group_order_stats(v, g, 5)
    with Engine(0) as other:
        c = other.group_order_stats(v, g, 5)
    for f in ("count", "sum", "min", "max", "lower", "upper"):
        assert a[f].tobytes() == b[f].tobytes() == c[f].tobytes(), f


def test_bad_arguments(eng):
    from cloud_map_evaluation_amd.engine import MapEvalError

    v = np.arange(10, dtype=np.float64)
    for g_bad in (3, -2, 64, 1 << 20, -(1 << 31)):
        g = np.zeros(10, np.int32)
        g[7] = g_bad
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            eng.group_order_stats(v, g, 3)
    for bad in (-1.0, np.nan, np.inf, -np.inf):  # a used value outside the contract
        w = v.copy()
        w[2] = bad
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            eng.group_order_stats(w, np.zeros(10, np.int32), 1)
    for n_groups in (0, 65, -1):
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            eng.group_order_stats(v, np.zeros(10, np.int32), n_groups)
    # the context stays usable
    assert eng.group_order_stats(v, np.zeros(10, np.int32), 1)["median"][0] == 4.5
