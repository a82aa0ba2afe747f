"""me_rank_select on the MI355X (csrc/me_errdist.hip) against the numpy model (tests/_errdist_ref.py).

count, min, max and value[] are compared EXACTLY, as bit patterns: they are elements of the input.  The sum is compared within the
derived bound (count - 1) 2^-53 sum, which holds for any order of adding non-negative terms; the model's sum is math.fsum's.
k_ed_stat gives every entry a thread of its own up to 256 * R.STAT_BLOCKS entries and strides above (four loads in flight above four
times that); the final block adds more than one partial per thread above 256 * R.FINAL_THREADS entries.  A list of at least
R.COMPACT_MIN entries is compacted after a pass in which at most 1 / R.COMPACT_DIV of it carried a live prefix."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _errdist_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
TWO_LEVEL = 256 * R.FINAL_THREADS + 1            # the first size at which a thread of the final block adds two block partials
STRIDED = R.IN_FLIGHT * 256 * R.STAT_BLOCKS + 1  # the first size at which a thread of k_ed_stat takes four loads in flight
COMPACT = R.COMPACT_MIN + 1
KINDS = ["random", "equal", "low_bit", "top_digit", "zeros", "denormals", "duplicates"]


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    with Engine(0) as e:
        yield e


def _f64(keys) -> np.ndarray:
    return np.asarray(keys, np.uint64).view(np.float64)


def _values(kind: str, n: int, rng) -> np.ndarray:  # (the kinds of test_gpu_group_select.py)
    if kind == "random":
        v = rng.random(n) * 2.0 ** rng.integers(-40, 40, n)
        if n > 4:
            v[rng.integers(0, n, n // 10)] = v[rng.integers(0, n, n // 10)]
        return v
    if kind == "equal":
        return np.full(n, 0.375)
    if kind == "low_bit":
        return np.where(rng.random(n) < 0.5, 1.0, np.nextafter(1.0, 2.0))
    if kind == "top_digit":
        return _f64((rng.integers(0, 0x7E, n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x000123456789AB))
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 2.0 ** -1074, 1.5]), n)
    if kind == "denormals":
        return _f64(rng.integers(1, 1000, n).astype(np.uint64))
    if kind == "duplicates":
        return np.where(rng.random(n) < 0.6, 0.5, rng.random(n))
    raise ValueError(kind)


def _rank_sets(count: int, rng):
    if count == 0:
        return [[]]
    sets = [[0], [count - 1], np.full(16, count // 2), rng.integers(0, count, 11)]  # (the last: unsorted, and with repeats once count < 11)
    sets.append(np.array([3, 0, 3, count - 1, 0]) % count)
    sets.append(rng.permutation(count)[:16] if count >= 16 else np.arange(count))  # distinct
    return sets


def _check(e, values, ranks, use=None):
    dev = e.rank_select(values, ranks, use)
    ref = R.rank_select(values, ranks, use)
    assert dev["count"] == ref["count"]
    for f in ("min", "max", "value"):
        assert np.array_equal(R.bits(dev[f]), R.bits(ref[f])), (f, dev[f], ref[f])
    assert abs(dev["sum"] - ref["sum"]) <= R.sum_bound(ref["count"], ref["sum"])
    return dev


def _compactions(e):
    return e.timer("rank_select_compactions")[1], e.timer("rank_select_list")[1]


@pytest.mark.parametrize("n", SIZES)
def test_every_kind_of_value_and_rank_set_at_the_tile_edges(eng, n):
    rng = np.random.default_rng(2000 + n)
    for kind in KINDS:
        v = _values(kind, n, rng)
        for use in (None, rng.random(n) < 0.5):
            count = n if use is None else int(use.sum())
            for ranks in _rank_sets(count, rng):
                _check(eng, v, ranks, use)


def test_use_all_zero_and_a_single_one(eng):
    rng = np.random.default_rng(4)
    v = rng.random(1000)
    dev = _check(eng, v, [], np.zeros(1000, np.uint8))
    assert (dev["count"], dev["sum"], dev["min"], dev["max"]) == (0, 0.0, 0.0, 0.0)
    one = np.zeros(1000, np.uint8)
    one[617] = 7
    dev = _check(eng, v, [0, 0, 0], one)
    assert dev["count"] == 1 and dev["min"] == dev["max"] == dev["sum"] == v[617] and list(dev["value"]) == [v[617]] * 3
    # the value of an unused entry is not looked at
    assert list(eng.rank_select([1.0, -5.0, np.nan, 3.0, np.inf], [1, 0], [1, 0, 0, 1, 0])["value"]) == [3.0, 1.0]


def test_adjacent_ranks_straddle_a_digit_boundary(eng):
    """Two adjacent ranks whose keys end one digit and begin the next, at each of the eight digit positions (position 0: the keys differ
    in the lowest bit): they share a histogram in every pass above the boundary and part there; with 14 more ranks around them."""
    rng = np.random.default_rng(8)
    for p in range(8):
        upper = np.uint64(0x3F5A5A5A5A5A5A5A) & ~np.uint64((1 << (8 * p)) - 1)
        lower = upper - np.uint64(1)
        below = lower - rng.integers(0, 1000, 40).astype(np.uint64)
        above = upper + rng.integers(0, 1000, 40).astype(np.uint64)
        keys = np.concatenate([below, above, [lower, upper]])
        v = _f64(keys[rng.permutation(len(keys))])
        n_below = int((np.sort(keys) < lower).sum())
        assert np.sort(keys)[n_below] == lower and np.sort(keys)[n_below + 1] == upper
        dev = _check(eng, v, [n_below + 1, n_below])
        assert R.bits(dev["value"])[0] == upper and R.bits(dev["value"])[1] == lower
        _check(eng, v, np.concatenate([[n_below, n_below + 1], rng.integers(0, len(v), 14)]))


@pytest.mark.parametrize("n", [TWO_LEVEL, STRIDED])
def test_second_reduction_level_and_striding_blocks(eng, n):
    rng = np.random.default_rng(n)
    for kind, use in (("random", None), ("duplicates", rng.random(n) < 0.7)):
        v = _values(kind, n, rng)
        count = n if use is None else int(use.sum())
        dev = _check(eng, v, rng.integers(0, count, 16), use)
        assert dev["count"] == count


@pytest.mark.parametrize("n", [1, 255, 256, 257, TWO_LEVEL, STRIDED, 2 * STRIDED + 77])
def test_sum_is_added_in_the_fixed_order(eng, n):
    """The sum, bit for bit, against R.rank_select_sum_in_order: the strided walk (2 * STRIDED + 77 runs the unrolled part twice and its
    tail), the block tree and the one-block total over the partials.  The values span 80 binades: another order shows."""
    rng = np.random.default_rng(7000 + n)
    v = _values("random", n, rng)
    for use in (None, rng.random(n) < 0.7):
        dev = eng.rank_select(v, [], use)
        ref = R.rank_select_sum_in_order(v, use)
        assert dev["count"] == (n if use is None else int(use.sum()))
        assert R.bits(dev["sum"])[0] == R.bits(ref)[0], (n, use is not None, dev["sum"], ref)


def test_just_past_the_compaction_trigger(eng):
    """COMPACT_MIN + 1 entries over many binades: after the second pass at the latest fewer than 1 / COMPACT_DIV of them carry the prefix
    of the one rank, and the later passes read a compacted list.  One entry fewer than COMPACT_MIN: never compacted.  Same results."""
    rng = np.random.default_rng(21)
    v = _values("random", COMPACT, rng)
    for ranks in ([COMPACT // 2], [0], [COMPACT - 1], rng.integers(0, COMPACT, 16)):
        _check(eng, v, ranks)
        done, last = _compactions(eng)
        assert done >= 1 and last * R.COMPACT_DIV <= COMPACT, (done, last)
    _check(eng, v[:R.COMPACT_MIN - 1], [1234, 5])
    assert _compactions(eng) == (0, R.COMPACT_MIN - 1)
    # a sparse use mask: the first pass already leaves less than an eighth, and the compacted list drops the use bytes
    use = rng.random(COMPACT) < 0.05
    _check(eng, v, rng.integers(0, int(use.sum()), 16), use)
    assert _compactions(eng) == (1, int(use.sum()))  # (the compacted list is below COMPACT_MIN: it stays)
    # all equal: every entry survives every pass, nothing to compact
    _check(eng, np.full(COMPACT, 0.375), [0, COMPACT - 1, 77])
    assert _compactions(eng) == (0, COMPACT)
    # sixteen ranks spread over the whole range keep sixteen prefixes alive: compaction comes later or leaves a longer list, never wrong
    w = _values("random", 8 * COMPACT, rng)
    _check(eng, w, np.linspace(0, len(w) - 1, 16).astype(np.int64))
    _check(eng, w, [len(w) // 3])
    assert _compactions(eng)[0] >= 1
    # a long list under a sparse use mask is compacted twice: by the mask after the first pass, by the digits later
    big = _values("random", STRIDED, rng)
    use = rng.random(STRIDED) < 0.1
    assert int(use.sum()) >= R.COMPACT_MIN
    _check(eng, big, [int(use.sum()) // 2], use)
    done, last = _compactions(eng)
    assert done >= 2 and last * R.COMPACT_DIV <= int(use.sum())


def test_bit_identical_across_calls_and_contexts(eng):
    from cloud_map_evaluation_amd.engine import Engine

    rng = np.random.default_rng(3)
    n = 3 * COMPACT + 17
    v, use, ranks = _values("random", n, rng), rng.random(n) < 0.8, rng.integers(0, n // 2, 16)
    a, b = eng.rank_select(v, ranks, use), eng.rank_select(v, ranks, use)
    with Engine(0) as other:
        c = other.rank_select(v, ranks, use)
    for f in ("count", "sum", "min", "max", "value"):
        assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes() == np.asarray(c[f]).tobytes(), f


def test_bad_arguments(eng):
    from cloud_map_evaluation_amd.engine import MapEvalError

    v = np.arange(10, dtype=np.float64)
    for ranks in ([10], [0, 3, 10], [-1], [1 << 40]):  # a rank equal to count, beyond it, negative
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            eng.rank_select(v, ranks)
    with pytest.raises(MapEvalError, match=r"^\[-1\]"):
        eng.rank_select(v, [5], np.arange(10) < 5)  # count = 5
    with pytest.raises(MapEvalError, match=r"^\[-1\]"):
        eng.rank_select(v, np.zeros(17, np.int64))  # n_ranks = 17
    with pytest.raises(MapEvalError, match=r"^\[-1\]"):
        eng.rank_select(v, [0], np.zeros(10))       # count == 0 admits no rank
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        w = v.copy()
        w[2] = bad
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            eng.rank_select(w, [0])
    # the context stays usable
    assert list(eng.rank_select(v, [4, 5])["value"]) == [4.0, 5.0]
