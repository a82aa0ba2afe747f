"""k_scs, k_hash_insert_keys, k_pack_keys and k_sum_masked through me_scs_table on the MI355X against the 50-digit model of
tests/_vmd_ref.py: |scs_dev - scs_model| <= _vmd_ref.scs_bound (derived there), NaN where the model is NaN, ME_ERR_ARG where the header
refuses."""
import numpy as np
import pytest

import _vmd_ref as V

pytestmark = pytest.mark.gpu

RADII = (1, 2, 5, 9, 10)
LIM = 2 ** 20 - 16  # |index| < LIM is accepted


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _check(e, keys, w, r, model=None):
    s, per, n_max = model if model is not None else V.scs(keys, w, r)
    got = e.scs_table(keys, w, r)
    if np.isnan(s) or np.isinf(s):
        assert (np.isnan(got) and np.isnan(s)) or got == s
        return got, 0.0
    bound = V.scs_bound(n_max, len(w), r, per)
    print(f"M={len(w)} r={r} N={n_max}: scs={s:.9f} off {abs(got - s) / V.U:.1f} u of {bound / V.U:.0f} u")
    assert abs(got - s) <= bound
    return got, bound


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("name", ["dense5", "slab9", "sparse700"])
def test_every_radius_on_a_dense_block_a_slab_and_a_sparse_table(name, r):
    """Radius 1 leaves 37 of the 64 lanes without a stencil cell; radius 10 asks for 21^3 * 8 = 74,088 bytes of dynamic LDS per block: the
    call answers with the model's value or with an error code, never ME_OK and another value."""
    from cloud_map_evaluation_amd.engine import MapEvalError

    keys, w = V.scs_tables()[name]
    assert keys.min() < 0 < keys.max()
    with _engine() as e:
        try:
            got, _ = _check(e, keys, w, r, V.scs_model(name, r))
        except MapEvalError as exc:
            assert r == 10 and str(exc).startswith("[-2]"), exc  # only the largest stencil's launch may be refused, and as ME_ERR_HIP
            print(f"radius 10 refused: {exc}")
            return
        assert e.scs_table(keys, w, r) == got  # two calls: the same value


@pytest.mark.parametrize("r", [1, 5, 10])
def test_neighbour_geometry_at_exactly_the_radius(r):
    w2 = np.array([0.25, 0.75])
    with _engine() as e:
        for axis in range(3):
            far = np.zeros((2, 3), np.int32)
            far[0] = (-3, 7, -11)
            far[1] = far[0]
            far[1, axis] += r  # exactly the radius apart on one axis: neighbours, one each, population std 0
            assert _check(e, far, w2, r)[0] == 0.0
            far[1, axis] += 1  # radius + 1: none
            assert np.isnan(_check(e, far, w2, r)[0])
        diag = np.array([(2, -4, 6), (2 - r, -4 + r, 6 - r)], np.int32)  # the corner of the cube
        assert _check(e, diag, w2, r)[0] == 0.0
        assert np.isnan(_check(e, diag[:1], w2[:1], r)[0])  # one voxel alone
        assert np.isnan(e.scs_table(np.zeros((0, 3), np.int32), np.zeros(0), r))  # n = 0
        three = np.array([(0, 0, 0), (r, 0, 0), (-r, r, -r), (2 * r + 1, 0, 0)], np.int32)  # the last sees nobody and is left out
        _check(e, three, np.array([0.5, 1.5, 1.0, 9.0]), r)


@pytest.mark.parametrize("m", [1, 2, 32, 33, 255, 256, 257])
def test_table_sizes_at_the_hash_and_block_edges(m):
    keys, w = V.scs_tables()[f"size{m}"]
    with _engine() as e:
        _check(e, keys, w, 2, V.scs_model(f"size{m}", 2))


def test_values_of_w():
    keys, w = V.scs_tables()["dense5"]
    with _engine() as e:
        got, bound = _check(e, keys, np.full(len(w), 0.37), 2)  # all equal: 0 within the bound (the mean's rounding is all there is)
        assert 0.0 <= got <= bound
        assert np.isnan(_check(e, keys, np.zeros(len(w)), 2)[0])  # all zero: 0 / 0 in every voxel, as the model
        huge = w.copy()
        huge[17] = 1e100
        _check(e, keys, huge, 2)
        centre = w.copy()
        centre[np.flatnonzero((keys == 0).all(axis=1))[0]] = 0.0  # a zero W is a value like any other (only w < 0 means "absent" in LDS)
        _check(e, keys, centre, 1)
        two = np.array([(0, 0, 0), (1, 0, 0), (40, 0, 0), (41, 0, 0)], np.int32)  # a voxel whose only neighbour has W = 0: 0 / 0, NaN
        assert np.isnan(_check(e, two, np.array([0.0, 1.0, 2.0, 3.0]), 1)[0])


def test_key_bounds():
    from cloud_map_evaluation_amd.engine import MapEvalError

    hi = LIM - 1  # 2^20 - 17: accepted; the stencil of radius 10 reaches 2^20 - 7, still a valid index, and finds nothing there
    keys = np.array([(hi, hi, hi), (hi - 10, hi, hi - 3), (-hi, -hi, -hi), (-hi + 1, -hi + 10, -hi), (hi, -hi, 0), (hi - 1, -hi + 1, 1),
                     (0, 0, 0)], np.int32)
    w = np.array([0.3, 0.9, 0.2, 0.5, 0.7, 0.8, 0.4])
    with _engine() as e:
        for r in (1, 10):
            _check(e, keys, w, r)
        for bad in (LIM, -LIM, 2 ** 20, -(2 ** 20), 2 ** 21 + 5, np.iinfo(np.int32).max, np.iinfo(np.int32).min):
            for axis in range(3):
                k = keys.copy()
                k[3, axis] = bad
                with pytest.raises(MapEvalError, match=r"^\[-1\]"):
                    e.scs_table(k, w, 1)
        _check(e, keys, w, 1)  # the context is usable after a refusal


def test_radius_argument():
    from cloud_map_evaluation_amd.engine import MapEvalError

    keys, w = V.scs_tables()["size32"]
    with _engine() as e:
        for r in (0, 11, -1):
            with pytest.raises(MapEvalError, match=r"^\[-1\]"):
                e.scs_table(keys, w, r)


def test_row_order_does_not_matter_beyond_the_bound():
    keys, w = V.scs_tables()["sparse700"]
    s, per, n_max = V.scs_model("sparse700", 5)
    bound = V.scs_bound(n_max, len(w), 5, per)
    rng = np.random.default_rng(11)
    with _engine() as e:
        for _ in range(3):
            p = rng.permutation(len(w))
            assert abs(e.scs_table(keys[p], w[p], 5) - s) <= bound


def test_negative_or_nan_w_and_duplicate_keys_are_refused():
    """W is a distance (include/mapeval_hip.h, me_scs_table): w < 0, NaN, or a key listed twice is ME_ERR_ARG."""
    from cloud_map_evaluation_amd.engine import MapEvalError

    keys, w = V.scs_tables()["size33"]
    with _engine() as e:
        for bad in (-1e-300, -1.0, np.nan, -np.inf):
            x = w.copy()
            x[20] = bad
            with pytest.raises(MapEvalError, match=r"^\[-1\]"):
                e.scs_table(keys, x, 2)
        k = keys.copy()
        k[32] = k[4]
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            e.scs_table(k, w, 2)
        x = w.copy()
        x[20] = 0.0  # -0.0 and 0.0 are values
        x[21] = -0.0
        _check(e, keys, x, 2)
