"""k_join, k_w2, the AWD mean, the CDF sort and k_scs through me_awd_scs on the MI355X, on clouds built voxel by voxel
(_vmd_ref.awd_cases), against the 50-digit model of tests/_vmd_ref.py: counts, n_rows, the bounds and population columns EQUAL, mu within
_vmd_ref.mu_bound, the stored matrices through _tol.assert_sigma_close, W within the 'voxels' tolerance of the model on the row's own
Gaussians, w_sorted = sort(W) bit for bit, awd within (M + 8) u of the mean of the rows' W, scs within _vmd_ref.scs_bound."""
import ctypes as C

import numpy as np
import pytest

import _vmd_ref as V

pytestmark = pytest.mark.gpu


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _run(e, name):
    est, gt, vs, min_pts, radius = V.awd_cases()[name]
    e.upload(0, est)
    e.upload(1, gt)
    got = e.calculateVMD(vs, min_pts, radius)
    again = e.calculateVMD(vs, min_pts, radius)
    assert (got["counts"], got["n_rows"]) == (again["counts"], again["n_rows"])  # two calls: identical bytes
    assert np.array([got["awd"], got["scs"]]).tobytes() == np.array([again["awd"], again["scs"]]).tobytes()
    assert got["rows"].tobytes() == again["rows"].tobytes() and got["w_sorted"].tobytes() == again["w_sorted"].tobytes()
    m = V.awd_model(name)
    V.check_awd(got, m, vs, radius)
    return got, m


@pytest.mark.parametrize("vs", [1.0, 0.37])
def test_populations_at_the_gate(vs):
    """(n_est, n_gt) = (99, 100), (100, 99), (100, 100), (99, 99), (101, 250) with min_pts = 100: exactly the third and the fifth match."""
    with _engine() as e:
        got, m = _run(e, f"gate_vs{vs}")
    assert got["counts"] == (5, 0, 0) and got["rows"][:, 10:12].tolist() == [[100.0, 100.0], [250.0, 101.0]]


@pytest.mark.parametrize("vs", [1.0, 0.37])
@pytest.mark.parametrize("min_pts", [2, 1])
def test_small_gates_cover_the_identity_branch_and_both_sides_of_the_storage_rule(min_pts, vs):
    """n in {1, 2, 3, 10, 11, 12} on both sides: n = 1 is the identity of regularize_sigma (min_pts = 1 lets it through, min_pts = 2 must
    not), n <= 10 stores the raw M2 and n > 10 M2 / (n - 1)^2, and all of them are divided by n - 1 once more."""
    with _engine() as e:
        got, m = _run(e, f"small_min{min_pts}_vs{vs}")
    n = got["rows"][:, 10:12]
    assert got["n_rows"] == (36 if min_pts == 1 else 25) and n.min() == min_pts and got["counts"] == (36, 0, 0)
    assert set(np.unique(n).astype(int)) == {1, 2, 3, 10, 11, 12} - ({1} if min_pts == 2 else set())


def test_est_only_and_gt_only_voxels_and_est_keys_beyond_every_gt_key():
    with _engine() as e:
        got, m = _run(e, "only_and_extreme")
    # est: (0,0,0) (1,0,0) match; (2,0,0) has 50 points; (5,5,5), (-9,0,0) below every gt key and (9,9,9) above every gt key are est-only
    assert got["counts"] == (3, 2, 3) and got["n_rows"] == 2


def test_one_ground_truth_voxel():
    with _engine() as e:
        got, m = _run(e, "vg1")
    assert got["counts"] == (1, 0, 2) and got["n_rows"] == 1 and np.isnan(got["scs"]) and got["awd"] == got["rows"][0, 9]


def test_257_est_voxels_of_which_3_match():
    with _engine() as e:
        got, m = _run(e, "est257")
    assert got["counts"] == (4, 1, 253) and got["n_rows"] == 3 and np.isnan(got["scs"])  # the three are 128 cells apart


def test_no_match_one_match_and_two_adjacent_matches():
    with _engine() as e:
        got, m = _run(e, "m0")
        assert got["n_rows"] == 0 and np.isnan(got["awd"]) and np.isnan(got["scs"]) and got["counts"] == (1, 1, 1)
        got, m = _run(e, "m1")
        assert got["n_rows"] == 1 and got["awd"] == got["rows"][0, 9] and np.isnan(got["scs"])
        got, m = _run(e, "m2_adjacent")
        assert got["n_rows"] == 2 and m["scs"] == 0.0 and abs(got["scs"]) <= V.scs_bound(1, 2, 1, np.zeros(2))


def test_capacity_too_small_sets_n_rows():
    from cloud_map_evaluation_amd.engine import MapEvalError, _addr

    est, gt, vs, min_pts, radius = V.awd_cases()["small_min2_vs1.0"]
    with _engine() as e:
        e.upload(0, est)
        e.upload(1, gt)
        rows, ws = np.full((24, 27), -7.0), np.full(24, -7.0)
        n, awd, scs = C.c_int64(24), C.c_double(), C.c_double()
        rc = e._L.me_awd_scs(e._ctx, vs, min_pts, radius, _addr(rows), _addr(ws), C.byref(n), C.byref(awd), C.byref(scs), 0)
        assert rc == -4 and n.value == 25  # ME_ERR_CAPACITY, the count still returned
        assert (rows == -7.0).all() and (ws == -7.0).all()
        with pytest.raises(MapEvalError, match=r"^\[-4\]"):
            e._ck(rc)
        for r in (0, 11):
            with pytest.raises(MapEvalError, match=r"^\[-1\]"):
                e.calculateVMD(vs, min_pts, r)
        got = e.calculateVMD(vs, min_pts, radius)  # the context is usable afterwards
        V.check_awd(got, V.awd_model("small_min2_vs1.0"), vs, radius)
