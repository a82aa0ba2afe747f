"""k_mme3 / mme_run / the radius index at their exact edges, against the brute-force model tests/_mme_ref.py (held to the oracle on
the CPU by test_mme_ref_cpu.py, which also asserts the properties the inputs are built to have).  Every cloud has <= 2e4 points.

Every case: valid flags, n_valid and the set ent == 0 equal the model's, entropies of valid points within rtol 1e-8 / atol 1e-10
(the bound of test_mme_parity_*), no neighbourhood handed to k_mme_refine, and a second call bit-identical to the first.
k per point is read off the device by sweeping min_k (one launch each): k_i = max{m : valid_i(m)}.

(a) exact ties d^2 == r^2 on a dyadic lattice are excluded, and included at r (1 + 2^-30);  (b) probe clusters whose shell point sits
at r (1 + delta), delta straddling the FP32 band E = 2^-12 h^2: the query's valid flag is the band decision;  (c) waves of 7 - 14
rounds, a dense run between sparse points;  (d) an index reused on cells up to 1.5x the radius;  (e) clouds of 1 .. 2049 points in one
ball and over 100 cells, 4096 +- 1 points in one cell;  (f) grids at shift 0 and 1, the documented error one notch past, UTM-sized
coordinates;  (g) run to run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mme_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
K_SWEEP_MAX = 128


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _twice(eng, r, min_k):
    """(g) the same call twice: everything bit-identical"""
    a = eng.mme(0, r, min_k)
    b = eng.mme(0, r, min_k)
    assert np.array_equal(a[2], b[2]) and np.array_equal(_bits(a[1]), _bits(b[1])) and a[3] == b[3] and _bits(a[4]) == _bits(b[4])
    return a


def _against_model(eng, name, r, min_k, refine_ok=False):
    """one mme pass (twice) of the uploaded case against the model at (r, min_k) -> valid flags"""
    k, cov = R.case_moments(name, r)
    rent, rval, rnv, rsum = R.entropy_of(k, cov, min_k)
    eng.timers_reset()
    mean, ent, val, nv, s = _twice(eng, r, min_k)
    refined = eng.timer("mme_refined")[1]
    val = val.astype(bool)
    assert np.array_equal(val, rval), (name, r, min_k, np.nonzero(val != rval)[0][:10], k[val != rval][:10])
    assert nv == rnv and np.array_equal(ent == 0.0, rent == 0.0)
    np.testing.assert_allclose(ent[rval], rent[rval], rtol=R.RTOL, atol=R.ATOL, err_msg=f"{name} r={r} min_k={min_k}")
    assert abs(s - rsum) <= R.RTOL * float(np.abs(rent).sum()) + R.ATOL * rnv
    assert mean == (s / nv if nv else 0.0)
    assert refine_ok or refined == 0, (name, refined)
    return val


def _device_k(eng, r, k_top):
    """k per point by the min_k sweep 2 .. k_top + 1: the largest m at which the point is valid (0: never valid)"""
    n = eng.size(0)
    kd = np.zeros(n, np.int64)
    for m in range(2, k_top + 2):
        val = _twice(eng, r, m)[2].astype(bool)  # (g): every launch of the sweep twice, so k is bit-identical too
        kd[val] = m
    return kd


def _check_k(eng, name, r):
    """the device's k equals the model's wherever the model's entropy is finite beyond rounding: k >= 4 (three points or fewer are
    always coplanar, their determinant is rounding noise on both sides) and det > 100 eps (r^2 / 4)^3 (the scale of its terms).
    Elsewhere the device may validate the point or not, but never above its true k.  Points with k > 128 must top the sweep."""
    k, cov = R.case_moments(name, r)
    top = int(min(k.max(), K_SWEEP_MAX))
    kd = _device_k(eng, r, top)
    det = R._det(cov).astype(np.float64)
    safe = (k >= 4) & (det > 100.0 * EPS * (r * r / 4.0) ** 3)
    assert not (k >= 4).any() or safe[k >= 4].mean() > 0.99
    print(f"\n[mme-edges] {name} r={r:.6g}: k compared at {int(safe.sum())} of {len(k)} points; not comparable: {int((k < 4).sum())} with k < 4, "
          f"{int(((k >= 4) & ~safe).sum())} with k >= 4 and a determinant of rounding size")
    low = safe & (k <= K_SWEEP_MAX)
    assert np.array_equal(kd[low], k[low]), (name, r, np.nonzero(low & (kd != k))[0][:10])
    assert np.all(kd[safe & (k > K_SWEEP_MAX)] == K_SWEEP_MAX + 1)
    assert np.all((kd[~safe] == 0) | (kd[~safe] == np.minimum(k[~safe], K_SWEEP_MAX + 1)))
    return np.where(safe, kd, -1)  # (-1: not comparable)


# ---- (a) exact ties, strict radius ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto_cell", [False, True])
@pytest.mark.parametrize("steps", [2, 3])
def test_lattice_ties_are_excluded_and_a_hair_more_radius_includes_them(eng, steps, auto_cell):
    for name in (f"lattice_r{steps}", f"lattice_r{steps}_ties_in"):
        xyz, r, k_int, info = R.case(name)
        it = info["interior"]
        eng.upload(0, xyz, cell_size=0.0 if auto_cell else r)
        val = _against_model(eng, name, r, k_int)
        assert np.all(val[it]) and it.sum() == 343                      # min_k = k_interior validates every interior point
        assert not _against_model(eng, name, r, k_int + 1).any()        # ... and one more validates none: no tie was accepted
        kd = _check_k(eng, name, r)
        assert np.all(kd[it] == k_int) and kd.max() == k_int  # (every lattice neighbourhood is comparable)
    assert k_int == sum(R.lattice_counts(steps))


# ---- (b) the band, (c) many rounds per wave ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["probes_k5", "probes_k10", "rounds_k5", "rounds_k10"])
def test_band_decisions_read_through_the_valid_flag(eng, name):
    xyz, r, min_k, info = R.case(name)
    eng.upload(0, xyz, cell_size=r)
    val = _against_model(eng, name, r, min_k)
    q, sh = info["query"], info["shell"]
    acc = R.d2_lib(xyz[q], xyz[sh]) < r * r
    assert np.array_equal(val[q], acc) and acc.any() and not acc.all()  # the query is valid exactly when its shell point is inside
    _check_k(eng, name, r)


def test_dense_blob_between_sparse_points(eng):
    xyz, r, min_k, info = R.case("blob_between_sparse")
    eng.upload(0, xyz, cell_size=r)
    val = _against_model(eng, "blob_between_sparse", r, min_k)
    assert val[info["label"] == info["blob"]].all()
    _check_k(eng, "blob_between_sparse", r)


# ---- (d) index reuse on a coarser grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.REUSE_CELLS)
@pytest.mark.parametrize("name", ["lattice_r2", "scan"])
def test_index_reused_on_cells_up_to_one_and_a_half_radii(eng, name, c):
    """mme_run keeps an index whose cell edge lies in [r, 1.5 r] (c.cell_h > 1.5 want_h rebuilds): the four radii inside the window
    launch no index build ("morton" timer count, as test_a_perturb_plus_suite_costs_one_index_build counts them), the fifth one
    does; results equal the model, validity and k equal a fresh upload at cell_size = r."""
    xyz, _, _, _ = R.case(name)
    min_k = R.REUSE_MIN_K[name]
    eng.timers_enable(True)
    try:
        for i, r in enumerate(R.reuse_radii(c)):
            eng.upload(0, xyz, cell_size=c)
            eng.timers_reset()
            first = eng.mme(0, r, min_k)
            builds = eng.timer("morton")[1]
            assert builds == (1 if i == 4 else 0), (c, r, builds)
            val = _against_model(eng, name, r, min_k)
            assert np.array_equal(first[2].astype(bool), val)
            kd = _check_k(eng, name, r)
            assert eng.timer("morton")[1] == 0  # (timers were reset by _against_model: the sweep rebuilt nothing either)
            eng.upload(0, xyz, cell_size=r)
            fresh = _against_model(eng, name, r, min_k)
            assert np.array_equal(fresh, val)
            kf = _device_k(eng, r, int(min(R.case_moments(name, r)[0].max(), K_SWEEP_MAX)))
            assert np.array_equal(kf[kd >= 0], kd[kd >= 0])
    finally:
        eng.timers_enable(False)


# ---- (e) sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_sizes_in_one_ball_and_over_100_cells(eng, n):
    name = f"ball_{n}"
    xyz, r, min_k, info = R.case(name)
    eng.upload(0, xyz, cell_size=r)
    val = _against_model(eng, name, r, min_k)
    assert val.all() == (n >= min_k + 1) and val.any() == (n >= min_k + 1)  # n = min_k: none valid; n = min_k + 1: all
    if n - 1 >= 4:  # k = n - 1 observed directly: valid at min_k = n - 1, not at n
        assert _against_model(eng, name, r, n - 1).all() and not _against_model(eng, name, r, n).any()
    name = f"scattered_{n}"
    xyz, r, min_k, _ = R.case(name)
    for cell in (r, 0.0):
        eng.upload(0, xyz, cell_size=cell)
        _against_model(eng, name, r, min_k)
    _check_k(eng, name, r)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_one_cell_with_thousands_of_points(eng, n):
    name = f"dense_{n}"
    xyz, r, min_k, info = R.case(name)
    eng.upload(0, xyz, cell_size=r)
    assert _against_model(eng, name, r, min_k).all()
    assert _against_model(eng, name, r, n - 1).all() and not _against_model(eng, name, r, n).any()


# ---- (f) extent and offsets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto_cell", [False, True])
@pytest.mark.parametrize("shift", [0, 1])
def test_grids_at_shift_0_and_1(eng, shift, auto_cell):
    """Two blobs of 500 points 15.7 km (7.9 km) apart at r = 0.01: the radius grid needs 2^21 (2^20) cells per axis.  The shift is
    asserted by cloud_build_index's own arithmetic (_mme_ref.grid): the index state is not reachable from outside.
    This test found cloud_build_index refusing such a cloud altogether ("octree deeper than the level table": the 1-NN octree, which
    no radius pass uses, was built eagerly); the octree of such an index is deferred now, DESIGN 4.3.1."""
    name = f"far_shift{shift}"
    xyz, r, min_k, info = R.case(name)
    assert R.grid(xyz, r)[2] == shift
    eng.upload(0, xyz, cell_size=0.0 if auto_cell else r)
    assert _against_model(eng, name, r, min_k).all()
    assert _against_model(eng, name, r, info["k"]).all() and not _against_model(eng, name, r, info["k"] + 1).any()
    # the 1-NN octree over these cells would be deeper than its level table: the index is built without it, and the refusal comes
    # from the pass that needs it
    from cloud_map_evaluation_amd.engine import MapEvalError

    with pytest.raises(MapEvalError, match="octree deeper than the level table"):
        eng.nn1(0, 0)


def test_one_notch_past_the_largest_grid_is_the_documented_error():
    from cloud_map_evaluation_amd.engine import Engine, MapEvalError

    xyz, _ = R.far_blobs(0.01, -1)
    with pytest.raises(ValueError):
        R.grid(xyz, 0.01)
    with Engine(0) as e:
        with pytest.raises(MapEvalError, match="cell size too small for the cloud extent"):
            e.upload(0, xyz, cell_size=0.01)
    with Engine(0) as e:
        e.upload(0, xyz)  # (the automatic cell, extent / 128, fits)
        with pytest.raises(MapEvalError, match="cell size too small for the cloud extent"):
            e.mme(0, 0.01, 10)


def test_utm_sized_coordinates(eng):
    """The scan slice at (5e5, 4.5e6, 100) and at its negative against the model on the same fp64 coordinates; k per point equals the
    unshifted cloud's wherever no pair of it lies within 2^-20 r^2 of r^2 (test_mme_ref_cpu.py: that excludes < 1 % of the points)."""
    xyz, r, min_k, _ = R.case("scan")
    near = R.near_radius_share(xyz, r)
    assert near.mean() < 0.01
    eng.upload(0, xyz, cell_size=r)
    _against_model(eng, "scan", r, min_k)
    k0 = _check_k(eng, "scan", r)
    for name in ("scan_utm", "scan_utm_neg"):
        sx = R.case(name)[0]
        for cell in (r, 0.0):
            eng.upload(0, sx, cell_size=cell)
            _against_model(eng, name, r, min_k)
        kd = _check_k(eng, name, r)
        assert np.array_equal(kd[~near], k0[~near])  # (comparable points are the same set: the model's k and det agree)
