"""me_m3c2 / me_m3c2_fetch on the MI355X against the brute-force model of tests/_m3c2_ref.py: the cylinder sets exactly, the strict
edges on a dyadic lattice, dist / var / lod within the derived bounds, the sign, core points inside, at the
edge of and far outside the other cloud's frame, the sizes around a wave and a block, the mask, the totals and the state rules."""
import ctypes as C
import math

import numpy as np
import pytest

import _m3c2_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _sheet(n, seed, z=0.0, noise=0.004, lo=(0.0, 0.0), hi=(1.0, 1.0)):
    rng = np.random.default_rng(seed)
    p = np.empty((n, 3))
    p[:, 0] = lo[0] + (hi[0] - lo[0]) * rng.random(n)
    p[:, 1] = lo[1] + (hi[1] - lo[1]) * rng.random(n)
    p[:, 2] = z + noise * rng.standard_normal(n)
    return np.ascontiguousarray(p)


def _tilted(n, seed, tilt=0.3):
    rng = np.random.default_rng(seed)
    v = np.array([0.0, 0.0, 1.0]) + tilt * rng.standard_normal((n, 3))
    return np.ascontiguousarray(v / np.linalg.norm(v, axis=1)[:, None])


def _run(own, other, nrm, rp, L, min_points=5, reg=0.0, mask=None, query=0, cell=0.0):
    from cloud_map_evaluation_amd.engine import Engine

    with Engine(0) as e:
        e.upload(query, own, cell_size=cell)
        e.upload(1 - query, other, cell_size=cell)
        e.set_normals(query, nrm)
        return e.m3c2(query, rp, L, min_points, reg, mask, fetch=True)


def _same_sets(pp, m):
    assert np.array_equal(pp["n_own"], m["n_own"]) and np.array_equal(pp["n_other"], m["n_other"])
    assert np.array_equal(pp["valid"], m["valid"])


# ---- 1. exact sets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_own,n_other,rp,L", [(700, 500, 0.05, 0.15), (4097, 3000, 0.03, 0.09), (900, 1100, 0.09, 0.03)])
def test_sets_equal_the_model_on_every_point(n_own, n_other, rp, L):
    """one cylinder longer than wide (two sizes), one wider than long; random tilted unit normals"""
    own, other = _sheet(n_own, 1), _sheet(n_other, 2, z=0.01)
    nrm = _tilted(n_own, 3)
    tot, pp = _run(own, other, nrm, rp, L)
    m = R.m3c2(own, other, nrm, rp, L, exact=False)
    _same_sets(pp, m)
    assert 0 < tot["n_valid"] == int(m["valid"].sum()) and tot["n_core"] == n_own and tot["n_no_normal"] == 0
    assert m["n_own"].max() > 8


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------
def test_points_on_the_wall_and_on_the_caps_are_excluded():
    """step 1/8, rp = 5/8, L = 2/8, normals +z: lattice points lie exactly on the cylinder's wall (3, 4, .) / (5, 0, .) and on its caps
    (k = +-2); every quantity is a small dyadic number, so the arithmetic is exact and the strict convention alone decides"""
    pts = np.array([(i / 8, j / 8, k / 8) for i in range(-6, 7) for j in range(-6, 7) for k in range(-3, 4)], np.float64)
    other = pts + [0.0, 0.0, 1 / 8]  # the same lattice one step up: the ties are there too
    nrm = np.tile([0.0, 0.0, 1.0], (len(pts), 1))
    tot, pp = _run(pts, other, nrm, 5 / 8, 2 / 8, min_points=2)
    m = R.m3c2(pts, other, nrm, 5 / 8, 2 / 8, min_points=2)
    _same_sets(pp, m)
    centre = int(np.flatnonzero((pts == 0).all(axis=1))[0])
    disc = sum(1 for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 25)  # 69 of the 81 with <= 25
    assert pp["n_own"][centre] == 3 * disc  # k in {-1, 0, 1}: one step inside the caps is in, the caps are out
    assert pp["n_other"][centre] == 3 * disc  # k' = k + 1 in {-1, 0, 1}
    # t, S and Q are exact here; the divisions by n and n - 1 and the square root round, so the values are held to the bounds of the
    # accuracy test, and where the model's own figure is exact (the centre: S = 0 in both clouds) to equality
    v = m["valid"]
    no, nt = pp["n_own"][v].astype(np.float64), pp["n_other"][v].astype(np.float64)
    assert (np.abs(pp["dist"][v] - m["dist"][v]) <= (no + nt) * U * 0.25).all()
    for key, cnt in (("var_own", no), ("var_other", nt)):
        assert (np.abs(pp[key][v] - m[key][v]) <= (3 * cnt + 10) * U * 0.25 * 0.25).all(), key
    lod = 1.96 * np.sqrt(pp["var_own"][v] / no + pp["var_other"][v] / nt)
    assert (np.abs(pp["lod"][v] - lod) <= 2 * np.spacing(lod)).all()
    assert np.array_equal(pp["significant"][v], np.abs(pp["dist"][v]) > pp["lod"][v])
    assert pp["dist"][centre] == 0.0 and pp["var_own"][centre] == pp["var_other"][centre] == m["var_own"][centre] > 0


# ---- 3. accuracy ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy_case():
    own, other = _sheet(1500, 11, noise=0.01), _sheet(1300, 12, z=0.02, noise=0.01)
    nrm = _tilted(1500, 13, 0.15)
    rp, L, reg = 0.08, 0.2, 0.003
    return own, other, nrm, rp, L, reg, _run(own, other, nrm, rp, L, 5, reg), R.m3c2(own, other, nrm, rp, L, 5, reg)


def test_dist_and_variances_within_the_derived_bounds(accuracy_case):
    own, other, nrm, rp, L, reg, (tot, pp), m = accuracy_case
    _same_sets(pp, m)
    v = m["valid"]
    assert v.sum() > 1000
    no, nt = pp["n_own"][v].astype(np.float64), pp["n_other"][v].astype(np.float64)
    err_d = np.abs(pp["dist"][v] - m["dist"][v])
    print("max |dist - model| / ((n_own + n_other) u L):", float((err_d / ((no + nt) * U * L)).max()))
    assert (err_d <= (no + nt) * U * L).all()
    for key, cnt in (("var_own", no), ("var_other", nt)):
        err = np.abs(pp[key][v] - m[key][v])
        print(key, "max err / ((3 n + 10) u L^2):", float((err / ((3 * cnt + 10) * U * L * L)).max()))
        assert (err <= (3 * cnt + 10) * U * L * L).all(), key  # (<= 8 n u L^2: DESIGN.md section 4.15)
        assert (pp[key][v] >= 0).all()
    assert (pp["dist"][~v] == 0).all() and (pp["lod"][~v] == 0).all() and (pp["var_own"][~v] == 0).all()


def test_lod_and_significance_follow_the_devices_own_values(accuracy_case):
    own, other, nrm, rp, L, reg, (tot, pp), m = accuracy_case
    v = pp["valid"]
    lod = 1.96 * (np.sqrt(pp["var_own"][v] / pp["n_own"][v] + pp["var_other"][v] / pp["n_other"][v]) + reg)
    assert (np.abs(pp["lod"][v] - lod) <= 2 * np.spacing(lod)).all()
    assert np.array_equal(pp["significant"][v], np.abs(pp["dist"][v]) > pp["lod"][v])
    assert not pp["significant"][~v].any()
    assert 0 < pp["significant"].sum() < v.sum()  # (a 2 cm offset under 1 cm of roughness: both outcomes occur)


# ---- 4. sign -------------------------------------------------------------------------------------------------------------------
def test_negated_normals_negate_dist_bit_for_bit(accuracy_case):
    own, other, nrm, rp, L, reg, (tot, pp), m = accuracy_case
    tot2, pp2 = _run(own, other, -nrm, rp, L, 5, reg)
    assert np.array_equal(pp2["dist"], -pp["dist"])
    for k in ("n_own", "n_other", "var_own", "var_other", "lod", "valid", "significant"):
        assert np.array_equal(pp2[k], pp[k]), k
    assert tot2["sum_dist"] == -tot["sum_dist"] and tot2["sum_abs_dist"] == tot["sum_abs_dist"] and tot2["argmax"] == tot["argmax"]


# ---- 5. frame edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap", [False, True])
def test_core_points_inside_at_the_edge_of_and_beyond_the_other_frame(swap):
    """the small cloud covers [0, 1]^2; the large one reaches 0.6 beyond it on every side: its points are inside the small cloud's box,
    outside it by less than R (they still collect the border points) and outside it by more than R (n_other == 0)"""
    small = _sheet(1500, 21, z=0.005)
    large = _sheet(6000, 22, lo=(-0.6, -0.6), hi=(1.6, 1.6))
    rp, L = 0.06, 0.12
    Rb = math.hypot(rp, L)
    own, other = (small, large) if swap else (large, small)
    nrm = _tilted(len(own), 23, 0.2)
    tot, pp = _run(own, other, nrm, rp, L, min_points=3)
    m = R.m3c2(own, other, nrm, rp, L, min_points=3, exact=False)
    _same_sets(pp, m)
    if not swap:
        lo, hi = small[:, :2].min(axis=0), small[:, :2].max(axis=0)
        out = np.maximum(np.maximum(lo - own[:, :2], own[:, :2] - hi), 0).max(axis=1)  # distance outside the box, per axis
        inside, near, far = out == 0, (out > 0) & (out < Rb), out > Rb
        assert inside.sum() > 500 and near.sum() > 300 and far.sum() > 1000
        assert (pp["n_other"][far] == 0).all() and not pp["valid"][far].any()
        assert (pp["n_other"][near] > 0).sum() > 100  # the border cell's block served them
        assert pp["valid"][inside].sum() > 400
    else:
        assert pp["valid"].sum() > 1000  # every core point lies inside the larger cloud's frame


# ---- 6. sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_sizes_around_a_wave_and_a_block_on_either_side(n):
    rp, L = 0.12, 0.2
    a, b = _sheet(n, 30 + n, hi=(0.5, 0.5)), _sheet(257, 31, z=0.01, hi=(0.5, 0.5))
    for own, other in ((a, b), (b, a)):
        nrm = _tilted(len(own), 32, 0.1)
        tot, pp = _run(own, other, nrm, rp, L, min_points=2)
        m = R.m3c2(own, other, nrm, rp, L, min_points=2, exact=False)
        _same_sets(pp, m)
        assert tot["n_core"] == len(own) and tot["n_valid"] == int(m["valid"].sum())
    if n == 1:  # the core point is its own only neighbour
        tot, pp = _run(a, b, _tilted(1, 32, 0.1), rp, L, min_points=2)
        assert pp["n_own"][0] == 1 and not pp["valid"][0] and tot["n_valid"] == 0 and tot["argmax"] == -1 and tot["max_abs_dist"] == 0


# ---- 7. mask, zero normals, totals -----------------------------------------------------------------------------------------------
def test_mask_zero_normals_and_totals():
    n = 3000
    own, other = _sheet(n, 41, noise=0.01), _sheet(2500, 42, z=0.015, noise=0.01)
    nrm = _tilted(n, 43, 0.1)
    nrm[5::50] = 0.0
    mask = np.zeros(n, np.uint8)
    mask[::3] = 1
    mask[5::50] = 7  # (any non-zero byte)
    rp, L, reg = 0.07, 0.15, 0.001
    tot, pp = _run(own, other, nrm, rp, L, 5, reg, mask)
    m = R.m3c2(own, other, nrm, rp, L, 5, reg, mask=mask, exact=False)
    _same_sets(pp, m)
    off = mask == 0
    for k in ("dist", "lod", "var_own", "var_other", "n_own", "n_other"):
        assert (pp[k][off] == 0).all(), k
    assert not pp["valid"][off].any() and not pp["significant"][off].any()
    zero = (mask != 0) & ~nrm.any(axis=1)
    assert not pp["valid"][zero].any() and (pp["n_own"][zero] > 0).all()
    v = pp["valid"]
    nv = int(v.sum())
    assert (tot["n_core"], tot["n_no_normal"], tot["n_valid"], tot["n_significant"]) == (int((mask != 0).sum()), int(zero.sum()), nv,
                                                                                          int(pp["significant"].sum()))
    assert tot["sum_n_own"] == int(pp["n_own"][v].sum()) and tot["sum_n_other"] == int(pp["n_other"][v].sum())
    d = pp["dist"][v]
    for key, terms in (("sum_dist", d), ("sum_abs_dist", np.abs(d)), ("sum_dist2", d * d), ("sum_lod", pp["lod"][v])):
        err, bound = abs(tot[key] - math.fsum(terms)), nv * U * float(np.abs(terms).max())
        print(key, "error / (n u max|term|):", err / bound)
        assert err <= bound, key
    worst = np.flatnonzero(np.abs(pp["dist"]) == np.abs(d).max())
    assert tot["max_abs_dist"] == np.abs(d).max() and tot["argmax"] == int(worst[v[worst]].min())
    assert tot["mean_dist"] == tot["sum_dist"] / nv and tot["significant_share"] == tot["n_significant"] / nv


# ---- 8. state ------------------------------------------------------------------------------------------------------------------
def test_state_rules_and_bit_identical_repeats():
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import Engine, MapEvalError

    own, other = _sheet(2000, 51, noise=0.008), _sheet(1800, 52, z=0.01, noise=0.008)
    nrm = _tilted(2000, 53, 0.1)
    rp, L = 0.06, 0.15
    keys = ("dist", "lod", "var_own", "var_other", "n_own", "n_other", "valid", "significant")

    def same(a, b):
        return all(np.array_equal(a[k], b[k]) for k in keys)

    # (the uploads ask for a cell far below R = 0.16: every first call re-indexes both slots at R, the same index each time)
    with Engine(0) as e:  # a fresh context
        e.upload(0, own, cell_size=0.02)
        e.upload(1, other, cell_size=0.02)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):  # ME_ERR_STATE: no normals on the query slot
            e.m3c2(0, rp, L)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):  # ... and no result to fetch
            e.m3c2_fetch(0)
        e.set_normals(0, nrm)
        t1, p1 = e.m3c2(0, rp, L, fetch=True)
        t2, p2 = e.m3c2(0, rp, L, fetch=True)  # two consecutive calls
        assert same(p1, p2) and t1 == t2
    with Engine(0) as e:  # after me_nn1 / me_mme / me_local_geometry left finer indexes and resident results
        e.upload(0, own, cell_size=0.02)
        e.upload(1, other, cell_size=0.02)
        e.set_normals(0, nrm)
        e.set_normals(1, _tilted(1800, 54))
        e.mme(0, 0.03, 5, per_point=False)
        e.local_geometry(0, 0.03)
        e.local_geometry(1, 0.03)
        e.nn1(0, 1, fetch=False)
        e.nn_surface_error(0)
        t3, p3 = e.m3c2(0, rp, L, fetch=True)
        assert same(p1, p3) and t1 == t3
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e.nn_surface_fetch(0)
        for s in (0, 1):
            assert e._L.me_local_geometry_fetch(e._ctx, s, None, None, None) == -3
        assert np.array_equal(e.get_normals(0), nrm)  # normals live in cloud order: they survive the re-index
        idx, d2 = e.nn1(0, 1)  # the 1-NN search works again
        brute = ((own[:50, None, :] - other[None, :, :]) ** 2).sum(axis=2).min(axis=1)
        assert np.allclose(d2[:50], brute, rtol=1e-12, atol=0)
        assert same(p1, e.m3c2_fetch(0))  # (the search re-indexed nothing: the result is still current)
        e.upload(1, other[:100], cell_size=0.02)  # the compared cloud changes: the result is stale
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e.m3c2_fetch(0)
        # the error returns
        p = _lib.M3c2Params(rp, L, 0.0, 5, 0)
        o = _lib.M3c2Out()
        assert e._L.me_m3c2(e._ctx, 0, C.byref(p), None, None) == -1  # out == NULL: ME_ERR_ARG
        assert e._L.me_m3c2(e._ctx, 0, None, None, C.byref(o)) == -1
        assert e._L.me_m3c2(e._ctx, 2, C.byref(p), None, C.byref(o)) == -1
        for bad in ((0.0, L, 0.0, 5), (rp, -1.0, 0.0, 5), (rp, L, -0.5, 5), (rp, L, 0.0, 1), (float("inf"), L, 0.0, 5), (rp, float("nan"), 0.0, 5)):
            with pytest.raises(MapEvalError, match=r"^\[-1\]"):
                e.m3c2(0, bad[0], bad[1], bad[3], bad[2])
    with Engine(0) as e:  # the other slot empty: ME_ERR_STATE
        e.upload(0, own, cell_size=0.02)
        e.set_normals(0, nrm)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e.m3c2(0, rp, L)
    with Engine(0) as e:  # slab mode: ME_ERR_ARG
        e.set_slab(0, 0.0, 0.5, 0.2)
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            e.m3c2(0, rp, L)


# ---- 9. the same cloud in both slots -------------------------------------------------------------------------------------------
def test_same_cloud_in_both_slots():
    own = _sheet(2000, 61, noise=0.01)
    nrm = _tilted(2000, 62, 0.15)
    rp, L = 0.07, 0.18
    tot, pp = _run(own, own, nrm, rp, L)
    assert np.array_equal(pp["n_own"], pp["n_other"])
    v = pp["valid"]
    assert v.sum() > 1500
    assert (np.abs(pp["dist"][v]) <= 2.0 * pp["n_own"][v] * U * L).all()  # the bound of the accuracy test, n_own + n_other = 2 n_own
    assert not pp["significant"].any()


def test_report_runs_both_directions_with_exact_quantiles():
    from cloud_map_evaluation_amd.engine import Engine

    est, gt = _sheet(3000, 71, z=0.012, noise=0.003), _sheet(3500, 72, noise=0.003)
    with Engine(0) as e:
        e.upload(0, est, cell_size=0.05)
        e.upload(1, gt, cell_size=0.05)
        rep = e.m3c2_report(0.08, 0.05, 0.1, quantiles=(0.1, 0.5, 0.9))
        for name, slot in (("est", 0), ("gt", 1)):
            d = rep[name]
            pp = e.m3c2_fetch(slot) if name == "gt" else None
            assert d["n_valid"] > 2000 and d["normals"]["n_valid"] > 2000
            assert 0.009 < d["mean_abs_dist"] < 0.015 and 0.0 <= d["significant_share"] <= 1.0
            if pp is not None:
                s = np.sort(pp["dist"][pp["valid"]])
                assert np.array_equal(d["quantile_dist"], s[d["rank"]])
        # the sign: seen from the map the truth lies on the other side than the map seen from the truth, up to each normal's own sign
        assert abs(abs(rep["est"]["mean_abs_dist"]) - abs(rep["gt"]["mean_abs_dist"])) < 0.002
