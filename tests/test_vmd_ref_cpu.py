"""The model of tests/_vmd_ref.py is right (it agrees with the project's oracle and with the reference's own printed run), its
tolerances are what was measured, and the inputs of the GPU edge tests have teeth: every deliberate mistake of the mutation table
exceeds the tolerance on an input of the family meant to catch it.  No GPU.  `pytest -s` prints the figures."""
import numpy as np
import pytest

import _vmd_ref as V

RADII = (1, 2, 5, 9, 10)


def _case(f, i):
    return f["mu1"][i], f["s1"][i], int(f["n1"][i]), f["mu2"][i], f["s2"][i], int(f["n2"][i])


def _family(name):
    return V.voxel_family() if name == "voxels" else V.w2_families()[name]


@pytest.mark.parametrize("family", list(V.W2_TOL))
def test_oracle_w2_is_within_the_measured_error_of_the_model(family):
    import oracle

    f = _family(family)
    d, s, w = V.w2_model(family)
    assert all(not isinstance(x, float) for x in d)  # the model defines a D for every input of the families
    e = max(V.w2_error_units(oracle.w2_gaussian(*_case(f, i)), d[i], s[i]) for i in range(len(w)))
    measured, tol = V.W2_TOL[family]
    print(f"\n{family:11s} {len(w):3d} inputs: oracle max e = {e:9.2f} u (written: {measured:g} u) -> tolerance {tol:g} u")
    assert e <= measured and tol == max(64.0, 8.0 * measured)
    assert e > measured / 4 or measured <= 8.0  # the written figure is the measured one, not a loose guess


def test_oracle_w2_at_nan_inputs_is_zero_as_the_model():
    import oracle

    f = V.w2_families()["generic"]
    for where in ("mu1", "mu2", "s1", "s2"):
        c = {k: f[k][3].copy() for k in f}
        c[where][1] = np.nan
        args = (c["mu1"], c["s1"], int(c["n1"]), c["mu2"], c["s2"], int(c["n2"]))
        assert V.w2_squared(*args)[2] == 0.0 and oracle.w2_gaussian(*args) == 0.0 and V.w2_f64(*args) == 0.0
    # a NaN in the matrix of a voxel of n <= 1 is never read: the identity stands in for it
    c = {k: f[k][3].copy() for k in f}
    c["s1"][4] = np.nan
    args = (c["mu1"], c["s1"], 1, c["mu2"], c["s2"], int(c["n2"]))
    d, s, w = V.w2_squared(*args)
    assert w > 0 and V.w2_error_units(oracle.w2_gaussian(*args), d, s) <= 64


def test_model_reproduces_the_w_column_of_the_reference_run(golden):
    """Every 23rd row of the fixture (310 of 7129): the inputs are 6-digit prints, so the bars are those of
    test_oracle_voxel.test_golden_w_per_voxel; against the oracle on the same printed inputs the model is held to the W tolerance."""
    import oracle

    rows = golden["rows"][::23]
    rel, e = [], []
    for r in rows:
        args = (r[18:21], V.full9(r[21:27])[0], int(r[10]), r[6:9], V.full9(r[12:18])[0], int(r[11]))
        d, s, w = V.w2_squared(*args)
        rel.append(abs(w - r[9]) / max(r[9], 1e-12))
        e.append(V.w2_error_units(oracle.w2_gaussian(*args), d, s))
    print(f"\ngolden: median rel {np.median(rel):.2e}, 99 % {np.quantile(rel, 0.99):.2e}; oracle max e = {max(e):.1f} u")
    assert np.median(rel) < 2e-3 and np.quantile(rel, 0.99) < 5e-2
    assert max(e) <= V.W2_TOL["voxels"][1]


@pytest.mark.parametrize("name", list(V.scs_tables()))
def test_oracle_scs_and_permuted_sums_are_within_the_bound(name):
    import oracle

    keys, w = V.scs_tables()[name]
    rng = np.random.default_rng(len(w))
    for r in RADII if not name.startswith("size") else (2,):
        s, per, n_max = V.scs_model(name, r)
        bound = V.scs_bound(n_max, len(w), r, per)
        o = oracle.scs(keys, w, r)
        if np.isnan(s):
            assert np.isnan(o) and np.isnan(V.scs_f64(keys, w, r))
            continue
        worst = max(abs(V.scs_f64(keys, w, r, rng=rng) - s) for _ in range(20))
        print(f"\n{name} r={r}: scs={s:.6f} N={n_max} bound={bound / V.U:.0f} u, oracle off {abs(o - s) / V.U:.1f} u, permuted off {worst / V.U:.1f} u")
        assert abs(o - s) <= bound and worst <= bound / 4


@pytest.mark.parametrize("name", list(V.awd_cases()))
def test_oracle_awd_scs_agrees_with_the_model(name):
    import oracle

    est, gt, vs, min_pts, radius = V.awd_cases()[name]
    m = V.awd_model(name)
    o = oracle.awd_scs(oracle.VoxelMap(gt, vs), oracle.VoxelMap(est, vs), min_pts, radius)
    V.check_awd(o, m, vs, radius)


# ---- the mutation table ------------------------------------------------------------------------------------------------------
W2_KILLERS = {  # mutant -> the families meant to catch it
    "div_n": ("generic", "small_n"), "no_third_division": ("generic",), "no_symmetrisation": ("asymmetric",),
    "no_clamp": ("planar", "line", "clamped"), "clamp_before_division": ("planar", "straddle", "clamped"),
    "zeros_for_n1": ("small_n",), "matrix_sqrt": ("generic",), "upper_cholesky": ("generic",),
}


def _w2_excess(family, mutant):
    """-> the largest e / tolerance of the float64 restatement with `mutant` over the family's inputs."""
    f = _family(family)
    d, s, _ = V.w2_model(family)
    return max(V.w2_error_units(V.w2_f64(*_case(f, i), mutant=mutant), d[i], s[i]) for i in range(len(d))) * V.U / V.w2_tol(family)


@pytest.mark.parametrize("family", list(V.W2_TOL))
def test_the_float64_restatement_itself_passes(family):
    assert _w2_excess(family, None) <= 1.0


@pytest.mark.parametrize("mutant", list(W2_KILLERS))
def test_every_w2_mutant_is_killed(mutant):
    killed = {fam: _w2_excess(fam, mutant) for fam in W2_KILLERS[mutant]}
    print(f"\n{mutant:22s} e / tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in killed.items()))
    assert all(v > 1.0 for v in killed.values())


def test_swapped_arguments_are_equivalent_for_w_and_caught_by_the_row_columns():
    """'arguments swapped (est first)' is dropped from the W table because it is provably equivalent there: L1 L2 is lower triangular with
    a positive diagonal and (L1 L2)(L1 L2)^T = L1 S2 L1^T, so by the uniqueness of the Cholesky factor chol(L1 S2 L1^T) = L1 L2 and its
    trace, sum_i L1_ii L2_ii, does not change when the two Gaussians change places.  A swap in k_w2 is caught where it shows: the rows
    carry n_gt, n_est, mu_est and mu_gt in fixed columns, compared for equality / to rounding, and the gate clouds have n_est != n_gt."""
    for fam in ("generic", "planar", "asymmetric", "small_n"):  # (in the 50-digit model: in float64 the two orders round differently)
        f = _family(fam)
        d, s, _ = V.w2_model(fam)
        for i in range(0, len(d), 5):
            mu1, s1, n1, mu2, s2, n2 = _case(f, i)
            assert abs(V.w2_squared(mu2, s2, n2, mu1, s1, n1)[0] - d[i]) <= 1e-40 * s[i]
    assert _w2_excess("generic", "swapped") <= 1.0
    rows = V.awd_model("gate_vs1.0")["rows"]
    assert (rows[:, 10] != rows[:, 11]).any() and (np.abs(rows[:, 6:9] - rows[:, 18:21]).max(axis=1) > 1e-3).all()


def test_the_storage_quirk_mutant_is_killed_by_the_small_gate_clouds():
    """'the n <= 10 quirk left out' acts where the stored matrix is formed, so it is evaluated from the points of the small-gate clouds:
    the voxels of 2, 3 and 10 points must see it, those of 11 and 12 must not."""
    est, gt, vs, min_pts, _ = V.awd_cases()["small_min2_vs1.0"]
    rows = V.awd_model("small_min2_vs1.0")["rows"]
    ke, kg = np.floor(est / vs), np.floor(gt / vs)
    seen = {}
    for r in rows:
        key = np.rint(r[0:3] / vs)
        pe, pg = est[(ke == key).all(axis=1)], gt[(kg == key).all(axis=1)]
        d, s, _ = V.w2_squared(r[18:21], V.full9(r[21:27])[0], int(r[10]), r[6:9], V.full9(r[12:18])[0], int(r[11]))
        for mutant in (None, "no_quirk"):
            (m1, s1, n1), (m2, s2, n2) = V.stored_sigma_f64(pg, mutant), V.stored_sigma_f64(pe, mutant)
            e = V.w2_error_units(V.w2_f64(m1, s1, n1, m2, s2, n2), d, s) * V.U / V.w2_tol("voxels")
            seen.setdefault((mutant, min(n1, n2) <= 10), []).append(e)
    print(f"\nno_quirk: e / tolerance up to {max(seen[('no_quirk', True)]):.3g} with a voxel of n <= 10")
    assert max(seen[(None, True)] + seen[(None, False)]) <= 1.0
    assert max(seen[("no_quirk", True)]) > 1.0 and max(seen[("no_quirk", False)]) <= 1.0


SCS_KILLERS = {  # mutant -> (table, radius) meant to catch it
    "centre_included": ("dense5", 1), "sample_variance": ("slab9", 2), "euclidean_ball": ("dense5", 2), "radius_plus_1": ("dense5", 1),
    "radius_minus_1": ("sparse700", 2), "neighbourless_as_zero": ("sparse700", 1), "ratio_of_means": ("sparse700", 5),
}


@pytest.mark.parametrize("mutant", V.SCS_MUTANTS)
def test_every_scs_mutant_is_killed(mutant):
    name, r = SCS_KILLERS[mutant]
    keys, w = V.scs_tables()[name]
    s, per, n_max = V.scs_model(name, r)
    bound = V.scs_bound(n_max, len(w), r, per)
    off = abs(V.scs_f64(keys, w, r, mutant=mutant) - s)
    print(f"\n{mutant:22s} on {name} r={r}: off by {off:.3e} = {off / bound:.3g} bounds")
    assert abs(V.scs_f64(keys, w, r) - s) <= bound / 4 and not off <= bound


@pytest.mark.parametrize("mutant", V.JOIN_MUTANTS)
def test_every_join_mutant_is_killed_by_the_gate_clouds(mutant):
    est, gt, vs, min_pts, _ = V.awd_cases()["gate_vs1.0"]
    (ek, ev), (gk, gv) = V.voxels(est, vs), V.voxels(gt, vs)
    en, gn = [v[2] for v in ev], [v[2] for v in gv]
    pairs, counts = V.join(ek, en, gk, gn, min_pts)
    assert [(en[i], gn[j]) for i, j in pairs] == [(100, 100), (101, 250)] and counts == (5, 0, 0)
    assert V.join_f64(ek, en, gk, gn, min_pts) == pairs and V.join_f64(ek, en, gk, gn, min_pts, mutant) != pairs
