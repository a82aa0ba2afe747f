"""The numpy model of the registration path (tests/_reg_ref.py) held to what exists before it judges the device: normal_open3d
against oracle.estimate_normals_knn (bit for bit; the points that differ at all are counted and capped at 1 %), against
normal_exact within the conditioning bound; gicp_cov / rotate_attr / the exact least-squares sums / the loop against the oracle's;
the caps on the points the GPU test may hand to a weaker check, with the oracle and normal_exact alone.  No GPU."""
import numpy as np
import pytest

import _reg_ref as R
import oracle
from cloud_map_evaluation_amd import icp, synth

N_SMALL = 20_000


@pytest.mark.parametrize("name", ["scan", "campus", "cube"])
def test_normal_open3d_is_the_oracle_and_both_stay_inside_the_caps(name):
    """Comparison: bit for bit wherever model and oracle agree on acos / cos (the model calls the C library's, as the oracle does);
    the points that differ at all are counted, must stay within 1e-12 and below 1 % of the scene.  Then the caps of the GPU test,
    from the oracle and normal_exact alone: <= 10 % of a scene handed from the 1e-9 comparison to the conditioning bound, <= 1 %
    with a bound above 1 rad (normal undefined) at k >= 5."""
    base = R.scene(name, N_SMALL)
    seen = set()
    for sh in ("none", "near", "far"):
        xyz = base + np.array(R.SHIFTS[sh])
        for k in R.KS:
            idx, _ = oracle.knn(xyz, xyz, k)
            ref = oracle.estimate_normals_knn(xyz, k)
            mo, br, _ = R.normal_open3d(xyz, idx)
            seen |= set(np.unique(br).tolist())
            differ = np.any(mo != ref, axis=1)
            ex = R.normal_exact(xyz, idx)
            ratio = R.normal_ratio(ref, ex)
            relgap = ex["gap01"] / np.maximum(ex["w"][:, 2], 1e-300)
            bound = R.C_DEV * R.U * ex["S"] / np.maximum(ex["gap01"], 1e-300)
            handed, undefined = ~(relgap > R.G_REL), bound > 1.0
            print(f"{name} {sh} k={k}: differ {differ.sum()} max {np.abs(mo - ref).max():.2e}; oracle C {np.nanmax(ratio):.3g}; "
                  f"handed {handed.mean():.4f} undefined {undefined.mean():.4f}")
            assert not np.isnan(ref).any() and not np.isnan(mo).any()
            assert differ.mean() <= 0.01 and np.abs(mo - ref).max() <= 1e-12
            assert np.abs(np.linalg.norm(mo, axis=1) - 1).max() < 1e-12
            assert handed.mean() <= 0.10
            if k >= 5:
                assert undefined.mean() <= 0.01
            # model against the definition, sign-free, within the bound given to the device.  C_REF is the reference's maximum over the
            # scenes of the GPU test; at k = 3 the ratio has a heavy tail on other scenes (printed above; three points leave the closed
            # form's own error, not the raw-moment subtraction, in charge), so the statement is made for k >= 4
            if k >= 4:
                ang = R.angle_sign_free(mo, ex["vec"])
                assert np.all(ang[~undefined] <= bound[~undefined])
    assert {R.BR_POS_CROSS, R.BR_NEG_EV0} <= seen


def test_degenerate_clouds_model_equals_oracle_and_reaches_every_branch():
    seen = set()
    for name, (xyz, k) in R.degenerate_clouds().items():
        idx, _ = oracle.knn(xyz, xyz, k)
        ref = oracle.estimate_normals_knn(xyz, k)
        mo, br, plain = R.normal_open3d(xyz, idx)
        seen |= set(np.unique(br).tolist())
        print(name, "branches", np.bincount(br, minlength=10).tolist(), "plain", int(plain.sum()), "nan", int(np.isnan(ref).any(1).sum()))
        assert np.array_equal(np.isnan(mo), np.isnan(ref)), name
        assert np.array_equal(mo, ref, equal_nan=True), name  # bit for bit: same C library, same operation order
    assert set(R.BR_REACHABLE) <= seen, sorted(seen)
    assert seen == set(R.BR_REACHABLE)  # (4, 5, 8: dead code, see _reg_ref.py)
    # the answers that can be stated without a model
    for a, nm in enumerate("xyz"):
        xyz, k = R.degenerate_clouds()[f"plane_{nm}_k5"]
        n = oracle.estimate_normals_knn(xyz, k)[R.lattice_interior()]
        assert np.array_equal(n, np.tile(np.eye(3)[a], (len(n), 1)))  # the axis of the zero variance
    g3, k = R.degenerate_clouds()["cubic_lattice_k7"]
    centre = np.all(g3 == 0.5, axis=1)  # x == y == z: the three variances are the same arithmetic, an exact three-way tie: z wins
    assert centre.sum() == 1 and np.array_equal(oracle.estimate_normals_knn(g3, k)[centre], [[0.0, 0, 1]])
    # a line along z: diag(0, 0, v), neither x nor y is STRICTLY smallest, so the tie goes to z, ALONG the line (upstream's rule)
    lz, k = R.degenerate_clouds()["line_z_k5"]
    assert np.array_equal(oracle.estimate_normals_knn(lz, k), np.tile([0.0, 0, 1], (len(lz), 1)))
    for nm, d in (("line_x_k5", [1.0, 0, 0]), ("line_y_k5", [0, 1.0, 0]), ("line_diag_k5", np.ones(3) / np.sqrt(3)),
                  ("line_diag_k12", np.ones(3) / np.sqrt(3))):
        xyz, k = R.degenerate_clouds()[nm]
        n = oracle.estimate_normals_knn(xyz, k)
        assert np.isfinite(n).all() and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12 and np.abs(n @ np.asarray(d)).max() < 1e-9, nm


def test_gicp_cov_and_rotate_attr_equal_the_oracle():
    rng = np.random.default_rng(3)
    n = rng.normal(size=(5000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    q = np.sqrt(1 - 0.99 ** 2)
    n[:8] = [[-1, 0, 0], [np.nextafter(-0.99, -1), q, 0], [-0.99, q, 0], [np.nextafter(-0.99, 0), q, 0], [0, 1, 0], [1, 0, 0],
             [0, 0, 1], [0.3, -2.0, 5.0]]
    for eps in (1e-6, 1e-3, 1.0):
        c = R.gicp_cov(n, eps)
        assert np.array_equal(c, oracle.gicp_covariances(n, eps))
        ident = n[:, 0] < -0.99
        assert ident[:2].all() and not ident[2:8].any()
        assert np.array_equal(c[ident], np.broadcast_to(np.diag([eps, 1.0, 1.0]), c[ident].shape))
        unit = ~ident & (np.arange(len(n)) != 7)
        assert np.abs(c[unit] - R.gicp_cov_definition(n[unit], eps)).max() < 1e-12
    c = R.gicp_cov(n, 1e-3)
    T = icp.vector6_to_matrix([0.3, -0.2, 0.5, 1, 2, 3])
    n2, c2 = R.rotate_attr(T, n, c)
    o2, oc2 = oracle.rotate_attributes(T, n, c)
    assert np.array_equal(n2, o2) and np.array_equal(c2, oc2)
    assert np.array_equal(R.transform_points(n * 7, T), oracle.transform(n * 7, T))
    assert np.array_equal(R.vector6_to_matrix([0.3, -0.2, 0.5, 1, 2, 3]), T)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shift", ["none", "near"])
def test_exact_sums_against_the_oracle_and_the_literal_rows(mode, shift):
    est, gt = synth.campus_pair(6000, seed=3)
    est, gt = est.numpy() + np.array(R.SHIFTS[shift]), gt.numpy() + np.array(R.SHIFTS[shift])
    n_gt = oracle.estimate_normals_knn(gt, 20)
    cs = R.gicp_cov(oracle.estimate_normals_knn(est, 20), 1e-3)
    ct = R.gicp_cov(n_gt, 1e-3)
    idx, d2 = oracle.nn1(gt, est)
    for max_d in (0.05, 0.5, 1e6):
        terms, keep = R.lsq_terms(mode, est, cs, gt, ct if mode == 2 else n_gt, idx, d2, max_d)
        s, a = R.lsq_sums_exact(terms)
        o = oracle.icp_lsq_sums(mode, est, cs if mode == 2 else None, gt, ct if mode == 2 else n_gt, max_d)
        assert o["n_corr"] == keep.sum() == len(terms)
        # the oracle adds the same fp64 terms one after the other: n - 1 additions, each within u of the running sum
        assert np.all(np.abs(R.device_sums(o) - s) <= len(terms) * R.U * a)
        # the exact sums are exact: invariant under a permutation of the rows, and equal to the integer-arithmetic sum
        perm = np.random.default_rng(0).permutation(len(terms))
        assert np.array_equal(R.lsq_sums_exact(terms[perm])[0], s)
        from fractions import Fraction
        for col in (0, 20, 26, 27):
            assert float(sum(map(Fraction, terms[:, col].tolist()))) == s[col]
        if max_d == 0.5:  # the literal per-row Open3D form, independent of lsq_terms
            JTJ, JTr, r2 = R.lsq_open3d_rows(mode, est, cs, gt, ct if mode == 2 else n_gt, idx, keep)
            mJ, mr, m2, _ = R.sums_to_system(s)
            scale = np.sqrt(np.outer(np.diag(mJ), np.diag(mJ)))
            assert np.abs((mJ - JTJ) / scale).max() < 1e-9 and abs(m2 - r2) <= 1e-9 * r2
            assert np.abs(mr - JTr).max() <= 1e-9 * np.sqrt(np.diag(mJ) * m2).max()
    # the model's own 1-NN against the oracle's
    from scipy.spatial import cKDTree
    i2, dd = R.nn1(cKDTree(gt), gt, est)
    assert np.array_equal(i2, idx) and np.array_equal(dd, d2)


def test_lsq_launch_and_bound():
    assert R.lsq_launch(1) == (1, 1) and R.lsq_launch(256) == (1, 1) and R.lsq_launch(257) == (2, 1)
    assert R.lsq_launch(100_097) == (392, 1) and R.lsq_launch(262_144) == (1024, 1) and R.lsq_launch(262_145) == (1024, 2)
    assert R.lsq_launch(5_000_000) == (1024, 20)
    assert R.lsq_bound(5_000_000, [1.0])[0] == (20 + 8 + 4 + 8) * R.U


@pytest.mark.parametrize("mode", [1, 2])
def test_loop_follows_the_oracle_on_a_full_rank_pair(mode):
    est, gt = synth.campus_pair(8000, seed=7)
    est, gt = est.numpy(), gt.numpy()
    T0 = icp.vector6_to_matrix([0.004, -0.003, 0.006, 0.05, -0.04, 0.03])
    src = oracle.transform(est, T0)
    n_gt = oracle.estimate_normals_knn(gt, 20)
    ref = oracle.registration_icp(mode, src, gt, 1.0, tgt_normals=n_gt if mode == 1 else None)
    if mode == 1:
        got = R.icp_lsq_loop(1, src, gt, 1.0, tgt_attr=n_gt)
    else:
        got = R.icp_lsq_loop(2, src, gt, 1.0, src_cov=R.gicp_cov(oracle.estimate_normals_knn(src, 20), 1e-3),
                             tgt_attr=R.gicp_cov(n_gt, 1e-3))
    assert got["iterations"] == ref["iterations"] and got["n_corr"] == ref["n_corr"]
    assert abs(got["fitness"] - ref["fitness"]) < 1e-12 and abs(got["inlier_rmse"] - ref["inlier_rmse"]) < 1e-9
    assert np.abs(got["transformation"] - ref["transformation"]).max() < 1e-8
    assert np.abs(got["cloud"] - ref["cloud"]).max() < 1e-7


def test_loop_singular_rule_and_empty_gate():
    """a horizontal plane against itself shifted in-plane: point-to-plane sees no residual and J^T J has rank 3; the loop returns,
    finite; a gate nothing passes: one evaluation, identity"""
    plane = R.plane_lattice(2, 30, 30, 0.25, 0.5)
    nrm = np.tile([0.0, 0, 1], (len(plane), 1))
    src = plane + np.array([0.0625, 0.03125, 0.0])
    got = R.icp_lsq_loop(1, src, plane, 0.5, tgt_attr=nrm)
    assert np.isfinite(got["transformation"]).all() and np.isfinite(got["cloud"]).all() and got["n_corr"] > 0
    far = R.icp_lsq_loop(1, src + 100.0, plane, 0.5, tgt_attr=nrm)
    assert far["iterations"] == 1 and far["n_corr"] == 0 and np.array_equal(far["transformation"], np.eye(4))
    assert np.array_equal(far["cloud"], src + 100.0)
    assert np.array_equal(R.lsq_update(np.zeros((6, 6)), np.ones(6)), np.eye(4))
    assert np.array_equal(R.lsq_update(np.zeros((6, 6)), np.ones(6)), icp.lsq_update(np.zeros((6, 6)), np.ones(6)))
