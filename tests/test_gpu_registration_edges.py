"""The registration path on the device (me_reg.hip: k_knn_normals + fast_eigen3x3, k_gicp_cov, k_rotate_attr, k_lsq_sums<1|2>,
k_lsq_final; icp.py: lsq_update, _icp_lsq) at scale and at its edges, judged by the numpy model of tests/_reg_ref.py next to the
oracle: every normal of 100 000 .. 5 000 000-point scenes (no mask: the oracle at 1e-9 where the eigenvalue gap allows it, the
perturbation bound of the raw-moment covariance elsewhere), exactly degenerate neighbourhoods, hand-made normals through
k_gicp_cov, attribute drift over 30 updates, the 29 sums of one step against math.fsum within the bound of the summation shape,
and the loops where the oracle's cannot follow (empty gate, rank-deficient J^T J, rotated attributes)."""
import math
import time

import numpy as np
import pytest

import _reg_ref as R

pytestmark = pytest.mark.gpu

SEEN_BRANCHES = set()
MAXIMA = dict(c_dev=0.0, c_ref=0.0, b_dev=0.0, b_ref=0.0)


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


_scene_cache = {}


def _scene(name, n):
    if (name, n) not in _scene_cache:
        _scene_cache.clear()  # (one scene at a time: the 5 M one holds 120 MB)
        _scene_cache[(name, n)] = R.scene(name, n)
    return _scene_cache[(name, n)]


# ---------------------------------------------------------------------------------------------------- normals ----
@pytest.mark.parametrize("name,n,k,shift", R.NORMAL_CASES, ids=lambda v: str(v))
def test_normals_every_point_is_judged(eng, name, n, k, shift):
    """Per point, with the device's own (bit-exact) neighbour list: unit and finite, no mask; equal to the oracle within 1e-9 where
    the relative gap (w1 - w0) / w2 of normal_exact exceeds G_REL; elsewhere within C_DEV u S / (w1 - w0) of normal_exact's
    eigenvector (the bound of a symmetric matrix perturbed by the rounding of E[xx] - E[x]E[x], S = max E[x_i^2]); only where that
    bound exceeds 1 rad is a point left with the first check.  C_DEV is twice the oracle's own maximum over these scenes (measured
    on the CPU, _reg_ref.C_REF).  The caps keep the test from passing by excluding."""
    import oracle

    xyz = _scene(name, n) + np.array(R.SHIFTS[shift])
    t0 = time.time()
    eng.upload(1, xyz, cell_size=0.1)
    nrm, idx, _ = eng.estimate_normals(1, k, with_neighbours=True)
    t1 = time.time()
    assert not np.isnan(nrm).any()
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-12
    ref = oracle.estimate_normals_knn(xyz, k)
    ex = R.normal_exact(xyz, idx)
    relgap = ex["gap01"] / np.maximum(ex["w"][:, 2], 1e-300)
    bound = R.C_DEV * R.U * ex["S"] / np.maximum(ex["gap01"], 1e-300)
    strict = relgap > R.G_REL
    undefined = ~strict & (bound > 1.0)
    r_dev, r_ref = R.normal_ratio(nrm, ex), R.normal_ratio(ref, ex)
    MAXIMA["c_dev"] = max(MAXIMA["c_dev"], float(np.nanmax(r_dev)))
    MAXIMA["c_ref"] = max(MAXIMA["c_ref"], float(np.nanmax(r_ref)))
    worst = np.abs(nrm[strict] - ref[strict]).max()
    print(f"\n{name} n={n} k={k} {shift}: device {t1 - t0:.2f} s, model {time.time() - t1:.1f} s; |dev - oracle| on {strict.mean():.4f} of the "
          f"points {worst:.2e}; handed {np.mean(~strict):.5f}, undefined {undefined.mean():.5f}; C device {np.nanmax(r_dev):.4g} "
          f"oracle {np.nanmax(r_ref):.4g}; differ from the oracle at all: {np.any(nrm != ref, axis=1).mean():.4f}")
    assert np.mean(~strict) <= 0.10
    if k >= 5:
        assert np.mean(bound > 1.0) <= 0.01
    assert worst < 1e-9
    soft = ~strict & ~undefined
    ang = R.angle_sign_free(nrm[soft], ex["vec"][soft])
    assert np.all(ang <= bound[soft])
    # the bound also holds on the strict points (a sign-free statement against the definition, not the oracle)
    assert np.all(R.angle_sign_free(nrm[strict], ex["vec"][strict]) <= np.minimum(bound[strict], math.pi))


def test_degenerate_neighbourhoods(eng):
    """Small exactly degenerate clouds.  Where the model takes a branch without acos / cos (zero matrix, diagonal matrix) the device
    equals it bit for bit; elsewhere it equals the oracle within 1e-9 where the gap allows, with NaN at the same places (none
    expected off the far lattice; printed).  Then the answers that need no model."""
    import oracle

    got = {}
    for name, (xyz, k) in R.degenerate_clouds().items():
        eng.upload(0, xyz, cell_size=0.1)
        nrm, idx, d2 = eng.estimate_normals(0, k, with_neighbours=True)
        oidx, od2 = oracle.knn(xyz, xyz, k)
        assert np.array_equal(idx, oidx) and np.array_equal(d2, od2), name
        ref = oracle.estimate_normals_knn(xyz, k)
        mo, br, plain = R.normal_open3d(xyz, idx)
        SEEN_BRANCHES.update(np.unique(br).tolist())
        nan = np.isnan(nrm).any(1)
        print(f"\n{name}: branches {np.bincount(br, minlength=10).tolist()} plain {int(plain.sum())} NaN device {int(nan.sum())} "
              f"oracle {int(np.isnan(ref).any(1).sum())}; |dev - oracle| {np.nanmax(np.abs(nrm - ref)):.2e}")
        assert np.array_equal(np.isnan(nrm), np.isnan(ref)) and np.array_equal(np.isnan(nrm), np.isnan(mo)), name
        fixed = br <= R.BR_DIAG_Z
        assert np.array_equal(nrm[fixed], mo[fixed]) and np.array_equal(nrm[fixed], ref[fixed]), name
        assert np.abs(np.linalg.norm(nrm[~nan], axis=1) - 1).max() < 1e-12, name
        if not name.startswith("far_") and not name.startswith("line_diag"):
            ex = R.normal_exact(xyz, idx)
            ok = ~fixed & (ex["gap01"] / np.maximum(ex["w"][:, 2], 1e-300) > R.G_REL)
            if ok.any():
                assert np.abs(nrm[ok] - ref[ok]).max() < 1e-9, name
        got[name] = nrm
    inner = R.lattice_interior()
    for a, nm in enumerate("xyz"):  # the axis of the zero variance, at k = 5 and k = 9
        for k in (5, 9):
            assert np.array_equal(got[f"plane_{nm}_k{k}"][inner], np.tile(np.eye(3)[a], (int(inner.sum()), 1)))
    g3 = R.degenerate_clouds()["cubic_lattice_k7"][0]
    # the centre, x == y == z: the three variances are the same arithmetic, an exact three-way tie, and z wins it
    assert np.array_equal(got["cubic_lattice_k7"][np.all(g3 == 0.5, axis=1)], [[0.0, 0, 1]])
    assert np.array_equal(got["line_z_k5"], np.tile([0.0, 0, 1], (12, 1)))  # x and y tie for the smallest: z, ALONG the line (upstream)
    for nm, d in (("line_x_k5", [1.0, 0, 0]), ("line_y_k5", [0, 1.0, 0]), ("line_diag_k5", np.ones(3) / math.sqrt(3)),
                  ("line_diag_k12", np.ones(3) / math.sqrt(3))):
        n = got[nm]
        assert np.isfinite(n).all() and np.abs(n @ np.asarray(d)).max() < 1e-9, nm
    tilt_n = (R._rot(1, 30.0) @ R._rot(0, 30.0))[:, 2]
    for nm in ("plane_tilted_k9", "plane_tilted_k20"):
        assert np.abs(np.abs(got[nm] @ tilt_n) - 1).max() < 1e-9, nm
    for nm in ("pile_k3", "pile_k5"):
        assert np.array_equal(got[nm][:5], np.tile([0.0, 0, 1], (5, 1))), nm
    tri = R.degenerate_clouds()["three_k3"][0]
    tn = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    tn /= np.linalg.norm(tn)
    for nm in ("three_k3", "three_k40"):
        assert np.abs(np.abs(got[nm] @ tn) - 1).max() < 1e-12, nm
    assert np.array_equal(got["two_k20"], [[0.0, 0, 1], [0, 0, 1]])
    # evec0 x evec1 on the half_det < 0 side: all three eigenvalues round to one number, nothing depends on an ulp of acos / cos, and the
    # SIGN is that of the oracle and the model
    xyz, k = R.degenerate_clouds()["isotropic_k7"]
    mo, br, _ = R.normal_open3d(xyz, oracle.knn(xyz, xyz, k)[0])
    assert np.all(br == R.BR_NEG_CROSS)
    assert np.abs(got["isotropic_k7"] - mo).max() < 1e-9 and np.abs(got["isotropic_k7"] - oracle.estimate_normals_knn(xyz, k)).max() < 1e-9
    assert set(R.BR_REACHABLE) <= SEEN_BRANCHES, sorted(SEEN_BRANCHES)


# ---------------------------------------------------------------------------------------------------- attributes ----
@pytest.mark.parametrize("eps", [1e-6, 1e-3, 1.0])
def test_gicp_covariances_of_hand_made_normals(eng, eps):
    import oracle

    rng = np.random.default_rng(8)
    m = 100_000
    nrm = rng.normal(size=(m + 16, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    s = math.sqrt(1 - 0.99 ** 2)
    special = np.array([[-1.0, 0, 0], [np.nextafter(-0.99, -1), s, 0], [-0.99, s, 0], [np.nextafter(-0.99, 0), s, 0], [0, 1.0, 0], [0, 0.6, -0.8],
                        [1.0, 0, 0], [0, 0, 1.0]])
    nrm[:8] = special
    nrm[8:16] = special * np.array([3.0, 0.5, 2.0, 1.5, 7.0, 0.25, 4.0, 9.0])[:, None]  # non-unit: through set_normals as they are
    nonunit = np.zeros(len(nrm), bool)
    nonunit[8:16] = True
    eng.upload(0, rng.uniform(0, 5, (len(nrm), 3)), cell_size=0.1)
    eng.set_normals(0, nrm)
    cov = eng.gicp_covariances(0, eps, fetch=True)
    assert np.array_equal(eng.get_normals(0), nrm)
    ref = oracle.gicp_covariances(nrm, eps)
    assert np.abs(cov - ref).max() < 1e-12
    assert np.abs(cov - R.gicp_cov(nrm, eps)).max() < 1e-12
    ident = nrm[:, 0] < -0.99
    assert ident[0] and ident[1] and not ident[2] and not ident[3] and ident[8] and not ident[9]  # (scaled: -3 and -0.495)
    assert 100 < ident.sum() < 2000  # (the cap x0 < -0.99 holds 0.5 % of the sphere)
    assert np.array_equal(cov[ident], np.broadcast_to(np.diag([eps, 1.0, 1.0]), (int(ident.sum()), 3, 3)))
    u = ~ident & ~nonunit
    Cu, nu = cov[u], nrm[u]
    assert np.abs(Cu - np.swapaxes(Cu, 1, 2)).max() < 1e-15
    assert np.abs(np.einsum("nij,nj->ni", Cu, nu) - eps * nu).max() < 1e-12
    assert np.abs(np.trace(Cu, axis1=1, axis2=2) - (2 + eps)).max() < 1e-12
    assert np.abs(Cu - R.gicp_cov_definition(nu, eps)).max() < 1e-12


def test_gicp_epsilon_must_be_positive(eng):
    from cloud_map_evaluation_amd.engine import MapEvalError

    eng.upload(0, np.random.default_rng(0).uniform(0, 1, (100, 3)), cell_size=0.1)
    for bad in (0.0, -1e-3, float("nan")):
        with pytest.raises(MapEvalError):
            eng.gicp_covariances(0, bad)


YAW135 = np.eye(4)
YAW135[:3, :3] = [[math.cos(math.radians(135.0)), -math.sin(math.radians(135.0)), 0],
                  [math.sin(math.radians(135.0)), math.cos(math.radians(135.0)), 0], [0, 0, 1]]
YAW135[:3, 3] = (12.0, -7.0, 1.5)  # (the pose of test_gpu_outlier.py::test_coarse_align_with_outlier_filter)


def test_attributes_do_not_drift_over_thirty_updates(eng):
    import oracle
    from cloud_map_evaluation_amd.icp import vector6_to_matrix

    xyz = R.scene("campus", 20_000)
    eng.upload(0, xyz, cell_size=0.1)
    nrm = eng.estimate_normals(0, 20)
    cov = eng.gicp_covariances(0, 1e-3, fetch=True)
    rng = np.random.default_rng(21)
    pts = xyz
    updates = [vector6_to_matrix(np.r_[rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)]) for _ in range(30)] + [YAW135]
    for i, T in enumerate(updates):
        eng.transform_cloud(0, T)
        nrm, cov = oracle.rotate_attributes(T, nrm, cov)
        pts = oracle.transform(pts, T)
        if i in (0, 9, 29, 30):
            dn, dc = eng.get_normals(0), eng.get_covariances(0)
            assert np.abs(np.linalg.norm(dn, axis=1) - 1).max() < 1e-13
            w = np.linalg.eigvalsh(dc)
            assert np.abs(w - np.array([1e-3, 1.0, 1.0])).max() < 1e-12
            # C <- (R C) R^T is not symmetric in rounded arithmetic: an entry is two nested 3-term dot products, within 6 u sum|R||C||R^T|
            # <= 18 u of the exact value (|C| <= 1, a row of |R| sums to <= sqrt(3)), so the asymmetry grows by <= 36 u per update
            assert np.abs(dc - np.swapaxes(dc, 1, 2)).max() <= 36 * R.U * (i + 1)
            assert np.abs(dn - nrm).max() < 1e-13 and np.abs(dc - cov).max() < 1e-13
            assert np.array_equal(eng.download(0), pts)
    # the model's rotation is the device's, bit for bit (same association, no contraction), over the whole chain
    n0 = eng.estimate_normals(0, 20)
    c0 = eng.gicp_covariances(0, 1e-3, fetch=True)
    eng.transform_cloud(0, YAW135)
    mn, mc = R.rotate_attr(YAW135, n0, c0)
    assert np.array_equal(eng.get_normals(0), mn) and np.array_equal(eng.get_covariances(0), mc)


# ---------------------------------------------------------------------------------------------------- the least-squares step ----
def _lsq_pair(kind, n, shift):
    from cloud_map_evaluation_amd import synth

    if kind == "campus":  # est = the thinned, perturbed ground truth, cut to 256 j + 1 points: the last block holds one thread's row
        est, gt = synth.campus_pair(n, seed=5)
        est, gt = est.numpy(), gt.numpy()
        est = est[:256 * ((len(est) - 1) // 256) + 1]
    else:                 # an independent scan of exactly n points (100 000: 391 blocks, no multiple of 256)
        est, gt = synth.scan_pair(n, seed=5)
        est, gt = est.numpy(), gt.numpy()
    sh = np.array(R.SHIFTS[shift])
    return est + sh, gt + sh


LSQ_CASES = [("campus", 100_000, "none"), ("campus", 100_000, "near"), ("scan", 100_000, "none"), ("scan", 100_000, "near"),
             ("campus", 1_000_000, "none"), ("campus", 1_000_000, "near"), ("scan", 1_000_000, "none"), ("scan", 1_000_000, "near"),
             ("campus", 5_000_000, "none"), ("scan", 5_000_000, "near")]  # (5 M: each pair once, one shifted: ~25 s of model per sum)


def _solve_distance_bound(JTJ, JTr, B):
    """|x_dev - x_exact|_2 for x = solve(JTJ, -JTr) when every entry of JTJ and JTr is within its B_k: with dA, db the matrices of the
    bounds, the classical perturbation result |dx| <= |A^-1| (|db| + |dA| |x|) / (1 - |A^-1| |dA|) in the 2-norm, plus the solver's
    own backward error 64 u cond(A) |x|.  It is cond(JTJ) times the relative size of the B_k, stated without dividing by a sum
    that may be 0."""
    dA, db, _, _ = R.sums_to_system(B)
    sv = np.linalg.svd(JTJ, compute_uv=False)
    x = np.linalg.solve(JTJ, -JTr)
    inv = 1.0 / sv[-1]
    na = np.linalg.norm(dA, 2)
    assert inv * na < 0.5, "the system is too ill-conditioned for its own rounding: no statement about the solution"
    return x, inv * (np.linalg.norm(db) + na * np.linalg.norm(x)) / (1 - inv * na) + 64 * R.U * (sv[0] / sv[-1]) * np.linalg.norm(x)


def _check_sums(eng, mode, est, cs, gt, tattr, idx, d2, max_d, tag, with_oracle=True, solve=True):
    import oracle

    s = eng.icp_lsq_sums(0, mode, max_d)
    terms, keep = R.lsq_terms(mode, est, cs, gt, tattr, idx, d2, max_d)
    exact, _ = R.lsq_sums_exact(terms)
    abs_sums = np.abs(terms).sum(0)  # (numpy's pairwise sum: a relative 1e-15 on the size of a bound)
    B = R.lsq_bound(len(est), abs_sums)
    dev = R.device_sums(s)
    JTJ = np.array(list(s.JTJ)).reshape(6, 6)
    assert s.n_corr == int(keep.sum()) and s.n_source == len(est), tag
    assert np.array_equal(JTJ, JTJ.T), tag
    with np.errstate(all="ignore"):
        r_dev = np.nanmax(np.where(B > 0, np.abs(dev - exact) / B, np.where(dev == exact, 0.0, np.inf)))
    MAXIMA["b_dev"] = max(MAXIMA["b_dev"], float(r_dev))
    line = f"{tag} mode {mode} max_d {max_d:g}: n_corr {s.n_corr}, |device - exact| / B {r_dev:.3f}"
    if with_oracle:
        o = R.device_sums(oracle.icp_lsq_sums(mode, est, cs if mode == 2 else None, gt, tattr, max_d))
        with np.errstate(all="ignore"):
            r_ref = np.nanmax(np.where(B > 0, np.abs(o - exact) / B, 0.0))
        MAXIMA["b_ref"] = max(MAXIMA["b_ref"], float(r_ref))
        line += f", |oracle - exact| / B {r_ref:.3f}"
    print(line)
    assert np.all(np.abs(dev - exact) <= B), (tag, mode, max_d, np.abs(dev - exact) / B)
    if solve and s.n_corr >= 6:
        eJ, er, _, _ = R.sums_to_system(exact)
        x_ex, dist = _solve_distance_bound(eJ, er, B)
        x_dev = np.linalg.solve(JTJ, -np.array(list(s.JTr)))
        assert np.linalg.norm(x_dev - x_ex) <= dist, (tag, mode, max_d, np.linalg.norm(x_dev - x_ex), dist)
    return s, exact, keep


@pytest.mark.parametrize("kind,n,shift", LSQ_CASES, ids=lambda v: str(v))
def test_lsq_sums_against_the_exact_sums(eng, kind, n, shift):
    """Each of the 29 sums within B_k = (m + 8 + ceil(nblocks / 256) + 8) u sum|term_k| of math.fsum over the same fp64 terms: the launch
    is min(1024, ceil(n / 256)) blocks of 256 threads (me_icp_lsq_sums), so a thread adds m = ceil(n / (256 nblocks)) terms in
    sequence, block_sum_256 is an 8-level tree (6 levels inside a wave, then (s0 + s1) + (s2 + s3)), k_lsq_final adds
    ceil(nblocks / 256) partials per thread and reduces with the same tree.  math.fsum is exact, so nothing is added for the
    reference.  The solution of the step is held to the perturbation bound of _solve_distance_bound."""
    est, gt = _lsq_pair(kind, n, shift)
    nb, m = R.lsq_launch(len(est))
    print(f"\n{kind} {n} {shift}: {len(est)} source points, {nb} blocks, m = {m}")
    if n == 100_000:
        assert nb % 256 != 0 and (kind != "campus" or len(est) % 256 == 1)
    eng.upload(0, est, cell_size=0.1)
    eng.upload(1, gt, cell_size=0.1)
    n_gt = eng.estimate_normals(1, 20)
    ct = eng.gicp_covariances(1, 1e-3, fetch=True)
    cs = eng.gicp_covariances(0, 1e-3, fetch=True)
    idx, d2 = eng.nn1(0, 1)
    for mode in (1, 2):
        for max_d in (0.05, 0.5, 1e6):
            _check_sums(eng, mode, est, cs, gt, ct if mode == 2 else n_gt, idx, d2, max_d, f"{kind} {n} {shift}",
                        with_oracle=(n < 5_000_000 or max_d == 0.5))


def _hand_attrs(eng, slot, n, seed):
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    eng.set_normals(slot, nrm)
    return nrm, eng.gicp_covariances(slot, 1e-3, fetch=True)


def test_lsq_gate_is_strict_at_dyadic_distances(eng):
    i = np.arange(16)
    tgt = np.stack([4.0 * i, np.zeros(16), np.zeros(16)], -1)
    src = tgt.copy()
    even = i % 2 == 0
    src[even, 0] += 0.5                       # d2 == 0.25 == max_d^2 exactly: excluded
    src[~even, 1] = np.nextafter(0.5, 0)      # d2 == 0.25 - 2^-54, one ulp of 0.25 below it: included
    eng.upload(0, src, cell_size=1.0)
    eng.upload(1, tgt, cell_size=1.0)
    _, cs = _hand_attrs(eng, 0, 16, 1)
    nt, ct = _hand_attrs(eng, 1, 16, 2)
    idx, d2 = eng.nn1(0, 1)
    assert np.array_equal(idx, i) and np.all(d2[even] == 0.25) and np.all(d2[~even] == 0.25 - 2.0 ** -54)
    for mode in (1, 2):
        s, _, keep = _check_sums(eng, mode, src, cs, tgt, ct if mode == 2 else nt, idx, d2, 0.5, "dyadic gate", solve=False)  # (collinear sources: no full-rank system)
        assert s.n_corr == 8 and np.array_equal(keep, ~even)
        assert s.sum_d2 == 8 * (0.25 - 2.0 ** -54)
        s = eng.icp_lsq_sums(0, mode, np.nextafter(0.5, 1))  # one ulp wider: max_d^2 rounds above 0.25, everything passes
        assert s.n_corr == 16


def test_lsq_empty_gate_and_identical_clouds(eng):
    est, gt = _lsq_pair("campus", 20_000, "near")
    eng.upload(0, est + 50.0, cell_size=0.1)
    eng.upload(1, gt, cell_size=0.1)
    n_gt = eng.estimate_normals(1, 20)
    eng.gicp_covariances(0, 1e-3)
    eng.gicp_covariances(1, 1e-3)
    eng.nn1(0, 1, fetch=False)
    for mode in (1, 2):  # nothing inside the gate: all 29 sums exactly 0
        s = eng.icp_lsq_sums(0, mode, 0.5)
        assert s.n_corr == 0 and s.n_source == len(est)
        assert np.array_equal(R.device_sums(s), np.zeros(29))
    eng.upload(0, gt, cell_size=0.1)  # source == target: every residual exactly 0
    cs = eng.gicp_covariances(0, 1e-3, fetch=True)
    ct = eng.gicp_covariances(1, 1e-3, fetch=True)
    assert np.array_equal(cs, ct)
    idx, d2 = eng.nn1(0, 1)
    assert np.array_equal(idx, np.arange(len(gt))) and not d2.any()
    for mode in (1, 2):
        s, exact, _ = _check_sums(eng, mode, gt, cs, gt, ct if mode == 2 else n_gt, idx, d2, 0.5, "source == target")
        assert s.n_corr == len(gt) and s.r2 == 0.0 and s.sum_d2 == 0.0 and not np.array(list(s.JTr)).any()
        assert np.linalg.eigvalsh(np.array(list(s.JTJ)).reshape(6, 6)).min() > 0


@pytest.mark.parametrize("ns", [1, 2, 255, 256, 257])
def test_lsq_tiny_source_against_a_large_target(eng, ns):
    est, gt = _lsq_pair("campus", 50_000, "none")
    est = est[1000:1000 + ns]
    eng.upload(0, est, cell_size=0.1)
    eng.upload(1, gt, cell_size=0.1)
    n_gt = eng.estimate_normals(1, 20)
    ct = eng.gicp_covariances(1, 1e-3, fetch=True)
    _, cs = _hand_attrs(eng, 0, ns, ns)
    idx, d2 = eng.nn1(0, 1)
    for mode in (1, 2):
        _check_sums(eng, mode, est, cs, gt, ct if mode == 2 else n_gt, idx, d2, 1e6, f"{ns} source points")


def test_lsq_attribute_requirements(eng):
    from cloud_map_evaluation_amd.engine import MapEvalError

    est, gt = _lsq_pair("campus", 20_000, "none")
    eng.upload(0, est, cell_size=0.1)
    eng.upload(1, gt, cell_size=0.1)
    eng.gicp_covariances(0, 1e-3)  # the source carries covariances (and normals), the target nothing
    eng.nn1(0, 1, fetch=False)
    with pytest.raises(MapEvalError, match="covariances"):
        eng.icp_lsq_sums(0, 2, 0.5)
    with pytest.raises(MapEvalError, match="normals"):
        eng.icp_lsq_sums(0, 1, 0.5)
    eng.estimate_normals(1, 20, fetch=False)
    with_src = R.device_sums(eng.icp_lsq_sums(0, 1, 0.5))
    eng.upload(0, est, cell_size=0.1)  # the same source without attributes: point-to-plane ignores the source's normals
    eng.nn1(0, 1, fetch=False)
    assert np.array_equal(R.device_sums(eng.icp_lsq_sums(0, 1, 0.5)), with_src)


# ---------------------------------------------------------------------------------------------------- the loops ----
def _pairwise_sums(terms):
    """the loop at 1 000 000 points: numpy's pairwise column sums (relative 1e-15) in place of math.fsum, for time; the comparison below
    is at 1e-8"""
    t = np.asarray(terms)
    return t.sum(0), np.abs(t).sum(0)


MOTION_SMALL = [0.004, -0.003, 0.006, 0.05, -0.04, 0.03]   # (test_gpu_registration.py)
MOTION_LARGE = [0.05, -0.04, 0.06, 0.3, -0.2, 0.1]         # ~3 degrees per axis, 0.3 m: n_corr changes from iteration to iteration


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("motion,max_d", [("small", 1.0), ("large", 0.5)])
def test_loops_follow_the_model_at_a_million_points(eng, monkeypatch, method, motion, max_d):
    import oracle
    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.icp import vector6_to_matrix

    est, gt = synth.campus_pair(1_000_000, seed=7)
    est, gt = est.numpy(), gt.numpy()
    src = oracle.transform(est, vector6_to_matrix(MOTION_SMALL if motion == "small" else MOTION_LARGE))
    eng.upload(0, src, cell_size=0.1)
    eng.upload(1, gt, cell_size=0.1)
    n_gt = eng.estimate_normals(1, 20)
    cs = ct = None
    if method == 2:
        eng.estimate_normals(0, 20, fetch=False)
        cs = eng.gicp_covariances(0, 1e-3, fetch=True)
        ct = eng.gicp_covariances(1, 1e-3, fetch=True)
    t0 = time.time()
    res = eng.performICPRegistration(max_d, method=method)
    t1 = time.time()
    monkeypatch.setattr(R, "lsq_sums_exact", _pairwise_sums)
    got = R.icp_lsq_loop(method, src, gt, max_d, src_cov=cs, tgt_attr=ct if method == 2 else n_gt)
    print(f"\nmethod {method} {motion}: device {t1 - t0:.1f} s, model {time.time() - t1:.1f} s, {res['iterations']} iterations, n_corr per "
          f"evaluation {[h[0] for h in got['history']]}")
    assert res["iterations"] == got["iterations"] and res["n_corr"] == got["n_corr"]
    assert res["fitness"] == got["fitness"]
    assert abs(res["inlier_rmse"] - got["inlier_rmse"]) < 1e-9
    assert np.abs(res["transformation"] - got["transformation"]).max() < 1e-8
    assert np.abs(eng.download(0) - got["cloud"]).max() < 1e-7
    if motion == "large":
        assert len({h[0] for h in got["history"]}) > 2
    else:  # the oracle's loop (the same program on a full-rank pair) on the small motion only: its CPU loop at 1 M points is the cost
        ref = oracle.registration_icp(method, src, gt, max_d, tgt_normals=n_gt if method == 1 else None)
        assert res["iterations"] == ref["iterations"] and res["n_corr"] == ref["n_corr"]
        assert abs(res["fitness"] - ref["fitness"]) < 1e-12
        assert np.abs(res["transformation"] - ref["transformation"]).max() < 1e-8


@pytest.mark.parametrize("method", [1, 2])
def test_loop_with_nothing_inside_the_gate(eng, method):
    est, gt = _lsq_pair("campus", 20_000, "none")
    src = est + np.array([0.0, 0.0, 80.0])
    eng.upload(0, src, cell_size=0.1)
    eng.upload(1, gt, cell_size=0.1)
    eng.estimate_normals(1, 20, fetch=False)
    res = eng.performICPRegistration(0.5, method=method)
    assert res["iterations"] == 1 and res["n_corr"] == 0 and res["fitness"] == 0.0 and res["inlier_rmse"] == 0.0
    assert np.array_equal(res["transformation"], np.eye(4))
    assert np.array_equal(eng.download(0), src)


def test_point_to_plane_on_a_plane_shifted_in_its_plane(eng):
    """J^T J of point-to-plane on one horizontal plane has rank 3 (rz, tx, ty are invisible).  Certain without Open3D at hand: the
    call returns, everything is finite, and fitness / n_corr are those of the model's loop under the same lsq_update rule."""
    plane = R.plane_lattice(2, 60, 60, 0.25, 0.5)
    nrm = np.tile([0.0, 0, 1], (len(plane), 1))
    src = plane + np.array([0.0625, 0.03125, 0.0])
    for method in (1, 2):
        eng.upload(0, src, cell_size=0.25)
        eng.upload(1, plane, cell_size=0.25)
        eng.set_normals(1, nrm)
        cs = ct = None
        if method == 2:
            eng.set_normals(0, nrm)
            cs = eng.gicp_covariances(0, 1e-3, fetch=True)
            ct = eng.gicp_covariances(1, 1e-3, fetch=True)
        res = eng.performICPRegistration(0.5, method=method)
        got = R.icp_lsq_loop(method, src, plane, 0.5, src_cov=cs, tgt_attr=ct if method == 2 else nrm)
        out = eng.download(0)
        print(f"\nplane, method {method}: {res['iterations']} iterations (model {got['iterations']}), n_corr {res['n_corr']}, fitness {res['fitness']}")
        assert np.isfinite(res["transformation"]).all() and np.isfinite(out).all()
        assert res["n_corr"] == got["n_corr"] and res["fitness"] == got["fitness"]
        if method == 1:  # exact zeros in rows rz, tx, ty: LAPACK reports the singular factor, the update is the identity
            assert res["iterations"] == 1 and np.array_equal(res["transformation"], np.eye(4)) and np.array_equal(out, src)


def test_rotated_attributes_enter_the_first_step_after_a_coarse_pose(eng):
    import oracle

    est, gt = _lsq_pair("scan", 100_000, "none")
    moved = est @ YAW135[:3, :3].T + YAW135[:3, 3]
    back = np.linalg.inv(YAW135)
    eng.upload(0, moved, cell_size=0.1)
    eng.upload(1, gt, cell_size=0.1)
    n0 = eng.estimate_normals(0, 20)
    c0 = eng.gicp_covariances(0, 1e-3, fetch=True)
    ct = eng.gicp_covariances(1, 1e-3, fetch=True)
    eng.transform_cloud(0, back)
    src = eng.download(0)
    assert np.array_equal(src, oracle.transform(moved, back))
    mn, mc = R.rotate_attr(back, n0, c0)
    on, oc = oracle.rotate_attributes(back, n0, c0)
    dn, dc = eng.get_normals(0), eng.get_covariances(0)
    assert np.abs(dn - on).max() < 1e-13 and np.abs(dc - oc).max() < 1e-13
    assert np.array_equal(dn, mn) and np.array_equal(dc, mc)  # (so the exact sums below are built from the bits the device holds)
    assert np.abs(np.linalg.norm(dn, axis=1) - 1).max() < 1e-13
    assert np.abs(np.linalg.eigvalsh(dc) - np.array([1e-3, 1.0, 1.0])).max() < 1e-12
    idx, d2 = eng.nn1(0, 1)
    _check_sums(eng, 2, src, mc, gt, ct, idx, d2, 1.0, "rotated attributes")
    res = eng.performICPRegistration(1.0, method=2)  # normals present: the covariances are rebuilt from the ROTATED normals
    got = R.icp_lsq_loop(2, src, gt, 1.0, src_cov=R.gicp_cov(mn, 1e-3), tgt_attr=ct)
    assert res["iterations"] == got["iterations"] and res["n_corr"] == got["n_corr"] and res["fitness"] == got["fitness"]
    assert np.abs(res["transformation"] - got["transformation"]).max() < 1e-8


def test_zz_report_maxima():
    """(runs last in the file) the figures DESIGN.md records"""
    print(f"\nMAXIMA normals: C device {MAXIMA['c_dev']:.4g}, oracle {MAXIMA['c_ref']:.4g} (C_REF {R.C_REF}); sums: |device - exact| / B "
          f"{MAXIMA['b_dev']:.3f}, |oracle - exact| / B {MAXIMA['b_ref']:.3f}")
    assert MAXIMA["b_dev"] <= 1.0
