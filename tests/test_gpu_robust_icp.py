"""The robust registration step on the device (me_reg.hip: k_lsq_sums_robust<1|2, L1..Tukey>, k_info_sums; icp.py: the loops with a
kernel, icp_multi_scale) judged by the numpy model of tests/_robust_reg_ref.py: exact weights on a lattice at every block-shape edge,
the 31 sums of both scene pairs against math.fsum within the bound of the summation shape, the L2 id against me_icp_lsq_sums bit for
bit, the W path against the B path, a non-SPD M, the empty gate, every error return, the information matrix, and the loops."""
import ctypes as C
import math

import numpy as np
import pytest

import _reg_ref as R
import _robust_reg_ref as RR

pytestmark = pytest.mark.gpu

ARG, STATE = "[-1]", "[-3]"
K = 0.25
HEIGHTS = np.array([0.0, K / 2, -K / 2, K, -K, 2 * K, -2 * K])  # (size 1 is the row at r == 0)
SIDE = 256


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    e.n_uploads = 0  # (counted so that _pair knows whether its scene is still the resident one)
    upload = e.upload

    def counted(*a, **k):
        e.n_uploads += 1
        return upload(*a, **k)

    e.upload = counted
    yield e
    e.close()


def _lattice():
    g = np.stack(np.meshgrid(np.arange(SIDE, dtype=np.float64), np.arange(SIDE, dtype=np.float64), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g, np.zeros((len(g), 1))], 1)


def _sym(s):
    J = np.array(list(s.JTJ)).reshape(6, 6)
    return np.array_equal(J, J.T)


@pytest.mark.parametrize("ns", [1, 2, 255, 256, 257, 4097, 300_000])
def test_exact_weights_on_a_lattice(eng, ns):
    """Sources above the nodes of a unit lattice on z = 0 at dyadic heights in {0, +-k/2, +-k, +-2k}: r is the height, every weight is the
    hand value of the CPU test.  300 000 sources: the 1024-block cap, two rows per thread."""
    tgt = _lattice()
    i = np.arange(ns)
    node = i % len(tgt)
    src = tgt[node].copy()
    src[:, 2] = HEIGHTS[i % 7]
    eng.upload(0, src, cell_size=1.0)
    eng.upload(1, tgt, cell_size=1.0)
    nrm = np.tile([0.0, 0.0, 1.0], (len(tgt), 1))
    eng.set_normals(1, nrm)
    idx, d2 = eng.nn1(0, 1)
    assert np.array_equal(idx, node) and np.array_equal(d2, src[:, 2] ** 2)
    if ns == 300_000:
        assert R.lsq_launch(ns) == (1024, 2)
    for name, kern in RR.KERNELS.items():
        s = eng.icp_lsq_sums_robust(0, 1, 0.75, name, K)
        terms, keep, n_zero, n_deg = RR.robust_terms(1, kern, K, src, None, tgt, nrm, idx, d2, 0.75)
        assert keep.all() and s.n_corr == ns and s.n_source == ns and s.n_degenerate == 0 == n_deg
        assert s.n_zero_weight == n_zero, name
        if kern == RR.L1:
            assert n_zero == int((src[:, 2] == 0).sum()) >= 1
        if kern == RR.TUKEY:
            assert n_zero == int((np.abs(src[:, 2]) >= K).sum())
        assert _sym(s)
        dev = RR.device_sums(s)
        assert np.all(np.isfinite(dev))
        RR.check_sums(dev, terms, ns, f"lattice {ns} {name}")
        assert s.sum_w == pytest.approx(math.fsum(RR.weight(kern, src[:, 2], K).tolist()), rel=1e-12)


_pair_cache = {}


def _pair(eng, kind, shift):
    """upload + attributes + 1-NN of a pair, once per (kind, shift) for as long as no other upload touched the shared engine"""
    key = (kind, shift)
    if _pair_cache.get("key") != key or _pair_cache.get("uploads") != eng.n_uploads:
        est, gt = RR.lsq_pair(kind, 100_000, R.SHIFTS[shift])
        eng.upload(0, est, cell_size=0.1)
        eng.upload(1, gt, cell_size=0.1)
        n_gt = eng.estimate_normals(1, 20)
        ct = eng.gicp_covariances(1, 1e-3, fetch=True)
        cs = eng.gicp_covariances(0, 1e-3, fetch=True)
        idx, d2 = eng.nn1(0, 1)
        _pair_cache.clear()
        _pair_cache.update(key=key, uploads=eng.n_uploads, v=(est, gt, n_gt, cs, ct, idx, d2))
    else:
        eng.nn1(0, 1, fetch=False)
    return _pair_cache["v"]


@pytest.mark.parametrize("shift", ["none", "far"])
@pytest.mark.parametrize("kind", ["campus", "scan"])
def test_scene_sums_against_the_exact_sums(eng, kind, shift):
    """Both pairs of the plain step's tests at 100 000 points, unshifted and 10 km from the datum, gates 0.05 and 0.5, five kernels x two
    modes: n_corr, n_zero_weight, n_degenerate exact, J^T J exactly symmetric, each of the 31 sums within R.lsq_bound of math.fsum."""
    est, gt, n_gt, cs, ct, idx, d2 = _pair(eng, kind, shift)
    for mode in (1, 2):
        for max_d in (0.05, 0.5):
            for name, kern in RR.KERNELS.items():
                s = eng.icp_lsq_sums_robust(0, mode, max_d, kern, 0.1)
                terms, keep, n_zero, n_deg = RR.robust_terms(mode, kern, 0.1, est, cs, gt, ct if mode == 2 else n_gt, idx, d2, max_d)
                tag = f"{kind} {shift} mode {mode} gate {max_d} {name}"
                assert (s.n_corr, s.n_source, s.n_zero_weight, s.n_degenerate) == (int(keep.sum()), len(est), n_zero, n_deg), tag
                assert _sym(s), tag
                RR.check_sums(RR.device_sums(s), terms, len(est), tag)


def test_l2_is_the_plain_step_bit_for_bit(eng):
    est, *_ = _pair(eng, "campus", "none")
    for mode in (1, 2):
        a = eng.icp_lsq_sums(0, mode, 0.5)
        b = eng.icp_lsq_sums_robust(0, mode, 0.5, "l2", float("nan"))  # (L2 reads no scale)
        assert np.array_equal(R.device_sums(a), R.device_sums(b)) and (a.n_corr, a.n_source) == (b.n_corr, b.n_source)
        assert b.sum_w == (3 if mode == 2 else 1) * a.n_corr and b.sum_wr2 == a.r2 and b.n_zero_weight == 0 == b.n_degenerate
        assert b.n_corr > 50_000


def test_w_path_against_b_path(eng):
    """Huber with k = 1e300: every weight is exactly 1, so the sums are those of me_icp_lsq_sums but for the rounding of W W against
    M^-1.  The model's own two forms (math.fsum of either set of terms) differ by `model`, relative to sum|term| per column and taken
    over the columns (2.5e-16 on the CPU for this pair); the device's two paths may differ by twice that."""
    est, gt, n_gt, cs, ct, idx, d2 = _pair(eng, "campus", "none")
    a = R.device_sums(eng.icp_lsq_sums(0, 2, 0.5))
    s = eng.icp_lsq_sums_robust(0, 2, 0.5, "huber", 1e300)
    b = RR.device_sums(s)[:29]
    assert s.n_degenerate == 0 and s.n_zero_weight == 0 and s.sum_w == 3 * s.n_corr
    tw, _, _, _ = RR.robust_terms(2, RR.HUBER, 1e300, est, cs, gt, ct, idx, d2, 0.5)
    tb, _ = R.lsq_terms(2, est, cs, gt, ct, idx, d2, 0.5)
    scale = np.abs(tb).sum(0)
    model = np.abs(R.lsq_sums_exact(tw[:, :29])[0] - R.lsq_sums_exact(tb)[0]) / scale
    dev = np.abs(a - b) / scale
    print(f"\nW path vs B path, relative to sum|term|: model {model.max():.3e}, device {dev.max():.3e}")
    assert dev.max() <= 2 * model.max()
    assert s.sum_wr2 == s.r2


def test_non_spd_m_is_counted_and_left_out(eng):
    """Normals set by hand; epsilon = 1e-30 makes C = R diag(eps, 1, 1) R^T singular to working precision.  Where source and target
    normals are different axes M is diagonal and fine; where both are the same oblique direction the smallest eigenvalue of M is rounding
    noise of either sign.  The model computes the same eigenvalues bit for bit, so it names the degenerate rows."""
    rng = np.random.default_rng(3)
    n = 600
    tgt = np.stack([np.arange(n, dtype=np.float64), np.zeros(n), np.zeros(n)], -1)
    src = tgt + rng.uniform(-0.1, 0.1, (n, 3))
    ns = np.tile([1.0, 0.0, 0.0], (n, 1))
    nt = np.tile([0.0, 1.0, 0.0], (n, 1))
    ob = rng.normal(size=(n // 2, 3))
    ob /= np.linalg.norm(ob, axis=1, keepdims=True)
    ns[::2] = ob
    nt[::2] = ob
    eng.upload(0, src, cell_size=1.0)
    eng.upload(1, tgt, cell_size=1.0)
    eng.set_normals(0, ns)
    eng.set_normals(1, nt)
    cs = eng.gicp_covariances(0, 1e-30, fetch=True)
    ct = eng.gicp_covariances(1, 1e-30, fetch=True)
    idx, d2 = eng.nn1(0, 1)
    assert np.array_equal(idx, np.arange(n))
    s = eng.icp_lsq_sums_robust(0, 2, 1.0, "cauchy", 0.5)
    terms, keep, n_zero, n_deg = RR.robust_terms(2, RR.CAUCHY, 0.5, src, cs, tgt, ct, idx, d2, 1.0)
    print(f"\n{n_deg} of {n} correspondences have a non-SPD M in the model, {s.n_degenerate} on the device")
    assert 1 <= n_deg < n // 2 + 1 and s.n_degenerate == n_deg and s.n_corr == n and s.n_zero_weight == n_zero
    dev = RR.device_sums(s)
    assert np.all(np.isfinite(dev))
    RR.check_sums(dev, terms, n, "non-SPD")  # (the model's rows of the degenerate correspondences are zero but for d2)
    assert dev[28] == pytest.approx(d2.sum(), rel=1e-13)


def test_empty_gate(eng):
    est, *_ = _pair(eng, "campus", "none")
    for mode in (1, 2):
        for name in RR.KERNELS:
            s = eng.icp_lsq_sums_robust(0, mode, 1e-9, name, 0.1)
            assert (s.n_corr, s.n_zero_weight, s.n_degenerate, s.n_source) == (0, 0, 0, len(est))
            assert np.array_equal(RR.device_sums(s), np.zeros(31)) and not np.any(np.signbit(RR.device_sums(s)))
    info, n = eng.icp_information(0, 1e-9)
    assert n == 0 and np.array_equal(info, np.zeros((6, 6)))


def test_every_error_return():
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import Engine, MapEvalError

    def fails(code, fn, *a):
        with pytest.raises(MapEvalError) as ei:
            fn(*a)
        assert str(ei.value).startswith(code), str(ei.value)

    rng = np.random.default_rng(0)
    pts = rng.uniform(0, 4, (500, 3))
    with Engine(0) as e:
        e.upload(0, pts, cell_size=0.5)
        e.upload(1, pts + 0.01, cell_size=0.5)
        fails(STATE, e.icp_lsq_sums_robust, 0, 1, 0.5, "tukey", 0.1)  # no 1-NN result yet
        fails(STATE, e.icp_information, 0, 0.5)
        e.nn1(0, 1, fetch=False)
        fails(STATE, e.icp_lsq_sums_robust, 0, 1, 0.5, "tukey", 0.1)  # no normals on the reference
        fails(STATE, e.icp_lsq_sums_robust, 0, 2, 0.5, "tukey", 0.1)  # no covariances
        fails(STATE, e.icp_lsq_sums_robust, 0, 2, 0.5, "l2", 0.1)
        e.gicp_covariances(1, 1e-3)
        fails(STATE, e.icp_lsq_sums_robust, 0, 2, 0.5, "huber", 0.1)  # none on the source
        e.gicp_covariances(0, 1e-3)
        e.nn1(0, 1, fetch=False)
        assert e.icp_lsq_sums_robust(0, 2, 0.5, "huber", 0.1).n_corr == 500
        assert e.icp_lsq_sums_robust(0, 1, 0.5, _lib.ME_ROBUST_L1, float("nan")).n_corr == 500  # (L1 reads no scale)
        for slot in (-1, 2):
            fails(ARG, e.icp_lsq_sums_robust, slot, 1, 0.5, "tukey", 0.1)
            fails(ARG, e.icp_information, slot, 0.5)
        for mode in (0, 3):  # point-to-point takes no kernel
            fails(ARG, e.icp_lsq_sums_robust, 0, mode, 0.5, "tukey", 0.1)
        for kern in (-1, 6):
            fails(ARG, e.icp_lsq_sums_robust, 0, 1, 0.5, kern, 0.1)
        with pytest.raises(ValueError):
            e.icp_lsq_sums_robust(0, 1, 0.5, "welsch", 0.1)
        for kern in ("huber", "cauchy", "gm", "tukey"):
            for k in (0.0, -1.0, float("inf"), float("nan")):
                fails(ARG, e.icp_lsq_sums_robust, 0, 1, 0.5, kern, k)
        for max_d in (0.0, -1.0, float("nan")):
            fails(ARG, e.icp_lsq_sums_robust, 0, 1, max_d, "tukey", 0.1)
            fails(ARG, e.icp_information, 0, max_d)
        assert e._L.me_icp_lsq_sums_robust(e._ctx, 0, 1, 0.5, 5, 0.1, None) == -1  # NULL out
        assert e._L.me_icp_information(e._ctx, 0, 0.5, None, C.byref(C.c_int64())) == -1
        assert e._L.me_icp_information(e._ctx, 0, 0.5, np.zeros(36).ctypes.data, None) == -1
        assert e._L.me_icp_lsq_sums_robust(None, 0, 1, 0.5, 5, 0.1, C.byref(_lib.IcpRobust())) == -1
        e.set_shard(0, 2)
        fails(ARG, e.icp_lsq_sums_robust, 0, 1, 0.5, "tukey", 0.1)
        fails(ARG, e.icp_information, 0, 0.5)
        e.set_shard(0, 1)
        e.set_slab(0, 0.0, 2.0, 0.5)
        fails(ARG, e.icp_lsq_sums_robust, 0, 1, 0.5, "tukey", 0.1)
        fails(ARG, e.icp_information, 0, 0.5)
        e.set_slab(-1)
        assert e.icp_information(0, 0.5)[1] == 500


# ---------------------------------------------------------------------------------------------------- the information matrix ----
@pytest.mark.parametrize("ns", [1, 2, 255, 256, 257, 4097, 300_000])
def test_information_on_a_plane_has_the_models_rank(eng, ns):
    """Targets on the plane z = 0 with in-plane correspondences: 21 sums within the bound of fsum, exactly symmetric, and the rank of
    the model's matrix (a single target point constrains 3 directions, a line 5, a plane all 6)."""
    tgt = _lattice()
    i = np.arange(ns)
    src = tgt[i % len(tgt)] + np.array([0.125, 0.0, 0.0])
    eng.upload(0, src, cell_size=1.0)
    eng.upload(1, tgt, cell_size=1.0)
    idx, d2 = eng.nn1(0, 1)
    info, n = eng.icp_information(0, 0.5)
    terms, keep = RR.info_terms(tgt, idx, d2, 0.5)
    assert n == ns == int(keep.sum()) and np.array_equal(info, info.T)
    dev = np.array([info[a, b] for a in range(6) for b in range(a, 6)])
    exact = RR.check_sums(dev, terms, ns, f"information {ns}")
    want = np.linalg.matrix_rank(RR.tri_to_sym(exact))
    assert np.linalg.matrix_rank(info) == want == (3 if ns == 1 else 5 if ns <= 256 else 6)


@pytest.mark.parametrize("shift", ["none", "far"])
@pytest.mark.parametrize("kind", ["campus", "scan"])
def test_information_on_the_scenes(eng, kind, shift):
    est, gt, n_gt, cs, ct, idx, d2 = _pair(eng, kind, shift)
    for max_d in (0.05, 0.5):
        info, n = eng.icp_information(0, max_d)
        terms, keep = RR.info_terms(gt, idx, d2, max_d)
        assert n == int(keep.sum()) and np.array_equal(info, info.T)
        RR.check_sums(np.array([info[a, b] for a in range(6) for b in range(a, 6)]), terms, len(est), f"information {kind} {shift} {max_d}")


# ---------------------------------------------------------------------------------------------------- the loops ----
def _device_history(eng, monkeypatch):
    hist = []
    orig = eng.icp_lsq_sums_robust

    def spy(*a, **k):
        s = orig(*a, **k)
        hist.append(int(s.n_corr))
        return s

    monkeypatch.setattr(eng, "icp_lsq_sums_robust", spy)
    return hist


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("name", ["huber", "tukey"])
def test_loops_follow_the_model(eng, monkeypatch, name, method):
    import oracle
    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.icp import vector6_to_matrix

    est, gt = synth.campus_pair(100_000, seed=7)
    est, gt = est.numpy(), gt.numpy()
    src = oracle.transform(est, vector6_to_matrix([0.004, -0.003, 0.006, 0.05, -0.04, 0.03]))
    eng.upload(0, src, cell_size=0.1)
    eng.upload(1, gt, cell_size=0.1)
    n_gt = eng.estimate_normals(1, 20)
    cs = ct = None
    if method == 2:
        eng.estimate_normals(0, 20, fetch=False)
        cs = eng.gicp_covariances(0, 1e-3, fetch=True)
        ct = eng.gicp_covariances(1, 1e-3, fetch=True)
    k = 0.1 if method == 1 else 1.0  # (mode 2 residuals are whitened: in units of sigma, not of metres)
    hist = _device_history(eng, monkeypatch)
    res = eng.performICPRegistration(0.5, method=method, kernel=name, kernel_scale=k)
    got = RR.robust_loop(method, RR.KERNELS[name], k, src, gt, 0.5, src_cov=cs, tgt_attr=ct if method == 2 else n_gt)
    print(f"\n{name} method {method}: {res['iterations']} iterations, n_corr per evaluation {hist}")
    assert hist == [h[0] for h in got["history"]]
    assert res["iterations"] == got["iterations"] and res["n_corr"] == got["n_corr"] and res["fitness"] == got["fitness"]
    assert np.abs(res["transformation"] - got["transformation"]).max() < 1e-8


def test_tukey_on_the_ghosted_map_inherits_the_models_win(eng):
    gt, m, pose = RR.outlier_scene()
    eng.upload(0, m, cell_size=0.1)
    eng.upload(1, gt, cell_size=0.1)
    n_gt = eng.estimate_normals(1, 20)
    res = eng.performICPRegistration(RR.OUTLIER_GATE, method=1, kernel="tukey", kernel_scale=RR.OUTLIER_TUKEY_K)
    got = RR.robust_loop(1, RR.TUKEY, RR.OUTLIER_TUKEY_K, m, gt, RR.OUTLIER_GATE, tgt_attr=n_gt)
    assert np.abs(res["transformation"] - got["transformation"]).max() < 1e-8 and res["iterations"] == got["iterations"]
    l2 = RR.robust_loop(1, RR.L2, 1.0, m, gt, RR.OUTLIER_GATE, tgt_attr=n_gt)
    e2, et = RR.pose_error(l2["transformation"], pose), RR.pose_error(res["transformation"], pose)
    print(f"\npose error: model L2 {e2:.3e}, device Tukey {et:.3e}")
    assert et < e2 / 100


@pytest.mark.parametrize("method", [0, 1, 2])
def test_multi_scale_is_its_levels_made_by_hand(eng, method):
    """levels (4v, 2v, 0) against the same calls made by hand, bit for bit: method 1 and 2 under Tukey (2: the covariances of the private
    copies, and those of the resident clouds at the last level), method 0 plain (point-to-point takes no kernel)"""
    from cloud_map_evaluation_amd import icp
    from cloud_map_evaluation_amd.engine import Engine

    gt, m, pose = RR.outlier_scene(30_000)
    v = 0.1
    voxels, dists, iters = [4 * v, 2 * v, 0.0], [1.0, 0.5, 0.25], [10, 10, 15]
    kw = {} if method == 0 else dict(kernel="tukey", kernel_scale=0.1 if method == 1 else 1.0)

    def load():
        eng.upload(0, m, cell_size=0.1)
        eng.upload(1, gt, cell_size=0.1)
        eng.estimate_normals(1, 20, fetch=False)

    def loop(e, d, it):
        if method == 0:
            return icp.icp_point_to_point(e, d, max_iteration=it)
        if method == 1:
            return icp.icp_point_to_plane(e, d, max_iteration=it, **kw)
        return icp.icp_generalized(e, d, max_iteration=it, **kw)

    with pytest.raises(ValueError):
        icp.icp_multi_scale(eng, voxels, dists[:2], iters, method)
    load()
    gt_before = eng.download(1)
    out = icp.icp_multi_scale(eng, voxels, dists, iters, method, **kw)
    map_after, gt_after = eng.download(0), eng.download(1)
    assert np.array_equal(gt_before, gt_after) and np.array_equal(gt_before, gt)
    assert len(out["levels"]) == 3 and all(set(l) >= {"fitness", "inlier_rmse", "n_corr", "iterations"} for l in out["levels"])
    # the same calls by hand
    load()
    total, ups = np.eye(4), []
    for vs, d, it in zip(voxels, dists, iters):
        if vs > 0:
            with Engine(0) as co:
                eng.downsample_into(0, co, 0, vs)
                eng.downsample_into(1, co, 1, vs)
                if method == 1:
                    co.estimate_normals(1, 20, fetch=False)
                r = loop(co, d, it)
            eng.transform_cloud(0, r["transformation"])
        else:
            r = loop(eng, d, it)
        ups.append(r["transformation"])
        total = r["transformation"] @ total
    assert np.array_equal(out["transformation"], total)
    assert all(l["n_corr"] > 0 for l in out["levels"]) and all(np.array_equal(l["transformation"], u) for l, u in zip(out["levels"], ups))
    assert np.array_equal(map_after, eng.download(0))
    moved = m
    for u in ups[:2]:
        moved = R.transform_points(moved, u)
    # (the last level runs on the resident map: its own updates were applied one iteration at a time, so only their product is known)
    assert np.abs(R.transform_points(moved, ups[2]) - map_after).max() < 1e-9
    if method != 0:  # (an alignment: a tenth of the misalignment it started from; how close a kernel gets is the ghosted-map test's matter)
        assert RR.pose_error(out["transformation"], pose) < RR.pose_error(np.eye(4), pose) / 10
