"""Coarse global registration on the MI355X (me_globreg.hip): the down-sample into another context, FPFH, feature matching and RANSAC
against the numpy model (tests/_globreg_ref.py), coarse_align + GICP end to end, and the error paths."""
import math

import numpy as np
import pytest

import _globreg_ref as G

pytestmark = pytest.mark.gpu

VOX = 0.5


@pytest.fixture(scope="module")
def scene():
    from cloud_map_evaluation_amd import synth

    est, gt = synth.scan_pair(300_000, density=2500.0, seed=21)
    return est.numpy(), gt.numpy()


def _rot(yaw, roll=0.0, pitch=0.0):
    cz, sz, cx, sx, cy, sy = math.cos(yaw), math.sin(yaw), math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return Rz @ Ry @ Rx


def _T(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def test_downsample_into_is_the_in_place_downsample(scene):
    est, gt = scene
    with _engine() as a, _engine() as b:
        a.upload(0, est, cell_size=0.1)
        a.upload(1, gt, cell_size=0.1)
        before = a.download(0)
        n = a.downsample_into(0, b, 1, VOX)
        b.upload(0, est, cell_size=0.1)
        n_ref = b.voxel_downsample(0, VOX)
        assert n == n_ref == b.size(1)
        assert np.array_equal(b.download(1), b.download(0))
        assert np.array_equal(a.download(0), before) and a.size(0) == len(est)  # src untouched
        # dst_ctx == src_ctx, another slot
        n2 = a.downsample_into(0, a, 1, VOX)
        assert n2 == n and np.array_equal(a.download(1), b.download(0))
        assert np.array_equal(a.download(0), before)


@pytest.fixture(scope="module")
def coarse(scene):
    """0.5 m down-samples of the pair, FPFH on the device, normals and features fetched."""
    est, gt = scene
    with _engine() as e:
        e.upload(0, est, cell_size=0.1)
        e.upload(1, gt, cell_size=0.1)
        e.voxel_downsample(0, VOX)
        e.voxel_downsample(1, VOX)
        out = {}
        for s in (0, 1):
            F = e.fpfh(s, radius=5 * VOX, max_nn=40, normal_knn=30)
            out[s] = dict(xyz=e.download(s), nrm=e.get_normals(s), F=F)
        corr_m, nc_m = e.fpfh_match(0, 1, mutual=True)
        corr_a, nc_a = e.fpfh_match(0, 1, mutual=False)
        corr_r, _ = e.fpfh_match(1, 0, mutual=False)
        out["match"] = (corr_m, nc_m, corr_a, nc_a, corr_r)
    return out


def _check_fpfh(xyz, nrm, F):
    ref, edge, m = G.fpfh(xyz, nrm, radius=5 * VOX, max_nn=40)
    ok = ~edge
    assert len(xyz) > 2000
    assert ok.mean() > 0.9
    assert np.array_equal(F[ok], ref[ok]), f"{np.count_nonzero((F[ok] != ref[ok]).any(1))} points differ off the bin edges"
    if edge.any():
        l1 = np.abs(F[edge] - ref[edge]).reshape(-1, 3, 11).sum(axis=2)
        bar = 2 * 100.0 / np.maximum(m[edge], 1)
        assert (l1 <= bar[:, None] + 1e-9).all()


def test_fpfh_matches_the_model(coarse):
    for s in (0, 1):
        _check_fpfh(coarse[s]["xyz"], coarse[s]["nrm"], coarse[s]["F"])


def test_fpfh_of_a_rigidly_moved_copy(coarse):
    T = _T(_rot(2.2, 0.05, -0.03), [30.0, -20.0, 4.0])
    with _engine() as e:
        e.upload(0, coarse[0]["xyz"], cell_size=0.1)
        e.set_normals(0, coarse[0]["nrm"])
        e.transform_cloud(0, T)
        F = e.fpfh(0, radius=5 * VOX, max_nn=40, normal_knn=30)
        xyz, nrm = e.download(0), e.get_normals(0)
    _check_fpfh(xyz, nrm, F)
    # a rigid motion changes the features by rounding only
    assert np.median(np.abs(F - coarse[0]["F"]).sum(axis=1)) < 1e-6


def test_fpfh_match_is_the_exact_feature_nn(coarse):
    corr_m, nc_m, corr_a, nc_a, corr_r = coarse["match"]
    Fs, Fr = coarse[0]["F"], coarse[1]["F"]
    ref_m, sr, rs = G.match(Fs, Fr, mutual=True)
    assert np.array_equal(corr_a, sr) and nc_a == len(sr)
    assert np.array_equal(corr_r, rs)
    assert np.array_equal(corr_m, ref_m) and nc_m == int((ref_m >= 0).sum()) > 20


def _moved_pair(coarse, T):
    src = coarse[0]["xyz"] @ T[:3, :3].T + T[:3, 3]
    return src, coarse[1]["xyz"]


def test_ransac_scores_and_winner_match_the_model(coarse):
    H, eps, seed = 3000, 1.5 * VOX, 9
    T0 = _T(_rot(1.9, 0.03, 0.02), [25.0, 14.0, -2.0])
    src, ref = _moved_pair(coarse, T0)
    with _engine() as e:
        e.upload(0, src, cell_size=0.1)
        e.upload(1, ref, cell_size=0.1)
        e.set_normals(0, coarse[0]["nrm"] @ T0[:3, :3].T)
        e.set_normals(1, coarse[1]["nrm"])
        kw = dict(radius=5 * VOX, max_corr_dist=eps, max_iterations=H, validate_top=16, seed=seed, scores=True)
        T, info, sc = e.global_register(0, 1, **kw)
        corr, nc = e.fpfh_match(0, 1, mutual=True)
        T2, info2, sc2 = e.global_register(0, 1, **kw)
        T3, info3, sc3 = e.global_register(0, 1, **dict(kw, seed=seed + 1))
    assert np.array_equal(sc, sc2) and np.array_equal(T, T2) and info == info2
    assert not np.array_equal(sc, sc3)
    sel = np.flatnonzero(corr >= 0)
    cs, cq = src[sel], ref[corr[sel]]
    ref_sc, fits = G.ransac_scores(cs, cq, seed, H, eps, 0.9)
    assert np.array_equal(sc, ref_sc)
    assert info["n_corr"] == nc == len(sel) and info["n_valid_hypotheses"] == int((ref_sc >= 0).sum())
    # the model's selection: top 16 by (score desc, h asc), then fitness / rmse on the whole source by brute-force 1-NN
    valid = np.flatnonzero(ref_sc >= 0)
    top = valid[np.lexsort((valid, -ref_sc[valid]))][:16]
    best = None
    for h in top:
        Th = fits[h]
        d2 = np.empty(len(src))
        for a in range(0, len(src), 256):
            d2[a:a + 256] = G.moved_d2(Th, src[a:a + 256, None, :], ref[None, :, :]).min(axis=1)
        inl = d2 < eps * eps
        fit = inl.sum() / len(src)
        rmse = math.sqrt(d2[inl].sum() / inl.sum()) if inl.any() else 0.0
        key = (-fit, rmse, h)
        if best is None or key < best[0]:
            best = (key, h, Th)
    assert info["best_hypothesis"] == best[1]
    assert info["best_corr_inliers"] == ref_sc[best[1]]
    np.testing.assert_allclose(T[:3, :], best[2], atol=1e-12, rtol=0)
    assert info["fitness"] == pytest.approx(-best[0][0], abs=2.0 / len(src))


def _angle_deg(R):
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2))))


CASES = [  # (scene, yaw, roll, pitch, translation)
    ("scan", 2.4, 0.04, -0.05, (35.0, -22.0, 3.0)),
    ("scan", -1.8, -0.06, 0.03, (-18.0, 41.0, -5.0)),
    ("multisession", 3.0, 0.05, 0.05, (12.0, 27.0, 2.0)),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_coarse_align_then_gicp(case):
    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Param

    name, yaw, roll, pitch, t = case
    if name == "scan":
        est, gt = synth.scan_pair(200_000, density=50.0, seed=31)
    else:
        est, gt = synth.multisession_pair(200_000, density=50.0, seed=32)
    est, gt = est.numpy(), gt.numpy()
    Tm = _T(_rot(yaw, roll, pitch), t)  # the map in its own frame: est_moved = Tm est
    est_m = est @ Tm[:3, :3].T + Tm[:3, 3]
    Ttrue = np.linalg.inv(Tm)
    vox = 1.0
    p = Param(icp_max_distance_=1.0, nn_radius_=0.1, vmd_voxel_size_=0.5)
    with _engine() as e:
        e.upload(0, est_m, cell_size=0.1)
        e.upload(1, gt, cell_size=0.1)
        Tc = e.coarse_align(vox, max_iterations=200_000)
        dR = Tc[:3, :3] @ Ttrue[:3, :3].T
        assert _angle_deg(dR) < 2.0
        # translation: the map's centroid lands within half a coarse voxel of where the true T puts it (the rotation bar above bounds
        # the rest: 2 degrees are ~1 m at the corners of this 60 m scene)
        c = est_m.mean(0)
        assert np.linalg.norm((Tc[:3, :3] @ c + Tc[:3, 3]) - (Ttrue[:3, :3] @ c + Ttrue[:3, 3])) < 0.5 * vox
        e.transform_cloud(0, Tc)
        r1 = e.performICPRegistration(1.0, method=2)
        T1 = r1["transformation"] @ Tc
        s1 = e.run_suite(p)
    with _engine() as e:
        e.upload(0, est_m, cell_size=0.1)
        e.upload(1, gt, cell_size=0.1)
        e.transform_cloud(0, Ttrue)
        r0 = e.performICPRegistration(1.0, method=2)
        T0 = r0["transformation"] @ Ttrue
        s0 = e.run_suite(p)
    assert _angle_deg(T1[:3, :3] @ T0[:3, :3].T) < 0.01
    assert np.linalg.norm(T1[:3, 3] - T0[:3, 3]) < 1e-3
    np.testing.assert_allclose(s1.est_gt.rmse[0], s0.est_gt.rmse[0], rtol=1e-3)
    np.testing.assert_allclose(s1.gt_est.fitness[0], s0.gt_est.fitness[0], rtol=1e-3)


def test_error_paths(coarse):
    from cloud_map_evaluation_amd.engine import MapEvalError

    xyz = coarse[0]["xyz"]
    with _engine() as e, _engine() as f:
        with pytest.raises(MapEvalError):
            e.fpfh(0, radius=1.0, fetch=False)  # not uploaded
        e.upload(0, xyz, cell_size=0.1)
        e.upload(1, 2.0 * xyz + 1000.0, cell_size=0.1)  # every edge twice as long: no sample passes the edge-length check
        for bad in (dict(radius=0.0), dict(radius=1.0, max_nn=0), dict(radius=1.0, max_nn=41), dict(radius=1.0, normal_knn=0)):
            with pytest.raises(MapEvalError, match="me_fpfh"):
                e.fpfh(0, **bad)
        with pytest.raises(MapEvalError, match="features"):
            e.fpfh_match(0, 1)
        for bad in (dict(max_corr_dist=0.0), dict(max_corr_dist=1.0, edge_ratio=1.5), dict(max_corr_dist=1.0, max_iterations=0),
                    dict(max_corr_dist=1.0, validate_top=0)):
            with pytest.raises(MapEvalError, match=r"\[-1\]"):
                e.global_register(0, 1, radius=2.5, **bad)
        with pytest.raises(MapEvalError, match=r"\[-1\]"):
            e.global_register(0, 0, radius=2.5, max_corr_dist=1.0)
        with pytest.raises(MapEvalError, match=r"\[-1\]"):
            e.downsample_into(0, e, 0, 0.5)
        with pytest.raises(MapEvalError, match=r"\[-1\]"):
            e.downsample_into(0, f, 0, 0.0)
        with pytest.raises(MapEvalError, match="no valid hypothesis"):
            e.global_register(0, 1, radius=2.5, max_corr_dist=1.0, max_iterations=2000, mutual=False)
        # fewer than 3 correspondences: three points only, matched mutually at most twice
        e.upload(0, xyz[:3], cell_size=0.1)
        e.upload(1, xyz[3:5], cell_size=0.1)
        with pytest.raises(MapEvalError, match="at least 3"):
            e.global_register(0, 1, radius=2.5, max_corr_dist=1.0)
        # shard mode is refused
        f.upload(0, xyz, cell_size=0.1)
        f.upload(1, xyz, cell_size=0.1)
        f.set_shard(0, 2)
        with pytest.raises(MapEvalError, match="single GPU"):
            f.fpfh(0, radius=2.5)
