"""Statistical and radius outlier removal on the MI355X (me_outlier.hip) against the numpy restatement (tests/_outlier_ref.py): per-point
values bit for bit, the statistics, the masks, both k-NN paths, the selection in place and into another context, and coarse alignment
on a map with sparse outliers."""
import math

import numpy as np
import pytest

import _outlier_ref as R

pytestmark = pytest.mark.gpu


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


_SCENES = {}


def _scene(n, kind="scan"):
    from cloud_map_evaluation_amd import synth

    key = (n, kind)
    if key not in _SCENES:
        if kind == "scan":
            est, _ = synth.scan_pair(n, density=2500.0, seed=51, outlier_ratio=0.002)
        else:
            est, _ = synth.campus_pair(n, density=2500.0, seed=52, outlier_ratio=0.002)
        _SCENES.clear()
        _SCENES[key] = est.numpy()
    return _SCENES[key]


def _check_sor(xyz, k, ratios, cell_size=0.0):
    avg_ref = R.sor_avg(xyz, k)
    with _engine() as e:
        e.upload(0, xyz, cell_size=cell_size)
        for ratio in ratios:
            info, avg, keep = e.statistical_outlier(0, k, ratio, fetch=True)
            assert np.array_equal(avg, avg_ref), f"k={k}: {np.count_nonzero(avg != avg_ref)} avg_dist differ"
            mean, std, thr = R.sor_stats_device(avg_ref, ratio)  # the device's summation tree, operation for operation
            print(f"k={k} ratio={ratio}: kept {info['n_kept']} / {len(xyz)}, fallback {info['n_fallback']}, "
                  f"mean {info['mean']!r} ({mean!r}) std {info['std_dev']!r} ({std!r}) threshold {info['threshold']!r} ({thr!r})")
            assert info["n_in"] == len(xyz)
            assert info["mean"] == mean and info["std_dev"] == std and info["threshold"] == thr
            # any order of n positive terms lies within (n - 1) 2^-53 of their sum: the tree against Open3D's serial mean
            assert abs(mean - R.sor_stats(avg_ref, ratio)[0]) <= (len(xyz) - 1) * 2.0 ** -53 * mean
            assert np.array_equal(keep.astype(bool), R.sor_keep(avg_ref, thr))  # every point
            assert info["n_kept"] == int(keep.sum())
    return info


@pytest.mark.parametrize("k", [1, 2, 12, 20, 28, 40])
def test_sor_bitwise_1e5(k):
    xyz = _scene(100_000)
    info = _check_sor(xyz, k, [0.5, 1.0, 2.0])
    if k == 1:
        assert info["n_kept"] == 0  # every point's only neighbour is itself


@pytest.mark.parametrize("k", [1, 2, 20, 40])
def test_sor_bitwise_1e6_campus(k):
    _check_sor(_scene(1_000_000, "campus"), k, [0.5, 1.0, 2.0], cell_size=0.1)


@pytest.mark.parametrize("k", [1, 2, 20, 40])
def test_sor_bitwise_5e6(k):
    _check_sor(_scene(5_000_000), k, [0.5, 1.0, 2.0], cell_size=0.1)


def test_sor_grid_and_fallback_both_run():
    xyz = _scene(100_000)
    with _engine() as e:
        e.upload(0, xyz)  # (automatic cell: the radius grid's cells hold the 20 nearest of a surface point)
        info = e.statistical_outlier(0, 20, 2.0)
    # the sparse outliers (0.2 %) are isolated: the walk settles them, the grid pass the rest
    assert 0 < info["n_fallback"] < len(xyz) // 10, info


@pytest.mark.parametrize("case", ["dup", "n_lt_k", "n1", "ties"])
def test_sor_small_clouds_brute(case):
    rng = np.random.default_rng(7)
    if case == "dup":
        base = rng.random((40, 3))
        xyz = np.concatenate([base, base[:10], base[:10], np.repeat(base[:1], 6, axis=0)])
    elif case == "n_lt_k":
        xyz = rng.random((13, 3))
    elif case == "n1":
        xyz = rng.random((1, 3))
    else:  # a lattice: many ties at the k-th distance
        g = np.arange(6, dtype=np.float64) * 0.25
        xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    for k in (1, 2, 7, 20, 40):
        ref = R.brute_sor_avg(xyz, k)
        with _engine() as e:
            e.upload(0, xyz)
            info, avg, keep = e.statistical_outlier(0, k, 1.0, fetch=True)
        assert np.array_equal(avg, ref), (case, k)
        mean, std, thr = R.sor_stats_device(ref, 1.0)
        assert info["mean"] == mean and (info["threshold"] == thr or case == "n1")  # (n = 1: std = 0 / 0, checked below)
        assert np.array_equal(keep.astype(bool), R.sor_keep(ref, thr))
        if case == "n1":
            assert info["n_kept"] == 0 and math.isnan(info["threshold"])
        if case == "dup" and k <= 9:
            assert keep[-6:].sum() == 0  # nine copies of one point: all neighbours at d2 = 0


@pytest.mark.parametrize("n", [100_000, 1_000_000])
def test_ror_counts_bitwise(n):
    xyz = _scene(n)
    for radius, nb in ((0.1, 5), (0.05, 2)):
        ref = R.ror_counts(xyz, radius)
        with _engine() as e:
            e.upload(0, xyz, cell_size=0.1)
            info, counts, keep = e.radius_outlier(0, nb, radius, fetch=True)
        assert np.array_equal(counts, ref)
        assert np.array_equal(keep.astype(bool), ref > nb)
        assert info["n_kept"] == int((ref > nb).sum()) and info["threshold"] == nb


def test_ror_points_exactly_at_radius():
    # points 0.5 apart on a line: d2 == r^2 exactly is not counted (strict)
    xyz = np.stack([np.arange(20) * 0.5, np.zeros(20), np.zeros(20)], 1)
    with _engine() as e:
        e.upload(0, xyz)
        _, counts, _ = e.radius_outlier(0, 0, 0.5, fetch=True)
    assert np.array_equal(counts, R.brute_ror_counts(xyz, 0.5))
    assert np.all(counts == 1)


def test_select_in_place_and_into_other_context_agree():
    xyz = _scene(100_000)
    nrm = np.random.default_rng(3).standard_normal((len(xyz), 3))
    with _engine() as a, _engine() as b:
        a.upload(0, xyz, cell_size=0.1)
        a.set_normals(0, nrm)
        info, avg, keep = a.statistical_outlier(0, 20, 1.0, fetch=True)
        m = a.select_kept_into(0, b, 1)
        kept = xyz[keep.astype(bool)]
        assert m == info["n_kept"] == len(kept)
        assert np.array_equal(b.download(1), kept)
        assert np.array_equal(b.get_normals(1), nrm[keep.astype(bool)])
        assert np.array_equal(a.download(0), xyz)  # src untouched, its mask still usable
        n2, info2 = a.remove_statistical_outlier(0, 20, 1.0)
        assert n2 == m and info2 == info
        assert np.array_equal(a.download(0), kept)
        assert np.array_equal(a.get_normals(0), nrm[keep.astype(bool)])
        # radius: in place
        c_ref = R.ror_counts(kept, 0.1)
        n3, _ = a.remove_radius_outlier(0, 3, 0.1)
        assert n3 == int((c_ref > 3).sum())
        assert np.array_equal(a.download(0), kept[c_ref > 3])


def test_nn1_after_removal_matches_fresh_upload():
    est = _scene(100_000)
    from cloud_map_evaluation_amd import synth

    gt = synth.scan_pair(100_000, density=2500.0, seed=51)[1].numpy()
    with _engine() as a, _engine() as b:
        a.upload(0, est, cell_size=0.1)
        a.upload(1, gt, cell_size=0.1)
        a.remove_statistical_outlier(0, 20, 2.0)
        kept = a.download(0)
        b.upload(0, kept, cell_size=0.1)
        b.upload(1, gt, cell_size=0.1)
        for q, r in ((0, 1), (1, 0)):
            ia, da = a.nn1(q, r)
            ib, db = b.nn1(q, r)
            assert np.array_equal(ia, ib) and np.array_equal(da, db)


def test_error_paths():
    from cloud_map_evaluation_amd.engine import MapEvalError

    xyz = _scene(100_000)
    with _engine() as e:
        e.upload(0, xyz, cell_size=0.1)
        with pytest.raises(MapEvalError, match="no outlier mask"):
            e.select_kept_into(0)
        with pytest.raises(MapEvalError, match=r"\[1, 40\]"):
            e.statistical_outlier(0, 41, 2.0)
        with pytest.raises(MapEvalError):
            e.statistical_outlier(0, 20, 0.0)
        with pytest.raises(MapEvalError):
            e.radius_outlier(0, -1, 0.1)
        e.statistical_outlier(0, 1, 2.0)  # k = 1 keeps nothing: the selection refuses an empty cloud
        with pytest.raises(MapEvalError, match="keeps no point"):
            e.select_kept_into(0)
        e.voxel_downsample(0, 0.5)  # a change of the cloud drops the mask
        with pytest.raises(MapEvalError, match="no outlier mask"):
            e.select_kept_into(0)
    with _engine() as e:
        e.set_slab(0, float(xyz[:, 0].min()) - 1, float(np.median(xyz[:, 0])), 1.0)
        e.upload(0, xyz, cell_size=0.1)  # (the slab's points + halo)
        with pytest.raises(MapEvalError, match="slab"):
            e.statistical_outlier(0, 20, 2.0)
        with pytest.raises(MapEvalError, match="slab"):
            e.radius_outlier(0, 2, 0.1)


def _angle_deg(R_):
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R_) - 1.0) / 2.0))))


def _rot_z(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def test_coarse_align_with_outlier_filter():
    """The documented failure regime: sparse outliers at 1 m voxels (DESIGN.md 4.7 "Limit"); the statistical filter in front of the
    down-sample recovers the pose."""
    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Param

    est, gt = synth.scan_pair(5_000_000, outlier_ratio=0.001)
    est, gt = est.numpy(), gt.numpy()
    Tm = np.eye(4)
    Tm[:3, :3] = _rot_z(math.radians(135.0))
    Tm[:3, 3] = (12.0, -7.0, 1.5)
    est_m = est @ Tm[:3, :3].T + Tm[:3, 3]
    Ttrue = np.linalg.inv(Tm)
    c = est_m.mean(0)

    def err(T):
        dr = _angle_deg(T[:3, :3] @ Ttrue[:3, :3].T)
        dt = float(np.linalg.norm((T[:3, :3] @ c + T[:3, 3]) - (Ttrue[:3, :3] @ c + Ttrue[:3, 3])))
        return dr, dt

    with _engine() as e:
        e.upload(0, est_m, cell_size=0.1)
        e.upload(1, gt, cell_size=0.1)
        before = e.download(0)
        T0 = e.coarse_align(1.0, max_iterations=200_000)
        print("unfiltered coarse alignment: %.2f deg, %.3f m" % err(T0))
        T1 = e.coarse_align(1.0, max_iterations=200_000, outlier_nb_neighbors=20)
        print("filtered coarse alignment: %.2f deg, %.3f m; filter %s" % (*err(T1), e.last_coarse_outliers))
        dr, dt = err(T1)
        assert dr < 1.0 and dt < 0.5
        assert np.array_equal(e.download(0), before) and e.size(0) == len(est_m)  # the resident clouds are untouched
        e.transform_cloud(0, T1)
        T1f = e.performICPRegistration(1.0, method=2)["transformation"] @ T1
    with _engine() as e:  # GICP from the true pose: the coarse start converges to the same place
        e.upload(0, est_m, cell_size=0.1)
        e.upload(1, gt, cell_size=0.1)
        e.transform_cloud(0, Ttrue)
        T0f = e.performICPRegistration(1.0, method=2)["transformation"] @ Ttrue
    assert _angle_deg(T1f[:3, :3] @ T0f[:3, :3].T) < 0.01
    assert np.linalg.norm(T1f[:3, 3] - T0f[:3, 3]) < 1e-3
