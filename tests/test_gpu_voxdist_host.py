"""The C++ host's evaluate_voxel_distances on the MI355X: the two result lines and voxel_distances.txt equal Engine.voxel_distances on the
same pair, and a configuration without the key (or with it false) writes exactly what it wrote before."""
import numpy as np
import pytest

from test_gpu_recon_host import _SKIP, _run, scene  # noqa: F401  (the pair of the reconstruction host test, its config and runner)

pytestmark = pytest.mark.gpu

VS, NN_RADIUS = 2.0, 0.5  # _run's config: vmd_voxel_size, nn_radius (the default bandwidth)
MMD, GAUSS = "VoxelMMD @", "VoxelKL-BD-W2: "


def _engine(scene, sigmas, max_points, floor):
    from cloud_map_evaluation_amd.engine import Engine, Param

    est, gt = scene
    T = np.eye(4)
    T[2, 3] = 0.02  # _run's initial_matrix
    with Engine(0) as e:
        e.run_suite_from(est, gt, Param(icp_max_distance_=1.0, nn_radius_=0.5, vmd_voxel_size_=2.0, initial_matrix_=T))
        return e.voxel_distances(VS, sigmas, min_pts=100, max_points=max_points, eig_floor=floor)


def _check(out, want, sigmas, max_points):
    lines = open(out / "map_results.txt").read().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith(MMD)]
    assert len(at) == 1 and lines[at[0] + 1].startswith(GAUSS) and lines[at[0] + 2].startswith("VMD: ")
    head, figures = lines[at[0]][len(MMD):].split(":")
    assert head == ",".join(f"{s:.15f}" for s in sigmas)
    assert figures.split() == [f"{x:.15f}" for b in range(len(sigmas)) for x in (want["mean_mmd"][b], want["mean_mmd2_u"][b])]
    assert lines[at[0] + 1][len(GAUSS):].split() == [f"{want[k]:.15f}" for k in ("mean_kl_est_gt", "mean_kl_gt_est", "mean_bhattacharyya", "mean_w2")]
    rows = [ln.split() for ln in open(out / "voxel_distances.txt").read().splitlines()]
    nh = 5 + len(sigmas) + 3
    head, rows = dict((h[0], h[1]) for h in rows[:nh] if h[0] != "sigma"), np.array(rows[nh:], np.float64)
    assert int(head["n_rows"]) == want["n_rows"] == rows.shape[0] > 0 and int(head["max_points"]) == max_points
    assert int(head["n_pairs"]) == want["n_pairs_total"] and int(head["n_rows_subsampled"]) == want["n_rows_subsampled"]
    assert rows.shape[1] == 11 + 5 * len(sigmas)
    np.testing.assert_array_equal(rows[:, 0:3], want["keys"])
    np.testing.assert_array_equal(rows[:, 3:5], want["n_pop"])
    np.testing.assert_array_equal(rows[:, 5:7], want["n_used"])
    np.testing.assert_array_equal(rows[:, 7:11], np.column_stack([want["kl_est_gt"], want["kl_gt_est"], want["bhattacharyya"], want["w2"]]))
    for b in range(len(sigmas)):
        np.testing.assert_array_equal(rows[:, 11 + 5 * b:14 + 5 * b], want["ksum"][:, b, :])
        np.testing.assert_array_equal(rows[:, 14 + 5 * b], want["mmd2_u"][:, b])
        np.testing.assert_array_equal(rows[:, 15 + 5 * b], want["mmd2_b"][:, b])


def test_lines_and_file_equal_the_engine(scene, tmp_path):
    out = _run(tmp_path, "on", scene, "evaluate_voxel_distances: true\n")
    _check(out, _engine(scene, [NN_RADIUS], 2048, 1e-6), [NN_RADIUS], 2048)
    out = _run(tmp_path, "keys", scene, "evaluate_voxel_distances: true\nmmd_sigmas: [0.25, 1.0]\nmmd_max_points: 128\nvoxel_distance_eig_floor: 1e-4\n")
    _check(out, _engine(scene, [0.25, 1.0], 128, 1e-4), [0.25, 1.0], 128)


def test_without_the_key_nothing_changes(scene, tmp_path):
    off = _run(tmp_path, "off", scene)
    false = _run(tmp_path, "false", scene, "evaluate_voxel_distances: false\nmmd_sigmas: [0.25]\nmmd_max_points: 64\n")
    on = _run(tmp_path, "on", scene, "evaluate_voxel_distances: true\n")
    names_off = sorted(p.name for p in off.iterdir())
    assert sorted(p.name for p in false.iterdir()) == names_off and "voxel_distances.txt" not in names_off
    assert sorted(p.name for p in on.iterdir()) == sorted(names_off + ["voxel_distances.txt"])
    keep = lambda folder: [ln for ln in open(folder / "map_results.txt").read().splitlines() if not any(s in ln for s in _SKIP)]  # noqa: E731
    assert keep(false) == keep(off) == [ln for ln in keep(on) if not ln.startswith((MMD, GAUSS))]
    assert "VoxelMMD" not in open(off / "map_results.txt").read() and "VoxelKL" not in open(false / "map_results.txt").read()
    for name in names_off:
        if name != "map_results.txt":
            assert (false / name).read_bytes() == (off / name).read_bytes(), name
            assert (on / name).read_bytes() == (off / name).read_bytes(), name
