"""The C++ host's evaluate_voxel_transport on the MI355X: the two result lines and voxel_transport.txt equal Engine.voxel_transport on the
same pair, replayed with the directions and the schedule the file lists, and a configuration without the key (or with it false) writes
exactly what it wrote before."""
import numpy as np
import pytest

from test_gpu_recon_host import _SKIP, _run, scene  # noqa: F401  (the pair of the reconstruction host test, its config and runner)

pytestmark = pytest.mark.gpu

VS, NN_RADIUS = 2.0, 0.5  # _run's config: vmd_voxel_size, nn_radius (the default blur)
SW2, SINK = "VoxelSW2 mean-max: ", "VoxelSinkhorn @"


def _engine(scene, dirs, eps, max_points):
    from cloud_map_evaluation_amd.engine import Engine, Param

    est, gt = scene
    T = np.eye(4)
    T[2, 3] = 0.02  # _run's initial_matrix
    with Engine(0) as e:
        e.run_suite_from(est, gt, Param(icp_max_distance_=1.0, nn_radius_=0.5, vmd_voxel_size_=2.0, initial_matrix_=T))
        return e.voxel_transport(VS, directions=dirs if len(dirs) else 0, eps_schedule=eps, min_pts=100, max_points=max_points)


def _check(out, scene, blur, n_dir, max_points, scaling):
    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import transport_schedule

    lines = [ln.split() for ln in open(out / "voxel_transport.txt").read().splitlines()]
    dirs = np.array([ln[1:] for ln in lines if ln[0] == "direction"], np.float64).reshape(-1, 3)
    eps = np.array([ln[1] for ln in lines if ln[0] == "eps"], np.float64)
    nh = 13 + len(dirs) + len(eps)
    head = dict((h[0], h[1]) for h in lines[:nh] if h[0] not in ("direction", "eps"))
    rows = np.array(lines[nh:], np.float64)
    # the parameters, the host's own schedule (the engine's arithmetic) and its direction table (the engine's to an ulp of the trigonometry)
    assert (float(head["voxel_size"]), int(head["min_pts"]), int(head["max_points"]), float(head["blur"]), float(head["scaling"])) == \
        (VS, 100, max_points, blur, scaling)
    assert (int(head["n_final"]), int(head["n_dir"]), int(head["n_eps"])) == (128, n_dir, len(eps)) and len(dirs) == n_dir
    assert eps.tobytes() == transport_schedule(VS, blur, scaling, 128).tobytes()
    if n_dir:
        assert np.abs(dirs - synth.fibonacci_directions(n_dir)).max() <= 4 * 2.0 ** -52
    want = _engine(scene, dirs, eps, max_points)
    assert int(head["n_rows"]) == want["n_rows"] == rows.shape[0] > 0 and rows.shape[1] == 17
    assert int(head["n_pairs"]) == want["n_pairs_total"] and int(head["n_rows_subsampled"]) == want["n_rows_subsampled"]
    assert float(head["max_marginal_err"]) == want["max_marginal_err"] and int(head["max_marginal_row"]) == want["max_marginal_row"]
    np.testing.assert_array_equal(rows[:, 0:3], want["keys"])
    np.testing.assert_array_equal(rows[:, 3:5], want["n_pop"])
    np.testing.assert_array_equal(rows[:, 5:7], want["n_used"])
    cols = ("sw2_sq", "sw2", "max_sw2_sq", "max_dir", "ot_xy", "ot_xx", "ot_yy", "s", "sinkhorn", "marginal_err")
    np.testing.assert_array_equal(rows[:, 7:17], np.column_stack([want[k] for k in cols]))  # (NaN equals NaN here: no sliced part)
    res = open(out / "map_results.txt").read().splitlines()
    at = [i for i, ln in enumerate(res) if ln.startswith(SW2)]
    assert len(at) == 1 and res[at[0] + 1].startswith(SINK) and res[at[0] + 2].startswith("VMD: ")
    assert res[at[0]][len(SW2):].split() == [f"{want[k]:.15f}" for k in ("mean_sw2", "mean_max_sw2")]
    head_blur, figures = res[at[0] + 1][len(SINK):].split(":")
    assert head_blur == f"{blur:.15f}"
    assert figures.split() == [f"{want[k]:.15f}" for k in ("mean_s", "mean_sinkhorn", "mean_marginal_err")]
    return res, at[0]


def test_lines_and_file_equal_the_engine(scene, tmp_path):
    out = _run(tmp_path, "on", scene, "evaluate_voxel_transport: true\n")
    _check(out, scene, NN_RADIUS, 32, 512, 0.5)
    out = _run(tmp_path, "keys", scene, "evaluate_voxel_transport: true\ntransport_blur: 0.8\ntransport_directions: 5\ntransport_max_points: 64\n"
                                        "transport_scaling: 0.7\n")
    _check(out, scene, 0.8, 5, 64, 0.7)
    # after the lines of evaluate_voxel_distances when both are on; no directions: no sliced part
    out = _run(tmp_path, "both", scene, "evaluate_voxel_transport: true\nevaluate_voxel_distances: true\ntransport_directions: 0\ntransport_max_points: 64\n")
    res, at = _check(out, scene, NN_RADIUS, 0, 64, 0.5)
    assert res[at - 2].startswith("VoxelMMD @") and res[at - 1].startswith("VoxelKL-BD-W2: ") and "nan" in res[at].lower()


def test_without_the_key_nothing_changes(scene, tmp_path):
    off = _run(tmp_path, "off", scene)
    false = _run(tmp_path, "false", scene, "evaluate_voxel_transport: false\ntransport_blur: 0.3\ntransport_directions: 7\ntransport_max_points: 64\n")
    on = _run(tmp_path, "on", scene, "evaluate_voxel_transport: true\ntransport_max_points: 64\n")
    names_off = sorted(p.name for p in off.iterdir())
    assert sorted(p.name for p in false.iterdir()) == names_off and "voxel_transport.txt" not in names_off
    assert sorted(p.name for p in on.iterdir()) == sorted(names_off + ["voxel_transport.txt"])
    keep = lambda folder: [ln for ln in open(folder / "map_results.txt").read().splitlines() if not any(s in ln for s in _SKIP)]  # noqa: E731
    assert keep(false) == keep(off) == [ln for ln in keep(on) if not ln.startswith((SW2, SINK))]
    assert "VoxelSW2" not in open(off / "map_results.txt").read() and "VoxelSinkhorn" not in open(false / "map_results.txt").read()
    for name in names_off:
        if name != "map_results.txt":
            assert (false / name).read_bytes() == (off / name).read_bytes(), name
            assert (on / name).read_bytes() == (off / name).read_bytes(), name
