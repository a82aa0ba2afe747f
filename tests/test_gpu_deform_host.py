"""The C++ host's evaluate_deformation on the MI355X: the result line and deformation_field.txt equal Engine.deformation_field on the
same pair, and a configuration without the key writes exactly the bytes it wrote before."""
import numpy as np
import pytest

from test_gpu_recon_host import _SKIP, _run, scene  # noqa: F401  (the pair of the reconstruction host test, its config and runner)

pytestmark = pytest.mark.gpu

VS, MAX_D, MIN_PAIRS = 2.0, 1.0, 30  # the defaults under _run's config: vmd_voxel_size, sqrt(icp_max_distance), 30 (min_spread = VS / 20)
LINE = "Deformation mean-rms-max share_t-share_R: "


def _engine_field(scene, vs, max_d, min_pairs, min_spread=None):
    from cloud_map_evaluation_amd.engine import Engine, Param

    est, gt = scene
    T = np.eye(4)
    T[2, 3] = 0.02  # _run's initial_matrix
    with Engine(0) as e:
        e.run_suite_from(est, gt, Param(icp_max_distance_=1.0, nn_radius_=0.5, vmd_voxel_size_=2.0, initial_matrix_=T))
        return e.deformation_field(0, vs, max_d, min_pairs=min_pairs, min_spread=min_spread)


def _check(out, want):
    lines = open(out / "map_results.txt").read().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith(LINE)]
    assert len(at) == 1 and lines[at[0] + 1].startswith("VMD: ")
    figures = [want["mean_disp"], want["rms_disp"], want["max_disp"], want["share_translation"], want["share_rigid"]]
    assert lines[at[0]][len(LINE):].split() == [f"{x:.15f}" for x in figures]
    rows = [ln.split() for ln in open(out / "deformation_field.txt").read().splitlines()]
    head, rows = rows[:4], np.array(rows[4:], np.float64)
    assert [h[0] for h in head] == ["voxel_size", "max_distance", "min_pairs", "min_spread"]
    has = want["n_pairs"] > 0
    assert rows.shape == (int(has.sum()), 15) and has.sum() > 0
    np.testing.assert_array_equal(rows[:, 0:3], want["keys"][has])
    np.testing.assert_array_equal(rows[:, 3], want["n_pairs"][has])
    np.testing.assert_array_equal(rows[:, 4], want["flags"][has])
    np.testing.assert_array_equal(rows[:, 5:8], want["t0"][has])
    np.testing.assert_array_equal(rows[:, 8:11], want["u"][has])
    np.testing.assert_allclose(rows[:, 11], want["angle"][has], rtol=0, atol=4e-16)  # (atan2 and sqrt of two libraries)
    np.testing.assert_array_equal(rows[:, 12:15], np.column_stack([want["e0"], want["e_t"], want["e_R"]])[has])
    return head


def test_line_and_file_equal_the_engine(scene, tmp_path):
    out = _run(tmp_path, "on", scene, "evaluate_deformation: true\n")
    want = _engine_field(scene, VS, MAX_D, MIN_PAIRS)
    head = _check(out, want)
    assert [float(h[1]) for h in head] == [VS, MAX_D, MIN_PAIRS, VS / 20.0]
    assert want["n_fit"] > 0 and want["n_rot"] > 0
    out = _run(tmp_path, "keys", scene, "evaluate_deformation: true\ndeformation_voxel_size: 1.0\ndeformation_max_distance: 0.05\n"
                                        "deformation_min_pairs: 50\ndeformation_min_spread: 0.1\n")
    head = _check(out, _engine_field(scene, 1.0, 0.05, 50, 0.1))
    assert [float(h[1]) for h in head] == [1.0, 0.05, 50, 0.1]


def test_without_the_key_nothing_changes(scene, tmp_path):
    off = _run(tmp_path, "off", scene)
    false = _run(tmp_path, "false", scene, "evaluate_deformation: false\ndeformation_voxel_size: 1.0\n")
    on = _run(tmp_path, "on", scene, "evaluate_deformation: true\n")
    names_off = sorted(p.name for p in off.iterdir())
    assert sorted(p.name for p in false.iterdir()) == names_off and "deformation_field.txt" not in names_off
    assert sorted(p.name for p in on.iterdir()) == sorted(names_off + ["deformation_field.txt"])
    keep = lambda folder: [ln for ln in open(folder / "map_results.txt").read().splitlines() if not any(s in ln for s in _SKIP)]  # noqa: E731
    assert keep(false) == keep(off) == [ln for ln in keep(on) if not ln.startswith(LINE)]
    assert "Deformation" not in open(off / "map_results.txt").read()
    for name in names_off:
        if name != "map_results.txt":
            assert (false / name).read_bytes() == (off / name).read_bytes(), name
            assert (on / name).read_bytes() == (off / name).read_bytes(), name
