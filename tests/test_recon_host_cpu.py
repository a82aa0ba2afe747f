"""The C++ host's evaluate_mesh keys through --parse-config: the defaults, the values read, and refusals that name the key.  No GPU."""
import json
import os
import subprocess

from test_mesh_host_cpu import _BASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")


def _parse(tmp_path, extra):
    cfg = tmp_path / "c.yaml"
    cfg.write_text(_BASE + extra)
    return subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)


def test_defaults(tmp_path):
    r = _parse(tmp_path, "")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_mesh"] is False and p["mesh_voxel_size"] == 0 and p["mesh_min_points"] == 8 and p["mesh_band"] == 1
    assert p["mesh_normal_radius"] == p["nn_radius"] == 0.15 and p["mesh_viewpoint"] is None
    r = _parse(tmp_path, "evaluate_mesh: true\nmesh_voxel_size: 0.05\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_mesh"] is True and p["mesh_voxel_size"] == 0.05 and p["mesh_radius"] == 3.0 * 0.05
    assert p["mesh_normal_radius"] == 0.15 and p["mesh_viewpoint"] is None and p["evaluate_mesh_distance"] is False


def test_keys_are_read(tmp_path):
    r = _parse(tmp_path, "evaluate_mesh: true\nmesh_voxel_size: 0.1\nmesh_radius: 0.25\nmesh_min_points: 5\nmesh_band: 2\n"
                         "mesh_normal_radius: 0.4\nmesh_viewpoint: [1.5, -2, 30]\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["mesh_voxel_size"], p["mesh_radius"], p["mesh_min_points"], p["mesh_band"], p["mesh_normal_radius"], p["mesh_viewpoint"]) == (
        0.1, 0.25, 5, 2, 0.4, [1.5, -2.0, 30.0])
    # the map against the reconstructed ground truth: no gt_mesh_path needed
    r = _parse(tmp_path, "evaluate_mesh: true\nmesh_voxel_size: 0.1\nevaluate_mesh_distance: true\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_mesh_distance"] is True and p["gt_mesh_path"] == ""


def test_refusals_name_the_key(tmp_path):
    ok = "evaluate_mesh: true\nmesh_voxel_size: 0.1\n"
    for extra, key in (("evaluate_mesh: true\n", "mesh_voxel_size: required with evaluate_mesh"),
                       ("evaluate_mesh: true\nmesh_voxel_size: 0\n", "mesh_voxel_size"),
                       ("evaluate_mesh: true\nmesh_voxel_size: -1\n", "mesh_voxel_size"),
                       (ok + "mesh_radius: 0.05\n", "mesh_radius"),
                       (ok + "mesh_min_points: 0\n", "mesh_min_points"),
                       (ok + "mesh_band: 3\n", "mesh_band"),
                       (ok + "mesh_band: -1\n", "mesh_band"),
                       (ok + "mesh_normal_radius: 0\n", "mesh_normal_radius"),
                       (ok + "mesh_viewpoint: [1, 2]\n", "mesh_viewpoint"),
                       (ok + "mesh_viewpoint: 3\n", "mesh_viewpoint"),
                       (ok + "num_gpus: 2\n", "evaluate_mesh: single GPU only (num_gpus must be 1)"),
                       ("evaluate_mesh: false\nevaluate_mesh_distance: true\n", "gt_mesh_path"),
                       ("evaluate_mesh_distance: true\n", "gt_mesh_path")):
        r = _parse(tmp_path, extra)
        assert r.returncode != 0 and key in r.stderr, (extra, r.stderr)
    # with the stage off nothing of it is judged
    assert _parse(tmp_path, "evaluate_mesh: false\nnum_gpus: 2\nmesh_band: 9\nmesh_radius: -1\n").returncode == 0
