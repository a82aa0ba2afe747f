"""The host's MOM keys through --parse-config (the result line and mom.txt need a device run: tests/test_gpu_mom_host.py).  No GPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")

_BASE = """registration_methods: 2
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
save_immediate_result: false
evaluate_mme: true
evaluate_gt_mme: %s
evaluate_using_initial: true
nn_radius: 0.15
vmd_voxel_size: 3.0
downsample_size: 0.0
estimate_map_path: /nonexistent/est
gt_map_path: /nonexistent/gt.pcd
scene_name: s
enable_debug: false
"""


def _parse(tmp_path, extra, gt_mme="true"):
    cfg = tmp_path / "c.yaml"
    cfg.write_text(_BASE % gt_mme + extra)
    return subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)


def test_defaults(tmp_path):
    r = _parse(tmp_path, "")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_mom"] is False and p["mom_parallel_deg"] == 10 and p["mom_orthogonal_deg"] == 10 and p["mom_min_axis_points"] == 1000
    assert p["evaluate_gt_mom"] is True
    p = json.loads(_parse(tmp_path, "evaluate_mom: true\n", gt_mme="false").stdout)
    assert p["evaluate_mom"] is True and p["evaluate_gt_mom"] is False  # (follows evaluate_gt_mme)
    assert p["evaluate_mpv"] is False and p["segment_planes"] is False  # (MOM runs its inputs itself: their own stages stay off)
    assert p["mpv_radius"] == 0.15  # (the radius of its eigenvalues: mpv_radius, by default nn_radius)


def test_keys_are_read(tmp_path):
    r = _parse(tmp_path, "evaluate_mom: true\nmom_parallel_deg: 7.5\nmom_orthogonal_deg: 12\nmom_min_axis_points: 250\nevaluate_gt_mom: false\n"
                         "mpv_radius: 0.3\nmpv_min_points: 8\nplane_max_planes: 12\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["evaluate_mom"], p["mom_parallel_deg"], p["mom_orthogonal_deg"], p["mom_min_axis_points"], p["evaluate_gt_mom"]) == \
        (True, 7.5, 12, 250, False)
    assert (p["mpv_radius"], p["mpv_min_points"], p["plane_max_planes"]) == (0.3, 8, 12)


def test_bad_values_and_combinations_are_refused(tmp_path):
    for extra, key in (("mom_parallel_deg: -1\n", "mom_parallel_deg"),
                       ("mom_parallel_deg: 90\n", "mom_parallel_deg"),
                       ("mom_orthogonal_deg: -0.5\n", "mom_orthogonal_deg"),
                       ("mom_orthogonal_deg: 90\n", "mom_orthogonal_deg"),
                       ("mom_parallel_deg: 50\nmom_orthogonal_deg: 40\n", "mom_parallel_deg + mom_orthogonal_deg"),
                       ("mom_min_axis_points: 0\n", "mom_min_axis_points"),
                       # the keys of its two inputs are checked although their own stages are off
                       ("mpv_radius: 0\n", "mpv_radius"),
                       ("mpv_min_points: 1\n", "mpv_min_points"),
                       ("plane_distance_threshold: 0\n", "plane_distance_threshold"),
                       ("plane_num_iterations: 0\n", "plane_num_iterations"),
                       ("plane_max_planes: 65\n", "plane_max_planes"),
                       ("plane_min_inliers: 2\n", "plane_min_inliers")):
        r = _parse(tmp_path, "evaluate_mom: true\n" + extra)
        assert r.returncode != 0 and key in r.stderr, (extra, r.stderr)
    r = _parse(tmp_path, "evaluate_mom: true\nnum_gpus: 2\n")
    assert r.returncode != 0 and "evaluate_mom: single GPU only (num_gpus must be 1)" in r.stderr
    assert _parse(tmp_path, "evaluate_mom: false\nnum_gpus: 2\nmom_parallel_deg: 95\nmom_min_axis_points: 0\n").returncode == 0  # (the stage is off)
    assert _parse(tmp_path, "evaluate_mom: true\nmom_parallel_deg: 0\nmom_orthogonal_deg: 0\n").returncode == 0  # (exact directions)


def test_shipped_reference_configs_keep_the_stage_off():
    ref_dir = os.path.join(ROOT, "tests", "golden", "reference_configs")
    for name in ("config.yaml", "config_building_day.yaml", "config_corridor.yaml", "config_geode.yaml"):
        r = subprocess.run([EXE, "--parse-config", os.path.join(ref_dir, name)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (name, r.stderr)
        assert json.loads(r.stdout)["evaluate_mom"] is False
