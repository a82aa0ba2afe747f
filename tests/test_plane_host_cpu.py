"""The host's plane-segmentation keys through --parse-config (the result lines themselves need a device run:
tests/test_gpu_plane_host.py).  No GPU."""
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
    assert p["segment_planes"] is False and p["plane_distance_threshold"] == 0.05 and p["plane_num_iterations"] == 1000
    assert p["plane_max_planes"] == 8 and p["plane_min_inliers"] == 1000 and p["plane_seed"] == 0 and p["plane_refit"] is True
    assert p["segment_gt_planes"] is True
    p = json.loads(_parse(tmp_path, "segment_planes: true\n", gt_mme="false").stdout)
    assert p["segment_planes"] is True and p["segment_gt_planes"] is False  # (follows evaluate_gt_mme)


def test_keys_are_read(tmp_path):
    r = _parse(tmp_path, "segment_planes: true\nplane_distance_threshold: 0.125\nplane_num_iterations: 250\nplane_max_planes: 3\n"
                         "plane_min_inliers: 40\nplane_seed: 77\nplane_refit: false\nsegment_gt_planes: false\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["segment_planes"], p["plane_distance_threshold"], p["plane_num_iterations"], p["plane_max_planes"], p["plane_min_inliers"],
            p["plane_seed"], p["plane_refit"], p["segment_gt_planes"]) == (True, 0.125, 250, 3, 40, 77, False, False)
    r = _parse(tmp_path, "remove_outliers: plane\nplane_min_inliers: 10\n")
    assert r.returncode == 0 and json.loads(r.stdout)["remove_outliers"] == "plane"


def test_bad_values_and_combinations_are_refused(tmp_path):
    for head in ("segment_planes: true\n", "remove_outliers: plane\n"):
        for extra, key in (("plane_distance_threshold: 0\n", "plane_distance_threshold"),
                           ("plane_distance_threshold: -0.05\n", "plane_distance_threshold"),
                           ("plane_num_iterations: 0\n", "plane_num_iterations"),
                           ("plane_max_planes: 0\n", "plane_max_planes"),
                           ("plane_max_planes: 65\n", "plane_max_planes"),
                           ("plane_min_inliers: 2\n", "plane_min_inliers")):
            r = _parse(tmp_path, head + extra)
            assert r.returncode != 0 and key in r.stderr, (head, extra, r.stderr)
    r = _parse(tmp_path, "segment_planes: true\nnum_gpus: 2\n")
    assert r.returncode != 0 and "segment_planes: single GPU only (num_gpus must be 1)" in r.stderr
    r = _parse(tmp_path, "remove_outliers: plane\nnum_gpus: 2\n")
    assert r.returncode != 0 and "single GPU only" in r.stderr
    assert _parse(tmp_path, "segment_planes: false\nnum_gpus: 2\nplane_distance_threshold: 0\n").returncode == 0  # (the stage is off)


def test_shipped_reference_configs_keep_the_stage_off():
    ref_dir = os.path.join(ROOT, "tests", "golden", "reference_configs")
    for name in ("config.yaml", "config_building_day.yaml", "config_corridor.yaml", "config_geode.yaml"):
        r = subprocess.run([EXE, "--parse-config", os.path.join(ref_dir, name)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (name, r.stderr)
        assert json.loads(r.stdout)["segment_planes"] is False
