"""The host's surface-error keys through --parse-config (the result lines and surface_error.txt need a device run:
tests/test_gpu_surface_host.py).  No GPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")

_BASE = """registration_methods: 2
icp_max_distance: 1.5
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
save_immediate_result: false
evaluate_mme: true
evaluate_gt_mme: true
evaluate_using_initial: true
nn_radius: 0.15
vmd_voxel_size: 3.0
downsample_size: 0.0
estimate_map_path: /nonexistent/est
gt_map_path: /nonexistent/gt.pcd
scene_name: s
enable_debug: false
"""


def _parse(tmp_path, extra, base=_BASE):
    cfg = tmp_path / "c.yaml"
    cfg.write_text(base + extra)
    return subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)


def test_defaults(tmp_path):
    r = _parse(tmp_path, "")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_surface_error"] is False and p["surface_gated"] is False
    assert p["normal_radius"] == 0.15 and p["normal_min_points"] == 5  # (nn_radius)
    assert p["surface_thresholds"] == [0.2, 0.1, 0.08, 0.05, 0.01]  # (the accuracy_level list)
    assert p["surface_angles_deg"] == [5, 10, 20]


def test_keys_are_read(tmp_path):
    r = _parse(tmp_path, "evaluate_surface_error: true\nnormal_radius: 0.25\nnormal_min_points: 8\nsurface_thresholds: [0.3, 0.0]\n"
                         "surface_angles_deg: [0, 45.5, 90]\nsurface_gated: true\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["evaluate_surface_error"], p["normal_radius"], p["normal_min_points"], p["surface_thresholds"], p["surface_angles_deg"],
            p["surface_gated"]) == (True, 0.25, 8, [0.3, 0], [0, 45.5, 90], True)
    assert _parse(tmp_path, "evaluate_surface_error: true\nsurface_thresholds: []\nsurface_angles_deg: []\n").returncode == 0
    assert _parse(tmp_path, "evaluate_surface_error: true\nsurface_angles_deg: [" + ", ".join(["5"] * 8) + "]\n").returncode == 0


def test_bad_values_and_combinations_are_refused(tmp_path):
    for extra, key in (("num_gpus: 2\n", "evaluate_surface_error: single GPU only (num_gpus must be 1)"),
                       ("normal_radius: 0\n", "normal_radius"),
                       ("normal_min_points: 1\n", "normal_min_points"),
                       ("surface_thresholds: [0.1, -0.2]\n", "surface_thresholds"),
                       ("surface_thresholds: [" + ", ".join(["0.1"] * 9) + "]\n", "surface_thresholds"),
                       ("surface_thresholds: 0.1\n", "surface_thresholds"),  # a scalar, not a list
                       ("surface_angles_deg: 5\n", "surface_angles_deg"),
                       ("surface_angles_deg: [5, 91]\n", "surface_angles_deg"),
                       ("surface_angles_deg: [-1]\n", "surface_angles_deg"),
                       ("surface_angles_deg: [" + ", ".join(["5"] * 9) + "]\n", "surface_angles_deg"),
                       ("evaluate_noised_gt: true\n", "evaluate_surface_error: not with evaluate_noised_gt")):
        r = _parse(tmp_path, "evaluate_surface_error: true\n" + extra)
        assert r.returncode != 0 and key in r.stderr, (extra, r.stderr)
    r = _parse(tmp_path, "evaluate_surface_error: true\n", _BASE.replace("evaluate_using_initial: true", "evaluate_using_initial: false"))
    assert r.returncode != 0 and "evaluate_surface_error: needs evaluate_using_initial" in r.stderr
    # the stage is off: its keys are not judged
    assert _parse(tmp_path, "evaluate_surface_error: false\nnum_gpus: 2\nnormal_min_points: 0\nsurface_angles_deg: [200]\n").returncode == 0


def test_shipped_reference_configs_keep_the_stage_off():
    ref_dir = os.path.join(ROOT, "tests", "golden", "reference_configs")
    for name in ("config.yaml", "config_building_day.yaml", "config_corridor.yaml", "config_geode.yaml"):
        r = subprocess.run([EXE, "--parse-config", os.path.join(ref_dir, name)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (name, r.stderr)
        assert json.loads(r.stdout)["evaluate_surface_error"] is False
