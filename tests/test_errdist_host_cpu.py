"""The host's error-distribution keys through --parse-config (the result lines and error_distribution.txt need a device run:
tests/test_gpu_errdist_host.py).  No GPU."""
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


def _parse(tmp_path, extra):
    cfg = tmp_path / "c.yaml"
    cfg.write_text(_BASE + extra)
    return subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)


def test_defaults(tmp_path):
    r = _parse(tmp_path, "")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_error_distribution"] is False and p["error_gated"] is False
    assert p["error_quantiles"] == [0.5, 0.9, 0.95, 0.99]
    assert p["error_thresholds"] == [0.2, 0.1, 0.08, 0.05, 0.01]  # (the accuracy_level list)
    assert p["error_cdf_bins"] == 1000 and p["error_cdf_max"] == 1.5  # (icp_max_distance)


def test_keys_are_read(tmp_path):
    r = _parse(tmp_path, "evaluate_error_distribution: true\nerror_quantiles: [0.25, 1.0, 0.0]\nerror_thresholds: [0.3, 0.0]\n"
                         "error_cdf_bins: 4096\nerror_cdf_max: 0.75\nerror_gated: true\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["evaluate_error_distribution"], p["error_quantiles"], p["error_thresholds"], p["error_cdf_bins"], p["error_cdf_max"],
            p["error_gated"]) == (True, [0.25, 1, 0], [0.3, 0], 4096, 0.75, True)
    assert _parse(tmp_path, "evaluate_error_distribution: true\nerror_cdf_bins: 0\nerror_quantiles: []\nerror_thresholds: []\n").returncode == 0
    assert _parse(tmp_path, "evaluate_error_distribution: true\nerror_quantiles: [" + ", ".join(["0.5"] * 16) + "]\n").returncode == 0


def test_bad_values_and_combinations_are_refused(tmp_path):
    for extra, key in (("num_gpus: 2\n", "evaluate_error_distribution: single GPU only (num_gpus must be 1)"),
                       ("error_quantiles: [" + ", ".join(["0.5"] * 17) + "]\n", "error_quantiles"),  # a 17th quantile
                       ("error_quantiles: [0.5, 1.5]\n", "error_quantiles"),
                       ("error_quantiles: [-0.1]\n", "error_quantiles"),
                       ("error_thresholds: [0.1, -0.2]\n", "error_thresholds"),
                       ("error_thresholds: [" + ", ".join(["0.1"] * 9) + "]\n", "error_thresholds"),
                       ("error_thresholds: 0.1\n", "error_thresholds"),  # a scalar, not a list
                       ("error_quantiles: 0.5\n", "error_quantiles"),
                       ("error_cdf_bins: 5000\n", "error_cdf_bins"),
                       ("error_cdf_bins: -1\n", "error_cdf_bins"),
                       ("error_cdf_max: 0\n", "error_cdf_max")):
        r = _parse(tmp_path, "evaluate_error_distribution: true\n" + extra)
        assert r.returncode != 0 and key in r.stderr, (extra, r.stderr)
    # the stage is off: its keys are not judged
    assert _parse(tmp_path, "evaluate_error_distribution: false\nnum_gpus: 2\nerror_cdf_bins: 5000\nerror_quantiles: [1.5]\n").returncode == 0


def test_shipped_reference_configs_keep_the_stage_off():
    ref_dir = os.path.join(ROOT, "tests", "golden", "reference_configs")
    for name in ("config.yaml", "config_building_day.yaml", "config_corridor.yaml", "config_geode.yaml"):
        r = subprocess.run([EXE, "--parse-config", os.path.join(ref_dir, name)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (name, r.stderr)
        assert json.loads(r.stdout)["evaluate_error_distribution"] is False
