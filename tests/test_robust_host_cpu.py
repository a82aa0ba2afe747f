"""The host's icp_robust_*, icp_multi_scale_* and icp_information_matrix keys through --parse-config: reading and refusals, and the shipped
reference configs still parse with the feature off."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")

_BASE = """registration_methods: 2
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
save_immediate_result: false
evaluate_mme: true
evaluate_gt_mme: true
evaluate_using_initial: false
nn_radius: 0.1
vmd_voxel_size: 3.0
downsample_size: 0.0
estimate_map_path: /nonexistent/est
gt_map_path: /nonexistent/gt.pcd
scene_name: s
enable_debug: false
"""
_LISTS = "icp_multi_scale_voxels: [0.4, 0.2, 0]\nicp_multi_scale_distances: [1.0, 0.5, 0.25]\nicp_multi_scale_iterations: [10, 10, 15]\n"


def _parse(tmp_path, extra, base=_BASE):
    cfg = tmp_path / "c.yaml"
    cfg.write_text(base + extra)
    return subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra", ["", "icp_robust_kernel: none\n", "icp_robust_kernel: l1\n", "icp_robust_kernel: tukey\nicp_robust_scale: 0.05\n",
                                   _LISTS, "icp_information_matrix: true\n",
                                   "icp_robust_kernel: huber\nicp_robust_scale: 0.1\n" + _LISTS + "icp_information_matrix: true\n"])
def test_accepted(tmp_path, extra):
    r = _parse(tmp_path, extra)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("extra,key", [
    ("icp_robust_kernel: tukey\n", "icp_robust_scale"),
    ("icp_robust_kernel: huber\n", "icp_robust_scale"),
    ("icp_robust_kernel: cauchy\n", "icp_robust_scale"),
    ("icp_robust_kernel: gm\n", "icp_robust_scale"),
    ("icp_robust_kernel: welsch\nicp_robust_scale: 0.1\n", "icp_robust_kernel"),
    ("icp_robust_kernel: tukey\nicp_robust_scale: 0\n", "icp_robust_scale"),
    ("icp_robust_kernel: tukey\nicp_robust_scale: -1\n", "icp_robust_scale"),
    ("icp_multi_scale_voxels: [0.4, 0.2]\n", "icp_multi_scale"),
    ("icp_multi_scale_voxels: [0.4, 0.2]\nicp_multi_scale_distances: [1.0, 0.5]\n", "icp_multi_scale"),
    ("icp_multi_scale_voxels: [0.4, 0.2]\nicp_multi_scale_distances: [1.0, 0.5, 0.2]\nicp_multi_scale_iterations: [5, 5]\n", "icp_multi_scale"),
    ("icp_multi_scale_voxels: [0.4]\nicp_multi_scale_distances: [0]\nicp_multi_scale_iterations: [5]\n", "icp_multi_scale"),
    ("icp_robust_kernel: l1\nnum_gpus: 2\n", "icp_robust_kernel"),
    (_LISTS + "num_gpus: 2\n", "icp_multi_scale_voxels"),
    ("icp_information_matrix: true\nnum_gpus: 2\n", "icp_information_matrix"),
])
def test_refused(tmp_path, extra, key):
    r = _parse(tmp_path, extra)
    assert r.returncode != 0
    assert key in r.stderr


@pytest.mark.parametrize("extra,key", [("icp_robust_kernel: l1\n", "icp_robust_kernel"), (_LISTS, "icp_multi_scale_voxels"),
                                       ("icp_information_matrix: true\n", "icp_information_matrix")])
def test_refused_on_the_initial_matrix_path(tmp_path, extra, key):
    base = _BASE.replace("evaluate_using_initial: false", "evaluate_using_initial: true")
    r = _parse(tmp_path, extra, base)
    assert r.returncode != 0 and key in r.stderr and "evaluate_using_initial" in r.stderr
    assert _parse(tmp_path, "icp_robust_kernel: none\nicp_information_matrix: false\n", base).returncode == 0


def test_shipped_reference_configs_still_parse():
    ref_dir = os.path.join(ROOT, "tests", "golden", "reference_configs")
    for name in ("config.yaml", "config_building_day.yaml", "config_corridor.yaml", "config_geode.yaml"):
        r = subprocess.run([EXE, "--parse-config", os.path.join(ref_dir, name)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (name, r.stderr)
