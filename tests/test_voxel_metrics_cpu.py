"""me_voxel_metrics without a GPU: the entry point is declared, exported and bound; the host's save_voxel_metrics key; the
numpy group-by the GPU tests take as their expectation (tests/_voxel_metrics_ref.py) against a plain loop."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _voxel_metrics_ref as ref  # noqa: E402

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
CONFIG = """registration_methods: 2
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix:
  - [1.0, 0.0, 0.0, 0.0]
  - [0.0, 1.0, 0.0, 0.0]
  - [0.0, 0.0, 1.0, 0.0]
  - [0.0, 0.0, 0.0, 1.0]
estimate_map_path: /a
gt_map_path: /b.pcd
scene_name: unit_test
save_immediate_result: true
evaluate_mme: true
use_tbb_mme: true
evaluate_gt_mme: true
nn_radius: 0.1
evaluate_using_initial: true
evaluate_noise_gt: false
vmd_voxel_size: 3.0
downsample_size: 0.0
use_visualization: false
enable_debug: false
"""


def test_entry_point_is_declared_exported_and_bound():
    from cloud_map_evaluation_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "mapeval_hip.h")).read()
    assert "int me_voxel_metrics(me_ctx *ctx, int slot, double voxel_size, double gate, int gate_mode, const double trunc[5]," in hdr
    assert "me_voxel_metrics" in _lib.SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "me_voxel_metrics")
    L = _lib.load()
    assert L.me_voxel_metrics.restype is ctypes.c_int and len(L.me_voxel_metrics.argtypes) == 12
    assert _lib.NN_PARTIAL_DTYPE.itemsize == ctypes.sizeof(_lib.NNPartial) == 144


def test_joined_table_has_44_columns():
    from cloud_map_evaluation_amd.engine import VOXEL_METRICS_COLUMNS

    assert len(VOXEL_METRICS_COLUMNS) == 44 and len(set(VOXEL_METRICS_COLUMNS)) == 44
    assert VOXEL_METRICS_COLUMNS[:5] == ["ix", "iy", "iz", "n_est", "n_gt"] and VOXEL_METRICS_COLUMNS[-1] == "w2"


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.dirname(EXE), "-s"])
    return EXE


def _parse(exe, tmp_path, extra):
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + extra)
    return subprocess.run([exe, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=120)


def test_parse_config_reports_save_voxel_metrics(exe, tmp_path):
    r = _parse(exe, tmp_path, "")
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["save_voxel_metrics"] is False  # default
    r = _parse(exe, tmp_path, "save_voxel_metrics: true\n")
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["save_voxel_metrics"] is True
    r = _parse(exe, tmp_path, "save_voxel_metrics: true\nnum_gpus: 1\n")
    assert r.returncode == 0 and json.loads(r.stdout)["save_voxel_metrics"] is True


def test_save_voxel_metrics_with_several_gpus_is_refused(exe, tmp_path):
    r = _parse(exe, tmp_path, "save_voxel_metrics: true\nnum_gpus: 2\n")
    assert r.returncode != 0 and "Failed to load configuration" in r.stderr and "save_voxel_metrics" in r.stderr
    r = _parse(exe, tmp_path, "save_voxel_metrics: false\nnum_gpus: 2\n")
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("gate_mode", [ref.GATE_LE_UNSQUARED, ref.GATE_LT_SQUARED])
@pytest.mark.parametrize("vs", [0.5, 1.0, 3.0])
def test_numpy_group_by_matches_a_plain_loop(gate_mode, vs):
    rng = np.random.default_rng(int(vs * 10) + gate_mode)
    n = 3000
    xyz = rng.uniform(-4.0, 4.0, (n, 3))
    xyz[:200] = np.round(xyz[:200] / vs) * vs  # points exactly on voxel faces (multiples of vs), negative ones included
    xyz[200:210] = [-vs, 0.0, vs]
    d2 = rng.exponential(0.05, n)
    d2[:50] = [0.2 ** 2, 0.1 ** 2, 0.08 ** 2, 0.05 ** 2, 0.01 ** 2] * 10  # distances exactly at the thresholds
    d2[50:60] = 0.3  # exactly at the gate (LE_UNSQUARED keeps them, LT_SQUARED with 0.3^2 does not)
    ent = rng.normal(-2.0, 1.5, n)
    valid = rng.random(n) < 0.7
    ent[~valid] = 0.0
    trunc = (0.2, 0.1, 0.08, 0.05, 0.01)
    got = ref.group(xyz, d2, vs, 0.3, gate_mode, trunc, ent, valid)
    want = ref.brute_force(xyz, d2, vs, 0.3, gate_mode, trunc, ent, valid)
    ref.assert_rows_equal(got, want)
    assert got["n_query"].sum() == n and got["n_H"].sum() == valid.sum()
    assert np.any(got["keys"] < 0)
    # the voxel index is floor(x / vs): a point at -vs lies in voxel -1, one at 0 in voxel 0
    assert (-1, 0, 1) in {tuple(k) for k in got["keys"]}


def test_t2max_is_the_largest_square_at_or_below_the_threshold():
    import math

    for t in (0.2, 0.1, 0.08, 0.05, 0.01, 1.0, 0.0):
        x = ref.t2max(t)
        assert math.sqrt(x) <= t and math.sqrt(float(np.nextafter(x, np.inf))) > t
    assert ref.t2max(-1.0) == -1.0
