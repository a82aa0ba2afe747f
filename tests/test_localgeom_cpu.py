"""The numpy / scipy model of me_local_geometry (tests/_localgeom_ref.py) pinned without a device — against O(N^2) brute force and on
analytic shapes — the binding's struct, and the host's evaluate_mpv keys through --parse-config (the result lines themselves need a
device run: tests/test_gpu_localgeom_host.py)."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np

import _localgeom_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")


def test_model_against_brute_force_2000():
    rng = np.random.default_rng(7)
    # a noisy plane, a clump with exact duplicates, and scattered points with few or no neighbours
    plane = np.c_[rng.uniform(0, 1, (1500, 2)), rng.normal(0, 0.005, 1500)]
    clump = rng.normal((0.5, 0.5, 0.3), 0.02, (300, 3))
    far = rng.uniform(-3, 3, (190, 3))
    xyz = np.vstack([plane, clump, far, clump[:10]])
    assert len(xyz) == 2000
    r = 0.1
    for min_k in (2, 5, 10):
        eig, k, valid = R.local_geometry(xyz, r, min_k, chunk=700)
        eb, kb, vb = R.brute(xyz, r, min_k)
        assert np.array_equal(k, kb)
        assert np.array_equal(valid, vb)
        # both covariances are two-pass in extended precision: they differ by the rounding to fp64 and eigvalsh's own error
        assert np.max(np.abs(eig - eb)) <= 16 * R.EPS * r * r
        assert np.all(eig[:, 0] >= eig[:, 1]) and np.all(eig[:, 1] >= eig[:, 2]) and np.all(eig[:, 2] >= 0)
        assert np.all(eig[~valid] == 0) and np.all(k[valid] >= min_k)
    assert (k == 0).any() and (k >= 10).any()
    sub = np.array([0, 1999, 1500, 17])
    es, ks, vs = R.local_geometry(xyz, r, 5, queries=sub)
    e5, k5, v5 = R.local_geometry(xyz, r, 5)
    assert np.array_equal(es, e5[sub]) and np.array_equal(ks, k5[sub]) and np.array_equal(vs, v5[sub])


def test_duplicates_stay_and_the_query_leaves_once():
    xyz = np.array([[0.0, 0, 0]] * 4 + [[0.01, 0, 0], [0, 0.02, 0], [5, 5, 5]])
    eig, k, valid = R.local_geometry(xyz, 0.1, 2)
    assert list(k) == [5, 5, 5, 5, 5, 5, 0]
    assert valid[:6].all() and not valid[6]
    eb, kb, vb = R.brute(xyz, 0.1, 2)
    assert np.array_equal(k, kb) and np.array_equal(valid, vb)


def test_plane_with_noise_gives_sigma2_and_planarity():
    """MPV of a plane with N(0, sigma^2) off-plane noise: the smallest eigenvalue of a neighbourhood's covariance is the off-plane
    sample variance up to the plane's tilt estimate — (k - 3) / (k - 1) sigma^2 in expectation for a fitted plane, at most sigma^2 —
    and a sample variance of k values has relative standard deviation sqrt(2 / (k - 1)).  The mean over the interior points
    (overlapping neighbourhoods: ~ n / k_mean independent ones) is judged at 4 sigma of that, plus the fit's 2 / (k_mean - 1) bias."""
    rng = np.random.default_rng(11)
    # (20 000 points / m^2: with k ~ 630 random points in a disc the two in-plane eigenvalues differ by ~ 1 / sqrt(k) = 4 % each, so
    # planarity (l2 - l3) / l1 sits near 0.94; at 2500 / m^2, k ~ 78, sampling alone holds it near 0.8)
    n, sigma, r, side = 20_000, 0.004, 0.1, 1.0
    xyz = np.c_[rng.uniform(0, side, (n, 2)), rng.normal(0, sigma, n)]
    eig, k, valid = R.local_geometry(xyz, r, 5)
    inner = valid & np.all((xyz[:, :2] > r) & (xyz[:, :2] < side - r), 1)
    km = k[inner].mean()
    mpv = eig[inner, 2].mean()
    n_indep = inner.sum() / km
    tol = 4 * math.sqrt(2 / (km - 1)) / math.sqrt(n_indep) + 2 / (km - 1)
    print(f"mean k {km:.1f}, MPV / sigma^2 = {mpv / sigma ** 2:.4f}, tolerance {tol:.4f}")
    assert 500 < km < 760
    assert abs(mpv / sigma ** 2 - 1) <= tol
    f = R.features(eig[inner])
    print(f"planarity {f[:, 1].mean():.4f}")
    assert f[:, 1].mean() > 0.9  # l1 ~ l2 ~ r^2 / 4, l3 = sigma^2
    s = R.summary(eig, k, valid)
    assert s["n_valid"] == int(valid.sum()) and s["mpv"] > 0


def test_line_and_ball():
    rng = np.random.default_rng(13)
    t = rng.uniform(0, 10, 5000)
    line = np.c_[t, 0.3 * t, -0.2 * t] + rng.normal(0, 1e-4, (5000, 3))
    eig, k, valid = R.local_geometry(line, 0.1, 5)
    assert valid.mean() > 0.95 and R.features(eig[valid])[:, 0].mean() > 0.9  # linearity
    v = rng.normal(size=(60_000, 3))
    ball = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, 1, (60_000, 1)) ** (1 / 3)
    eig, k, valid = R.local_geometry(ball, 0.2, 5)
    inner = valid & (np.linalg.norm(ball, axis=1) < 0.75)
    assert inner.sum() > 10_000 and R.features(eig[inner])[:, 2].mean() > 0.5  # sphericity


def test_summary_without_a_valid_point():
    xyz = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    eig, k, valid = R.local_geometry(xyz, 0.1, 5)
    s = R.summary(eig, k, valid)
    assert s["n_valid"] == 0 and s["mpv"] == 0.0 and s["mean_k"] == 0.0 and s["sphericity"] == 0.0


def test_struct_layout_matches_the_header():
    from cloud_map_evaluation_amd import _lib

    assert C.sizeof(_lib.LocalGeomOut) == 8 * 8
    assert [f for f, _ in _lib.LocalGeomOut._fields_] == ["n", "n_valid", "sum_l3", "sum_linearity", "sum_planarity", "sum_sphericity",
                                                          "sum_surface_variation", "sum_k"]
    hdr = open(os.path.join(ROOT, "include", "mapeval_hip.h")).read()
    body = hdr[hdr.index("typedef struct me_local_geom_out {"):hdr.index("} me_local_geom_out;")]
    assert "".join(body.split()) == ("typedefstructme_local_geom_out{int64_tn,n_valid;doublesum_l3,sum_linearity,sum_planarity,"
                                     "sum_sphericity,sum_surface_variation;int64_tsum_k;")
    assert "me_local_geometry" in _lib.SYMBOLS and "me_local_geometry_fetch" in _lib.SYMBOLS


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


def test_host_keys_defaults(tmp_path):
    r = _parse(tmp_path, "")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_mpv"] is False and p["mpv_radius"] == 0.15 and p["mpv_min_points"] == 5 and p["evaluate_gt_mpv"] is True
    p = json.loads(_parse(tmp_path, "evaluate_mpv: true\n", gt_mme="false").stdout)
    assert p["evaluate_mpv"] is True and p["evaluate_gt_mpv"] is False  # (follows evaluate_gt_mme)


def test_host_keys_are_read(tmp_path):
    r = _parse(tmp_path, "evaluate_mpv: true\nmpv_radius: 0.25\nmpv_min_points: 8\nevaluate_gt_mpv: false\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["evaluate_mpv"], p["mpv_radius"], p["mpv_min_points"], p["evaluate_gt_mpv"]) == (True, 0.25, 8, False)


def test_host_bad_values_and_combinations_are_refused(tmp_path):
    for extra, key in (("evaluate_mpv: true\nmpv_radius: 0\n", "mpv_radius"),
                       ("evaluate_mpv: true\nmpv_radius: -0.1\n", "mpv_radius"),
                       ("evaluate_mpv: true\nmpv_min_points: 1\n", "mpv_min_points")):
        r = _parse(tmp_path, extra)
        assert r.returncode != 0 and key in r.stderr, (extra, r.stderr)
    r = _parse(tmp_path, "evaluate_mpv: true\nnum_gpus: 2\n")
    assert r.returncode != 0 and "evaluate_mpv: single GPU only (num_gpus must be 1)" in r.stderr
    assert _parse(tmp_path, "evaluate_mpv: false\nnum_gpus: 2\n").returncode == 0


def test_shipped_reference_configs_keep_the_stage_off():
    ref_dir = os.path.join(ROOT, "tests", "golden", "reference_configs")
    for name in ("config.yaml", "config_building_day.yaml", "config_corridor.yaml", "config_geode.yaml"):
        r = subprocess.run([EXE, "--parse-config", os.path.join(ref_dir, name)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (name, r.stderr)
        assert json.loads(r.stdout)["evaluate_mpv"] is False
