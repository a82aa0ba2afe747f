"""CPU checks of the simulation mode: the numpy Philox4x64-10 of tests/_perturb_ref.py against numpy's own Philox stream, hand cases of
the deform stage and of the outlier clamp, the host's noise_* keys (--parse-config) and the ABI struct."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _perturb_ref as R  # noqa: E402

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
M64 = (1 << 64) - 1


def _numpy_stream(counter, key, n_blocks):
    """numpy increments the counter BEFORE each block: Philox(counter=c).random_raw(4) is block c + 1; so start one below."""
    c = (sum(w << (64 * i) for i, w in enumerate(counter)) - 1) % (1 << 256)
    g = np.random.Philox(counter=np.array([(c >> (64 * i)) & M64 for i in range(4)], dtype=np.uint64), key=key)
    return g.random_raw(4 * n_blocks).reshape(n_blocks, 4)


def test_philox_known_answer_and_numpy_stream():
    # Random123's known answer for counter 0, key 0 (numpy: counter 2^64 - 1 in all four words, then one increment)
    got = np.random.Philox(counter=[M64] * 4, key=0).random_raw(4)
    assert [int(w) for w in got] == [0x16554D9ECA36314C, 0xDB20FE9D672D0FDC, 0xD7E772CEE186176B, 0x7E68B68AEC7BA23B]
    w = R.philox4x64_10(0, 0, 0, 0, 0, 0)
    assert [int(x[0]) for x in w] == [int(v) for v in got]
    # 10^4 consecutive counters from a start whose low word carries into the next words, with a two-word key
    for start, key in (([M64 - 4999, 5, 0, 0], (0x0123456789ABCDEF, 0xFEDCBA9876543210)),
                       ([M64 - 2, M64, M64 - 1, 3], (7, 0)),
                       ([0, 1, 0, 0], (M64, 0))):
        n = 10_000
        stream = _numpy_stream(start, key[0] | (key[1] << 64), n)
        c = sum(v << (64 * i) for i, v in enumerate(start))
        ctr = [[((c + j) % (1 << 256)) >> (64 * i) & M64 for j in range(n)] for i in range(4)]
        mine = R.philox4x64_10(*[np.array(x, dtype=np.uint64) for x in ctr], key[0], key[1])
        assert np.array_equal(np.stack(mine, axis=1), stream)


def test_uniform_and_box_muller_ranges():
    w = np.array([0, M64, 1 << 11, (1 << 11) - 1], dtype=np.uint64)
    u = R.u01(w)
    assert u[0] == 0.0 and u[1] == 1.0 - 2.0 ** -53 and u[2] == 2.0 ** -53 and u[3] == 0.0
    v = R.u01_open0(w)
    assert v[0] == 2.0 ** -53 and v[1] == 1.0
    n0, n1 = R.box_muller(np.array([M64], np.uint64), np.array([0], np.uint64))
    assert n0[0] == 0.0 and n1[0] == 0.0  # radius sqrt(-2 ln 1) = 0
    # a million normals: mean 0, variance 1
    blk = R.philox4x64_10(np.arange(500_000, dtype=np.uint64), 2, 0, 0, 3)
    a, b = R.box_muller(blk[0], blk[1])
    z = np.concatenate([a, b])
    assert abs(z.mean()) < 5e-3 and abs(z.var() - 1) < 5e-3


def test_deform_hand_cases():
    c = np.array([1.0, 2.0, 3.0])
    R_, s = 2.0, 0.5
    pts = np.array([c,                            # at the centre: unchanged (normalize() leaves a zero vector)
                    c + [2.0, 0.0, 0.0],          # d == R exactly: outside (strict d < R)
                    c + [0.0, 0.0, -2.5],         # beyond R
                    c + [0.3, -0.4, 1.2]])        # inside: d = 1.3
    out = R.deform(pts, R_, s, c)
    assert np.array_equal(out[0], pts[0]) and np.array_equal(out[1], pts[1]) and np.array_equal(out[2], pts[2])
    d = 1.3
    w = 0.5 * (1 + np.cos(np.pi * d / R_))
    np.testing.assert_allclose(out[3], pts[3] + np.array([0.3, -0.4, 1.2]) / d * s * w, rtol=0, atol=1e-15)
    dv = pts[3] - c
    dd = np.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
    assert np.array_equal(out[3], pts[3] + dv / dd * s * (0.5 * (1.0 + np.cos(np.pi * dd / R_))))
    # off: radius <= 0 or strength == 0
    assert np.array_equal(R.deform(pts, 0.0, s, c), pts) and np.array_equal(R.deform(pts, R_, 0.0, c), pts)


def test_outlier_clamp_at_u_near_one():
    # the largest uniform, u = 1 - 2^-53: (int64)(u n) = n - 1 for every n the upload admits (< 2^31), so the clamp never binds for a
    # 53-bit u; it keeps b inside the cloud for a draw that reaches 1.0 (the reference's uniform_real_distribution can round to it)
    u_max = float(R.u01(np.array([M64], np.uint64))[0])
    assert u_max == 1.0 - 2.0 ** -53
    n = np.unique(np.concatenate([np.arange(1, 5000), np.random.default_rng(1).integers(1, 1 << 31, 100_000), [(1 << 31) - 1]]))
    assert np.array_equal((u_max * n.astype(np.float64)).astype(np.int64), n - 1)
    assert np.array_equal(np.minimum(n - 1, (1.0 * n.astype(np.float64)).astype(np.int64)), n - 1)  # u = 1.0: clamped
    for n_kept in (1, 2, 3, 1000, (1 << 30) + 7):
        b = R.outlier_bases(n_kept, 5000, seed=9)
        assert b.min() >= 0 and b.max() <= n_kept - 1
    assert np.all(R.outlier_bases(1, 100, seed=3) == 0)


def test_pipeline_model_invariants():
    g = np.random.default_rng(0)
    src = g.uniform(-5, 5, (20_000, 3))
    full = R.perturb(src, noise_std=0.1, sparse_ratio=0.2, dense_ratio=0.8, region_size=2.0, outlier_ratio=0.1, outlier_range=1.0,
                     deform_radius=3.0, deform_strength=0.2, deform_center=(0, 0, 0), seed=4)
    nk = full["n_kept"]
    assert len(full["points"]) == nk + int(nk * 0.1)
    # survivors keep the source order, and their noise is a function of the source index only
    assert np.all(np.diff(full["src_index"]) > 0)
    other = R.perturb(src, noise_std=0.1, sparse_ratio=0.7, dense_ratio=0.8, region_size=2.0, deform_radius=3.0,
                      deform_strength=0.2, deform_center=(0, 0, 0), seed=4)
    common, i1, i2 = np.intersect1d(full["src_index"], other["src_index"], return_indices=True)
    assert len(common) > 1000
    assert np.array_equal(full["points"][i1], other["points"][i2])
    off = R.perturb(src)
    assert np.array_equal(off["points"], src)


# ---- the C++ host's keys -------------------------------------------------------------------------------------------------------------
_BASE = """registration_methods: 0
icp_max_distance: 0.5
save_immediate_result: true
evaluate_mme: true
evaluate_gt_mme: true
evaluate_using_initial: true
nn_radius: 0.1
vmd_voxel_size: 0.5
downsample_size: 0.0
estimate_map_path: /nonexistent/
gt_map_path: /nonexistent/gt.pcd
scene_name: s
enable_debug: false
"""


def _parse(tmp_path, extra):
    if not os.path.exists(EXE):
        pytest.skip("host binary not built")
    cfg = tmp_path / "c.yaml"
    cfg.write_text(_BASE + extra)
    return subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)


def test_parse_config_defaults(tmp_path):
    r = _parse(tmp_path, "")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_noised_gt"] is False and p["noise_std_dev"] == 0.1  # map_eval.h:87
    assert (p["noise_seed"], p["noise_sparse_ratio"], p["noise_dense_ratio"], p["noise_region_size"]) == (0, 1, 1, 0)
    assert (p["noise_outlier_ratio"], p["noise_outlier_range"], p["noise_deform_radius"], p["noise_deform_strength"]) == (0, 0, 0, 0)
    assert p["noise_deform_center"] == [0, 0, 0] and p["noise_sweep"] == []


def test_parse_config_reads_the_noise_keys(tmp_path):
    r = _parse(tmp_path, """evaluate_noised_gt: true
noise_std_dev: 0.03
noise_seed: 18446744073709551615
noise_sparse_ratio: 0.25
noise_dense_ratio: 0.75
noise_region_size: 4.0
noise_outlier_ratio: 0.02
noise_outlier_range: 1.5
noise_deform_radius: 3.0
noise_deform_strength: -0.2
noise_deform_center: [1.5, -2, 0.25]
noise_sweep: [0.01, 0.02, 0.04]
""")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_noised_gt"] is True and p["noise_std_dev"] == 0.03 and p["noise_seed"] == M64
    assert (p["noise_sparse_ratio"], p["noise_dense_ratio"], p["noise_region_size"]) == (0.25, 0.75, 4.0)
    assert (p["noise_outlier_ratio"], p["noise_outlier_range"]) == (0.02, 1.5)
    assert (p["noise_deform_radius"], p["noise_deform_strength"], p["noise_deform_center"]) == (3.0, -0.2, [1.5, -2, 0.25])
    assert p["noise_sweep"] == [0.01, 0.02, 0.04]


def test_misspelt_key_of_the_shipped_configs_is_not_read(tmp_path):
    r = _parse(tmp_path, "evaluate_noise_gt: true\n")
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["evaluate_noised_gt"] is False


@pytest.mark.parametrize("extra,key", [
    ("evaluate_noised_gt: true\nnum_gpus: 2\n", "evaluate_noised_gt"),
    ("noise_sweep: [0.01, 0.02]\n", "noise_sweep"),                                                   # without evaluate_noised_gt
    ("evaluate_noised_gt: true\nnoise_sweep: [0.01]\nnum_gpus: 2\n", "evaluate_noised_gt"),
    ("noise_deform_center: [1, 2]\n", "noise_deform_center"),
    ("noise_seed: -3\n", "noise_seed"),
    ("noise_sweep: []\n", "noise_sweep"),
])
def test_parse_config_refuses_bad_combinations(tmp_path, extra, key):
    r = _parse(tmp_path, extra)
    assert r.returncode != 0
    assert key in r.stderr


def test_sweep_needs_the_initial_matrix_path(tmp_path):
    r = _parse(tmp_path, "evaluate_noised_gt: true\nnoise_sweep: [0.01]\n")
    assert r.returncode == 0, r.stderr
    cfg = tmp_path / "c2.yaml"
    cfg.write_text(_BASE.replace("evaluate_using_initial: true", "evaluate_using_initial: false") +
                   "evaluate_noised_gt: true\nnoise_sweep: [0.01]\n")
    r = subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "noise_sweep" in r.stderr


def test_perturb_params_struct_matches_the_header():
    from cloud_map_evaluation_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "mapeval_hip.h")).read()
    body = re.search(r"typedef struct me_perturb_params \{(.*?)\} me_perturb_params;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n_double = 0
    for decl in re.findall(r"double ([^;]+);", body):
        for name in decl.split(","):
            m = re.search(r"\[(\d+)\]", name)
            n_double += int(m.group(1)) if m else 1
    n_u64 = len(re.findall(r"uint64_t \w+;", body))
    assert (n_double, n_u64) == (11, 1)
    assert C.sizeof(_lib.PerturbParams) == 8 * n_double + 8 * n_u64 == 96
    assert [f[0] for f in _lib.PerturbParams._fields_] == ["noise_std", "sparse_ratio", "dense_ratio", "region_size", "outlier_ratio",
                                                          "outlier_range", "deform_radius", "deform_strength", "deform_center", "seed"]
    assert "me_perturb_cloud" in _lib.SYMBOLS
