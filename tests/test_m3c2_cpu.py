"""The brute-force M3C2 model (tests/_m3c2_ref.py) against closed forms, the binding's structs, and the host's M3C2 keys through
--parse-config (the result line and m3c2.txt need a device run: tests/test_gpu_m3c2_host.py).  No GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import _m3c2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")


def _lattice(nx, ny, zs, step):
    g = np.array([(i * step, j * step, z) for i in range(-nx, nx + 1) for j in range(-ny, ny + 1) for z in zs], np.float64)
    return np.ascontiguousarray(g)


def test_two_lattice_planes_give_the_offset_and_no_variance():
    delta = 1.0 / 16.0  # dyadic: every t, S and Q is exact
    own = _lattice(6, 6, [0.0], 0.125)
    other = _lattice(6, 6, [delta], 0.125)
    nrm = np.tile([0.0, 0.0, 1.0], (len(own), 1))
    m = R.m3c2(own, other, nrm, 0.3, 0.25, min_points=5)
    centre = int(np.flatnonzero((own[:, 0] == 0) & (own[:, 1] == 0))[0])
    disc = sum(1 for i in range(-6, 7) for j in range(-6, 7) if (i * i + j * j) * 0.125 * 0.125 < 0.3 * 0.3)
    assert m["n_own"][centre] == disc == m["n_other"][centre]
    assert m["valid"].all()
    assert (m["dist"] == delta).all() and (m["var_own"] == 0).all() and (m["var_other"] == 0).all() and (m["lod"] == 0).all()
    assert m["significant"].all()
    # the other way round and with the normals turned: the sign follows +N
    m2 = R.m3c2(own, other, -nrm, 0.3, 0.25)
    assert (m2["dist"] == -delta).all()
    # the planes further apart than the cylinder is long: nothing of the other cloud inside, every point invalid
    far = R.m3c2(own, other + [0, 0, 1.0], nrm, 0.3, 0.25)
    assert (far["n_other"] == 0).all() and not far["valid"].any() and (far["dist"] == 0).all()


def test_hand_counted_disc_and_strict_edges():
    # step 1/8, rp = 5/8, L = 2/8, normal +z: (3, 4) and (5, 0) lie exactly ON the cylinder's wall, |k| = 2 exactly on its caps
    pts = np.array([(i / 8, j / 8, k / 8) for i in range(-6, 7) for j in range(-6, 7) for k in range(-3, 4)], np.float64)
    inside, t = R.members(np.zeros(3), np.array([0.0, 0.0, 1.0]), pts, 5 / 8, 2 / 8)
    disc = sum(1 for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 25)  # 69: the 12 points with i*i + j*j == 25 are out
    assert disc == 69 and int(inside.sum()) == disc * 3  # k in {-1, 0, 1}
    assert not inside[(np.abs(pts[:, 2]) == 0.25)].any()
    on_wall = (pts[:, 0] ** 2 + pts[:, 1] ** 2 == 25 / 64)
    assert on_wall.sum() == 12 * 7 and not inside[on_wall].any()
    # one lattice step inside both
    assert inside[(pts[:, 0] == 0.5) & (pts[:, 1] == 0.25) & (pts[:, 2] == 0.125)].all()


def test_mask_min_points_and_zero_normals_in_the_model():
    rng = np.random.default_rng(5)
    own = rng.random((200, 3)) * [1, 1, 0.02]
    other = rng.random((150, 3)) * [1, 1, 0.02] + [0, 0, 0.01]
    nrm = np.tile([0.0, 0.0, 1.0], (200, 1))
    nrm[7] = 0
    mask = np.zeros(200, np.uint8)
    mask[::3] = 1
    mask[7] = 1
    m = R.m3c2(own, other, nrm, 0.2, 0.1, min_points=4, mask=mask)
    off = mask == 0
    assert not m["valid"][off].any() and (m["n_own"][off] == 0).all() and (m["dist"][off] == 0).all()
    assert not m["valid"][7] and m["n_own"][7] > 0  # a zero normal: the counts are kept, the point is invalid
    v = m["valid"]
    assert v.any() and (m["n_own"][v] >= 4).all() and (m["n_other"][v] >= 4).all()
    assert (np.abs(m["dist"][v] - 0.01) < 0.02).all() and (m["var_own"][v] >= 0).all()
    lod = 1.96 * np.sqrt(m["var_own"][v] / m["n_own"][v] + m["var_other"][v] / m["n_other"][v])
    assert np.allclose(m["lod"][v], lod, rtol=1e-14, atol=0)


def test_binding_structs_match_the_header():
    from cloud_map_evaluation_amd import _lib

    assert C.sizeof(_lib.M3c2Params) == 32 and C.sizeof(_lib.M3c2Out) == 96
    assert _lib.M3c2Out.max_abs_dist.offset == 80 and _lib.M3c2Out.argmax.offset == 88
    assert "me_m3c2" in _lib.SYMBOLS and "me_m3c2_fetch" in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "mapeval_hip.h")).read()
    assert "int me_m3c2(me_ctx *ctx, int query_slot, const me_m3c2_params *p, const uint8_t *core_mask, me_m3c2_out *out);" in hdr
    assert "int me_m3c2_fetch(" in hdr


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


def test_defaults_are_printed_with_the_stage_off(tmp_path):
    r = _parse(tmp_path, "")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_m3c2"] is False
    assert (p["m3c2_normal_radius"], p["m3c2_projection_radius"], p["m3c2_max_depth"]) == (0.15, 0.15, 4 * 0.15)  # (from nn_radius)
    assert (p["m3c2_min_points"], p["m3c2_reg_error"], p["m3c2_core_every"]) == (5, 0, 1)


def test_keys_are_read(tmp_path):
    r = _parse(tmp_path, "evaluate_m3c2: true\nm3c2_normal_radius: 0.25\nm3c2_projection_radius: 0.125\nm3c2_max_depth: 0.75\n"
                         "m3c2_min_points: 8\nm3c2_reg_error: 0.005\nm3c2_core_every: 4\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["evaluate_m3c2"], p["m3c2_normal_radius"], p["m3c2_projection_radius"], p["m3c2_max_depth"], p["m3c2_min_points"],
            p["m3c2_reg_error"], p["m3c2_core_every"]) == (True, 0.25, 0.125, 0.75, 8, 0.005, 4)
    assert _parse(tmp_path, "evaluate_m3c2: true\nevaluate_surface_error: true\n").returncode == 0


def test_bad_values_and_combinations_are_refused(tmp_path):
    for extra, key in (("num_gpus: 2\n", "evaluate_m3c2: single GPU only (num_gpus must be 1)"),
                       ("m3c2_normal_radius: 0\n", "m3c2_normal_radius"),
                       ("m3c2_projection_radius: -1\n", "m3c2_projection_radius"),
                       ("m3c2_max_depth: 0\n", "m3c2_max_depth"),
                       ("m3c2_min_points: 1\n", "m3c2_min_points"),
                       ("m3c2_reg_error: -0.1\n", "m3c2_reg_error"),
                       ("m3c2_core_every: 0\n", "m3c2_core_every"),
                       ("evaluate_noised_gt: true\n", "evaluate_m3c2: not with evaluate_noised_gt")):
        r = _parse(tmp_path, "evaluate_m3c2: true\n" + extra)
        assert r.returncode != 0 and key in r.stderr, (extra, r.stderr)
    r = _parse(tmp_path, "evaluate_m3c2: true\n", _BASE.replace("evaluate_using_initial: true", "evaluate_using_initial: false"))
    assert r.returncode != 0 and "evaluate_m3c2: needs evaluate_using_initial" in r.stderr
    # the stage is off: its keys are not judged
    assert _parse(tmp_path, "evaluate_m3c2: false\nnum_gpus: 2\nm3c2_min_points: 0\nm3c2_max_depth: -3\n").returncode == 0


def test_shipped_reference_configs_keep_the_stage_off():
    ref_dir = os.path.join(ROOT, "tests", "golden", "reference_configs")
    for name in ("config.yaml", "config_building_day.yaml", "config_corridor.yaml", "config_geode.yaml"):
        r = subprocess.run([EXE, "--parse-config", os.path.join(ref_dir, name)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (name, r.stderr)
        assert json.loads(r.stdout)["evaluate_m3c2"] is False
