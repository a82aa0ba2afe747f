"""The C++ host with global_registration: true, from PCD files: a map in its own frame (a yaw > 90 degrees rotation and tens of metres
away) evaluated from an identity initial_matrix against a run given the true initial_matrix, global_registration.txt, and no new output
without the key."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")


def _write_pcd(path, pts):
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


def _rot(yaw, roll, pitch):
    cz, sz, cx, sx, cy, sy = math.cos(yaw), math.sin(yaw), math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    from cloud_map_evaluation_amd import synth

    est, gt = synth.scan_pair(200_000, density=50.0, seed=31)
    Tm = np.eye(4)
    Tm[:3, :3] = _rot(2.4, 0.04, -0.05)
    Tm[:3, 3] = (35.0, -22.0, 3.0)
    d = tmp_path_factory.mktemp("pair")
    _write_pcd(d / "gt.pcd", gt.numpy())
    est_m = est.numpy() @ Tm[:3, :3].T + Tm[:3, 3]
    return d, est_m, np.linalg.inv(Tm)


def _run(pair, name, initial, extra=""):
    base, est_m, _ = pair
    d = base / name
    d.mkdir()
    _write_pcd(d / "map.pcd", est_m)
    rows = "\n".join("  - [" + ", ".join(repr(float(v)) for v in initial[i]) + "]" for i in range(4))
    cfg = d / "config.yaml"
    cfg.write_text(f"""registration_methods: 2
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix:
{rows}
estimate_map_path: {d}
gt_map_path: {base / 'gt.pcd'}
scene_name: coarse
save_immediate_result: true
evaluate_mme: false
evaluate_gt_mme: false
nn_radius: 0.1
evaluate_using_initial: false
vmd_voxel_size: 0.5
downsample_size: 0.0
enable_debug: false
{extra}""")
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=600)
    return r, d / "map_results"


def _results(folder):
    txt = open(folder / "map_results.txt").read()
    return {k: [float(v) for v in re.search(rf"^{re.escape(k)}: (.*)$", txt, flags=re.M).group(1).split()] for k in ("RMSE/AC", "Comp")}


def test_host_global_registration_from_identity(pair):
    _, _, Ttrue = pair
    r0, f0 = _run(pair, "true_initial", Ttrue)
    assert r0.returncode == 0, r0.stdout[-2000:] + r0.stderr[-2000:]
    r1, f1 = _run(pair, "global", np.eye(4), "global_registration: true\nglobal_voxel_size: 1.0\nglobal_max_iterations: 200000\n")
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    a, b = _results(f1), _results(f0)
    np.testing.assert_allclose(a["RMSE/AC"][0], b["RMSE/AC"][0], rtol=1e-3)
    np.testing.assert_allclose(a["Comp"][0], b["Comp"][0], rtol=1e-3)
    # global_registration.txt: T_c, then fitness, rmse, counts, seed
    lines = open(f1 / "global_registration.txt").read().splitlines()
    Tc = np.array([[float(v) for v in lines[i].split()] for i in range(4)])
    kv = dict(l.split() for l in lines[4:])
    assert set(kv) == {"fitness", "inlier_rmse", "correspondences", "valid_hypotheses", "seed"}
    assert 0 < float(kv["fitness"]) <= 1 and int(kv["correspondences"]) >= 3 and int(kv["valid_hypotheses"]) >= 1 and kv["seed"] == "0"
    dR = Tc[:3, :3] @ Ttrue[:3, :3].T
    assert math.degrees(math.acos(min(1.0, (np.trace(dR) - 1) / 2))) < 2.0
    assert np.allclose(Tc[3], [0, 0, 0, 1])
    # without the key: no file, and stdout has no line of the feature
    assert not (f0 / "global_registration.txt").exists()
    assert "global" not in r0.stdout.lower()


def test_host_min_fitness_refuses_a_poor_alignment(pair):
    r, f = _run(pair, "strict", np.eye(4), "global_registration: true\nglobal_max_iterations: 2000\nglobal_min_fitness: 1.01\n")
    assert r.returncode != 0
    assert "global_min_fitness" in (r.stdout + r.stderr)
    assert (f / "global_registration.txt").exists()
    assert "RMSE/AC" not in open(f / "map_results.txt").read()  # (the file is opened in append mode at the start, as the reference's)
