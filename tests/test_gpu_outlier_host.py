"""The C++ host's outlier keys on the MI355X: remove_outliers (statistical; radius with outlier_filter_gt) gives the result files of a run
without the key on PCDs of the kept points, and global_outlier_nb_neighbors lets global_registration find the pose of a map with sparse
outliers."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")


def _write_pcd(path, pts):  # binary, 8-byte fields: the values survive exactly
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


def _run(base, name, est, gt, extra="", initial=np.eye(4), using_initial=True):
    d = base / name
    d.mkdir()
    _write_pcd(d / "map.pcd", est)
    _write_pcd(d / "gt.pcd", gt)
    rows = "\n".join("  - [" + ", ".join(repr(float(v)) for v in initial[i]) + "]" for i in range(4))
    cfg = d / "config.yaml"
    cfg.write_text(f"""registration_methods: 2
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix:
{rows}
estimate_map_path: {d}
gt_map_path: {d / 'gt.pcd'}
scene_name: outliers
save_immediate_result: true
evaluate_mme: true
evaluate_gt_mme: true
nn_radius: 0.1
evaluate_using_initial: {'true' if using_initial else 'false'}
vmd_voxel_size: 0.5
downsample_size: 0.0
enable_debug: false
{extra}""")
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return d / "map_results"


_SKIP = ("Time", "Path:", "=====")  # (timings, the run's own paths, the dated header)


def _same_results(a, b):
    fa = sorted(p.name for p in a.iterdir() if p.name != "outlier_removal.txt")
    fb = sorted(p.name for p in b.iterdir())
    assert fa == fb
    for name in fa:
        if name.endswith(".txt"):
            la = [ln for ln in open(a / name).read().splitlines() if not any(s in ln for s in _SKIP)]
            lb = [ln for ln in open(b / name).read().splitlines() if not any(s in ln for s in _SKIP)]
            assert la == lb, name
        else:
            assert open(a / name, "rb").read() == open(b / name, "rb").read(), name


@pytest.fixture(scope="module")
def scene():
    from cloud_map_evaluation_amd import synth

    est, gt = synth.scan_pair(200_000, density=2500.0, seed=61, outlier_ratio=0.003)
    return est.numpy(), gt.numpy()


def _kept(xyz, how):
    from cloud_map_evaluation_amd.engine import Engine

    with Engine(0) as e:
        e.upload(0, xyz, cell_size=0.1)
        if how[0] == "statistical":
            _, _, keep = e.statistical_outlier(0, how[1], how[2], fetch=True)
        else:
            _, _, keep = e.radius_outlier(0, how[1], how[2], fetch=True)
    return xyz[keep.astype(bool)]


def test_statistical_equals_a_run_on_the_kept_points(scene, tmp_path):
    est, gt = scene
    f1 = _run(tmp_path, "filtered", est, gt, "remove_outliers: statistical\noutlier_nb_neighbors: 20\noutlier_std_ratio: 2.0\n")
    kept = _kept(est, ("statistical", 20, 2.0))
    assert len(kept) < len(est)
    f0 = _run(tmp_path, "kept", kept, gt)
    _same_results(f1, f0)
    lines = open(f1 / "outlier_removal.txt").read().splitlines()
    assert lines[:4] == ["method statistical", "nb_neighbors 20", "std_ratio 2", "filter_gt false"]
    est_line = lines[4].split()
    assert est_line[0] == "est" and int(est_line[1]) == len(est) and int(est_line[2]) == len(kept) and len(lines) == 5
    assert not (f0 / "outlier_removal.txt").exists()  # (every key at its default: no new file)


def test_radius_with_gt_equals_a_run_on_the_kept_points(scene, tmp_path):
    est, gt = scene
    f1 = _run(tmp_path, "filtered", est, gt,
              "remove_outliers: radius\noutlier_nb_points: 3\noutlier_radius: 0.1\noutlier_filter_gt: true\n")
    ke, kg = _kept(est, ("radius", 3, 0.1)), _kept(gt, ("radius", 3, 0.1))
    assert len(ke) < len(est)
    f0 = _run(tmp_path, "kept", ke, kg)
    _same_results(f1, f0)
    lines = open(f1 / "outlier_removal.txt").read().splitlines()
    assert [ln.split()[0] for ln in lines] == ["method", "nb_points", "radius", "filter_gt", "est", "gt"]
    assert int(lines[5].split()[2]) == len(kg)


def _rot_z(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def test_global_registration_with_the_outlier_filter(tmp_path):
    from cloud_map_evaluation_amd import synth

    est, gt = synth.scan_pair(5_000_000, outlier_ratio=0.001)
    est, gt = est.numpy(), gt.numpy()
    Tm = np.eye(4)
    Tm[:3, :3] = _rot_z(math.radians(135.0))
    Tm[:3, 3] = (12.0, -7.0, 1.5)
    est_m = est @ Tm[:3, :3].T + Tm[:3, 3]
    Ttrue = np.linalg.inv(Tm)
    f = _run(tmp_path, "global", est_m, gt, "global_registration: true\nglobal_voxel_size: 1.0\nglobal_max_iterations: 200000\n"
             "global_outlier_nb_neighbors: 20\nevaluate_mme: false\nevaluate_gt_mme: false\n", using_initial=False)
    lines = open(f / "global_registration.txt").read().splitlines()
    Tc = np.array([[float(v) for v in lines[i].split()] for i in range(4)])
    names = [ln.split()[0] for ln in lines[4:]]
    assert names[-4:] == ["outlier_nb_neighbors", "outlier_std_ratio", "outlier_est", "outlier_gt"]
    c = est_m.mean(0)
    dR = Tc[:3, :3] @ Ttrue[:3, :3].T
    assert math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2)))) < 1.0
    assert np.linalg.norm((Tc[:3, :3] @ c + Tc[:3, 3]) - (Ttrue[:3, :3] @ c + Ttrue[:3, 3])) < 0.5
