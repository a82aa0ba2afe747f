"""The C++ host's evaluate_observable stage on the MI355X: the `Observable` line of map_results.txt and observable.txt carry the numbers
of Engine.observable_report on the same files, each refusal is given by name, and without the key nothing changes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _mesh_ref as M
import _ply_mesh_files as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
T = np.eye(4)
T[0, 3] = 0.05
T[:2, :2] = [[0.8, -0.6], [0.6, 0.8]]
THS, TOL, RANGE, STRIDE = [0.5, 0.05], 0.01, 30.0, 2
KEYS = (f"gt_mesh_path: MESH\ntrajectory_path: TRAJ\nobservable_pose_stride: {STRIDE}\nobservable_max_range: {RANGE}\n"
        f"observable_tolerance: {TOL}\nobservable_thresholds: {THS}\n")
TRAJ = """# timestamp x y z qx qy qz qw
0.0 2.0 2.0 1.5 0 0 0 1

0.1 2.5 2.0 1.5 0 0 0 1
  0.2 1.0 3.0 1.0 0 0 0.6 0.8
0.3 3.0 1.0 2.0 0 0 0 1
0.4 1.5 1.5 0.5 0 0 0 1
"""
POSES = np.array([[2.0, 2.0, 1.5], [2.5, 2.0, 1.5], [1.0, 3.0, 1.0], [3.0, 1.0, 2.0], [1.5, 1.5, 0.5]])


def _write_pcd(path, pts):  # binary, 8-byte fields: the values survive exactly
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


def _config(base, name, scene, extra="", traj=TRAJ, head=""):
    v, tri, est, gt = scene
    d = base / name
    d.mkdir()
    _write_pcd(d / "map.pcd", est)
    _write_pcd(d / "gt.pcd", gt)
    F.write_ply_mesh(d / "gt_mesh.ply", v, [tuple(t) for t in tri], binary=True)
    (d / "traj.txt").write_text(traj)
    cfg = d / "config.yaml"
    cfg.write_text(f"""registration_methods: 0
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix:
  - [0.8, -0.6, 0.0, 0.05]
  - [0.6, 0.8, 0.0, 0.0]
  - [0.0, 0.0, 1.0, 0.0]
  - [0.0, 0.0, 0.0, 1.0]
estimate_map_path: {d}
gt_map_path: {d / 'gt.pcd'}
scene_name: rooms
save_immediate_result: true
evaluate_mme: true
evaluate_gt_mme: true
nn_radius: 0.5
evaluate_using_initial: true
vmd_voxel_size: 2.0
downsample_size: 0.0
enable_debug: false
{head}{extra.replace('MESH', str(d / 'gt_mesh.ply')).replace('TRAJ', str(d / 'traj.txt'))}""")
    return d, cfg


def _run(base, name, scene, extra="", **kw):
    d, cfg = _config(base, name, scene, extra, **kw)
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return d / "map_results"


def _cube(x0):
    v = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)]) * [4.0, 4.0, 3.0] + [x0, 0.0, 0.0]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)


@pytest.fixture(scope="module")
def scene():
    """Two closed rooms side by side, the trajectory inside the first; the map covers the first room only."""
    v1, t1 = _cube(0.0)
    v2, t2 = _cube(4.5)
    v, tri = np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)])
    a, b = M.sample(v1, t1, 6000, 1)[0], M.sample(v2, t2, 4000, 2)[0]
    gt = np.concatenate([a, b])
    on = a[::2] + np.random.default_rng(3).normal(0, 0.005, (3000, 3))
    est = (on - T[:3, 3]) @ T[:3, :3]  # the map as loaded: the initial matrix brings it back into the room
    return v, tri, np.ascontiguousarray(est), np.ascontiguousarray(gt)


def _lines(folder):
    return open(folder / "map_results.txt").read().splitlines()


def test_line_and_file_equal_engine(scene, tmp_path):
    from cloud_map_evaluation_amd.engine import Engine

    v, tri, est, gt = scene
    with Engine(0) as e:
        e.upload(0, est, cell_size=0.5)
        e.upload(1, gt, cell_size=0.5)
        e.transform_cloud(0, T)  # (the host's calls, in the host's order)
        e.mesh_upload(v, tri)
        rep = e.observable_report(POSES[::STRIDE], THS, tolerance=TOL, max_range=RANGE)
    vis, ga, go = rep["visibility"], rep["all"]["gt"], rep["observable"]["gt"]
    assert vis["n_visible"] == 6000 and vis["n_points"] == 10000
    out = _run(tmp_path, "on", scene, "evaluate_observable: true\n" + KEYS)
    lines = _lines(out)
    want = f"Observable visible-share COM@t: {rep['visible_share']:.5f}" + "".join(
        f" {t:.5f} {rep['all']['recall'][k]:.5f} {rep['observable']['recall'][k]:.5f}" for k, t in enumerate(THS))
    assert [ln for ln in lines if ln.startswith("Observable")] == [want]
    order = [ln.split(":")[0] for ln in lines]
    assert order.index("FULL CD") < order.index("Observable visible-share COM@t") < order.index("VMD")
    rows = [r.split() for r in open(out / "observable.txt").read().splitlines() if not r.startswith("#")]
    by = {r[0]: r[1:] for r in rows if not r[0][0].isdigit()}
    assert [int(by[k][0]) for k in ("poses_in_file", "pose_stride", "poses_used")] == [5, STRIDE, 3]
    assert [float(by["max_range"][0]), float(by["tolerance"][0])] == [RANGE, TOL]
    assert [int(by[k][0]) for k in ("n_points", "n_visible", "n_in_range", "n_tests")] == [vis[k] for k in ("n_points", "n_visible", "n_in_range", "n_tests")]
    assert float(by["visible_share"][0]) == rep["visible_share"]
    assert [int(by["n_used_all"][0]), int(by["n_used_observable"][0])] == [ga["n_used"], go["n_used"]] == [10000, 6000]
    th = [r for r in rows if r[0][0].isdigit()]
    assert [float(r[0]) for r in th] == THS
    assert [int(r[1]) for r in th] == ga["n_within"].tolist() and [int(r[3]) for r in th] == go["n_within"].tolist()
    assert [float(r[2]) for r in th] == rep["all"]["recall"].tolist() and [float(r[4]) for r in th] == rep["observable"]["recall"].tolist()
    assert float(th[0][4]) > 0.99 > float(th[0][2])


def test_each_refusal_is_named(scene, tmp_path):
    on = "evaluate_observable: true\n"
    cases = [
        ("gpus", on + KEYS + "num_gpus: 2\n", TRAJ, "evaluate_observable: single GPU only"),
        ("notraj", on + "gt_mesh_path: MESH\n", TRAJ, "trajectory_path: required with evaluate_observable"),
        ("nomesh", on + "trajectory_path: TRAJ\n", TRAJ, "evaluate_observable: needs a mesh"),
        ("stride", on + KEYS.replace(f"observable_pose_stride: {STRIDE}", "observable_pose_stride: 0"), TRAJ, "observable_pose_stride: must be an integer >= 1"),
        ("tol", on + KEYS.replace(f"observable_tolerance: {TOL}", "observable_tolerance: -1"), TRAJ, "observable_tolerance: must be finite and >= 0"),
        ("short", on + KEYS, TRAJ + "0.5 1.0 2.0\n", "line 8"),
        ("word", on + KEYS, TRAJ.replace("0.1 2.5", "0.1 x2.5"), "line 4"),
        ("missing", on + KEYS.replace("TRAJ", "/nonexistent/traj.txt"), TRAJ, "cannot open trajectory"),
    ]
    for name, extra, traj, msg in cases:
        d, cfg = _config(tmp_path, name, scene, extra, traj=traj)
        r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and msg in r.stdout + r.stderr, (name, r.stdout[-1500:], r.stderr[-1500:])


def test_parse_config_shows_the_defaults(scene, tmp_path):
    d, cfg = _config(tmp_path, "parse", scene)
    r = subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_observable"] is False and p["trajectory_path"] == "" and p["observable_pose_stride"] == 1
    assert p["observable_max_range"] == float("inf") and p["observable_tolerance"] == 0.05
    assert p["observable_thresholds"] == p["accuracy_level"]


_SKIP = ("Time", "Path:", "=====")  # (timings, the run's own paths, the dated header)


def test_without_the_key_nothing_changes(scene, tmp_path):
    """a run without the new keys equals, byte for byte, a run that carries them with the stage set to false; a run with the stage
    differs from both by exactly its line and its file"""
    off = _run(tmp_path, "off", scene)
    false = _run(tmp_path, "false", scene, "evaluate_observable: false\n" + KEYS)
    on = _run(tmp_path, "on", scene, "evaluate_observable: true\n" + KEYS)
    names_off = sorted(p.name for p in off.iterdir())
    assert "observable.txt" not in names_off and sorted(p.name for p in false.iterdir()) == names_off
    assert sorted(p.name for p in on.iterdir()) == sorted(names_off + ["observable.txt"])
    keep = lambda folder: [ln for ln in _lines(folder) if not any(s in ln for s in _SKIP)]
    lo, lf, ln_on = keep(off), keep(false), keep(on)
    assert lf == lo and not any(ln.startswith("Observable") for ln in lo)
    assert [ln for ln in ln_on if not ln.startswith("Observable")] == lo and len(ln_on) == len(lo) + 1
    for name in names_off:
        if name != "map_results.txt":
            assert (false / name).read_bytes() == (off / name).read_bytes(), name
            assert (on / name).read_bytes() == (off / name).read_bytes(), name
