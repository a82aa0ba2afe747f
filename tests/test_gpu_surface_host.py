"""The C++ host's evaluate_surface_error stage on the MI355X: the three lines of map_results.txt and surface_error.txt equal
Engine.radius_normals + Engine.surface_report on the same file-loaded clouds (lines, counts and the maximum to the last digit, sums
within n 2^-52), on the one-call metric phase and on the
separate stages before it, and without the key nothing changes."""
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
TAUS = [0.2, 0.1, 0.08, 0.05, 0.01]
ANGS = [5.0, 10.0, 20.0]
T = np.eye(4)
T[0, 3] = 0.05
T[:2, :2] = [[0.8, -0.6], [0.6, 0.8]]  # a rotation too: the normals must ride it


def _write_pcd(path, pts):  # binary, 8-byte fields: the values survive exactly
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


def _run(base, name, est, gt, extra="", icp=1.0):
    d = base / name
    d.mkdir()
    _write_pcd(d / "map.pcd", est)
    _write_pcd(d / "gt.pcd", gt)
    cfg = d / "config.yaml"
    cfg.write_text(f"""registration_methods: 0
icp_max_distance: {icp}
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix:
  - [0.8, -0.6, 0.0, 0.05]
  - [0.6, 0.8, 0.0, 0.0]
  - [0.0, 0.0, 1.0, 0.0]
  - [0.0, 0.0, 0.0, 1.0]
estimate_map_path: {d}
gt_map_path: {d / 'gt.pcd'}
scene_name: cube
save_immediate_result: true
evaluate_mme: true
evaluate_gt_mme: true
nn_radius: 0.5
evaluate_using_initial: true
vmd_voxel_size: 2.0
downsample_size: 0.0
enable_debug: false
{extra}""")
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return d / "map_results"


@pytest.fixture(scope="module")
def scene():
    from cloud_map_evaluation_amd import synth

    est, gt = synth.cube_pair(6000, seed=3)
    gt = gt.numpy()
    est = (est.numpy()[:5000] - T[:3, 3]) @ T[:3, :3]  # the map as loaded: the initial matrix brings it back onto the ground truth
    return np.ascontiguousarray(est), np.ascontiguousarray(gt)


@pytest.fixture(scope="module")
def report(scene):
    """the stage with Engine: normals on the clouds as loaded, the transform, the two searches, surface_report — ungated and gated"""
    from cloud_map_evaluation_amd.engine import ME_GATE_LE_UNSQUARED, Engine

    est, gt = scene
    with Engine(0) as e:
        e.upload(0, est, cell_size=0.5)
        e.upload(1, gt, cell_size=0.5)
        rn = (e.radius_normals(0, 0.3, 6), e.radius_normals(1, 0.3, 6))
        e.transform_cloud(0, T)
        e.nn1(0, 1, fetch=False)
        e.nn1(1, 0, fetch=False)
        return (e.surface_report(TAUS, ANGS), e.surface_report(TAUS, ANGS, gate=0.001, gate_mode=ME_GATE_LE_UNSQUARED), rn)


KEYS = "normal_radius: 0.3\nnormal_min_points: 6\n"


def _lines(folder):
    return open(folder / "map_results.txt").read().splitlines()


def _check(folder, rep, rn, gate):
    lines = _lines(folder)
    i = next(j for j, ln in enumerate(lines) if ln.startswith("FULL CD:"))
    est, gt = rep["est"], rep["gt"]
    assert lines[i + 1] == f"PlaneError est-gt-chamfer: {est['mean_e']:.5f} {gt['mean_e']:.5f} {rep['plane_chamfer']:.5f}"
    assert lines[i + 2] == "PlaneAC @t: " + " ".join(f"{t:.5f} {est['plane_rmse'][k]:.5f}" for k, t in enumerate(TAUS))
    assert lines[i + 3] == f"NormalConsistency est-gt: {est['mean_c']:.5f} {gt['mean_c']:.5f}"
    assert lines[i + 4].startswith("VMD:")
    rows = [r.split() for r in open(folder / "surface_error.txt").read().splitlines()]
    assert rows[0][0] == "normal_radius" and float(rows[0][1]) == 0.3
    assert rows[1] == ["normal_min_points", "6"] and float(rows[2][1]) == gate and rows[3] == ["gate_mode", "0"]
    assert rows[4][0] == "thresholds" and [float(v) for v in rows[4][1:]] == TAUS
    assert rows[5][0] == "angles_deg" and [float(v) for v in rows[5][1:]] == ANGS
    k = 6
    for s, (tag, d) in enumerate((("est", est), ("gt", gt))):
        assert rows[k] == [tag, "normals", str(rn[s]["n"]), str(rn[s]["n_valid"]), str(rn[s]["sum_k"])]
        r = rows[k + 1]
        k += 2
        assert r[0] == tag and [int(r[1]), int(r[2]), int(r[3]), int(r[9])] == [d["n_query"], d["n_used"], d["n_normal_used"], d["argmax"]]
        # (%.17g) max_e is an element of the input; a sum is formed in the order of the slot's index, which the host's stages and
        # Engine's build at different moments: any order of n non-negative terms agrees within n 2^-52 relative
        assert float(r[8]) == d["max_e"]
        for v, key in zip(r[4:8], ("sum_e", "sum_e2", "sum_t2", "sum_c")):
            assert math.isclose(float(v), d[key], rel_tol=d["n_query"] * 2.0 ** -52, abs_tol=0.0), key
        for j, t in enumerate(TAUS):
            r = rows[k]
            k += 1
            assert r[:2] == [tag, "t"] and [float(r[2]), int(r[3])] == [t, d["n_within"][j]]
            assert math.isclose(float(r[4]), d["sum_e2_within"][j], rel_tol=d["n_query"] * 2.0 ** -52, abs_tol=0.0)
        for j, a in enumerate(ANGS):
            r = rows[k]
            k += 1
            assert r[:2] == [tag, "a"] and [float(r[2]), float(r[3]), int(r[4])] == [a, math.cos(a * (math.pi / 180.0)), d["n_angle"][j]]
    assert k == len(rows)


def test_lines_and_file_equal_engine_to_the_last_digit(scene, report, tmp_path):
    est, gt = scene
    ungated, gated, rn = report
    assert 0 < ungated["est"]["n_normal_used"] <= ungated["est"]["n_used"] <= 5000 and ungated["gt"]["n_used"] > 0
    assert gated["est"]["n_used"] < ungated["est"]["n_used"]
    # the normals ride the one call of the metric phase (no error-distribution lines: the three lines follow FULL CD)
    _check(_run(tmp_path, "one", est, gt, "evaluate_surface_error: true\n" + KEYS), ungated, rn, -1.0)
    # next to the other stages on the resident clouds
    _check(_run(tmp_path, "sep", est, gt, "evaluate_surface_error: true\nevaluate_mpv: true\n" + KEYS), ungated, rn, -1.0)
    # with the metric path's own gate
    _check(_run(tmp_path, "gated", est, gt, "evaluate_surface_error: true\nsurface_gated: true\n" + KEYS, icp=0.001), gated, rn, 0.001)


def test_after_the_error_distribution_lines(scene, tmp_path):
    est, gt = scene
    lines = _lines(_run(tmp_path, "both", est, gt, "evaluate_surface_error: true\nevaluate_error_distribution: true\n" + KEYS))
    i = next(j for j, ln in enumerate(lines) if ln.startswith("Fscore P-R-F @t:"))
    assert lines[i + 1].startswith("PlaneError est-gt-chamfer:") and lines[i + 2].startswith("PlaneAC @t:")
    assert lines[i + 3].startswith("NormalConsistency est-gt:") and lines[i + 4].startswith("VMD:")


_SKIP = ("Time", "Path:", "=====")  # (timings, the run's own paths, the dated header)
_NEW = ("PlaneError est-gt-chamfer:", "PlaneAC @t:", "NormalConsistency est-gt:")


def test_without_the_key_nothing_changes(scene, tmp_path):
    """a run without the key equals, byte for byte, a run that sets it to false; a run with the key differs from both by exactly its three
    lines and its file"""
    est, gt = scene
    off = _run(tmp_path, "off", est, gt, KEYS)
    false = _run(tmp_path, "false", est, gt, "evaluate_surface_error: false\n" + KEYS)
    on = _run(tmp_path, "on", est, gt, "evaluate_surface_error: true\n" + KEYS)
    names_off = sorted(p.name for p in off.iterdir())
    assert "surface_error.txt" not in names_off and sorted(p.name for p in false.iterdir()) == names_off
    assert sorted(p.name for p in on.iterdir()) == sorted(names_off + ["surface_error.txt"])
    lo = [ln for ln in _lines(off) if not any(s in ln for s in _SKIP)]
    lf = [ln for ln in _lines(false) if not any(s in ln for s in _SKIP)]
    ln_on = [ln for ln in _lines(on) if not any(s in ln for s in _SKIP)]
    assert lf == lo and not any(ln.startswith(_NEW) for ln in lo)
    assert [ln for ln in ln_on if not ln.startswith(_NEW)] == lo and len(ln_on) == len(lo) + 3
    for name in names_off:
        if name != "map_results.txt":
            assert (false / name).read_bytes() == (off / name).read_bytes(), name
            assert (on / name).read_bytes() == (off / name).read_bytes(), name
