"""The C++ host's evaluate_m3c2 stage on the MI355X: the line of map_results.txt and m3c2.txt equal Engine.radius_normals + Engine.m3c2
on the same file-loaded clouds, the map moved by the initial matrix (line and counts to the last digit, sums within n 2^-52), alone and
next to the surface-error stage, and without the key nothing changes."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
T = np.eye(4)
T[0, 3] = 0.05
T[:2, :2] = [[0.8, -0.6], [0.6, 0.8]]
NR, RP, L, MINP, REG, EVERY = 0.3, 0.2, 0.45, 6, 0.002, 3
KEYS = (f"m3c2_normal_radius: {NR}\nm3c2_projection_radius: {RP}\nm3c2_max_depth: {L}\nm3c2_min_points: {MINP}\nm3c2_reg_error: {REG}\n"
        f"m3c2_core_every: {EVERY}\nnormal_min_points: 6\n")


def _write_pcd(path, pts):  # binary, 8-byte fields: the values survive exactly
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


def _run(base, name, est, gt, extra=""):
    d = base / name
    d.mkdir()
    _write_pcd(d / "map.pcd", est)
    _write_pcd(d / "gt.pcd", gt)
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
def engine_result(scene):
    """the stage with Engine, in the host's order: uploads at nn_radius, the map moved, normals on both clouds, m3c2 both ways"""
    from cloud_map_evaluation_amd.engine import Engine

    est, gt = scene
    with Engine(0) as e:
        e.upload(1, gt, cell_size=0.5)
        e.upload(0, est, cell_size=0.5)
        e.transform_cloud(0, T)
        rn = (e.radius_normals(0, NR, 6), e.radius_normals(1, NR, 6))
        out = []
        for slot in (0, 1):
            mask = np.zeros(e.size(slot), np.uint8)
            mask[::EVERY] = 1
            out.append(e.m3c2(slot, RP, L, MINP, REG, mask))
        return out, rn


def _lines(folder):
    return open(folder / "map_results.txt").read().splitlines()


def _check(folder, res, rn):
    lines = _lines(folder)
    i = next(j for j, ln in enumerate(lines) if ln.startswith("M3C2 est-gt:"))
    d = res[0]
    assert lines[i] == f"M3C2 est-gt: {d['mean_dist']:.5f} {d['mean_abs_dist']:.5f} {d['rms_dist']:.5f} {d['significant_share']:.5f}"
    assert lines[i + 1].startswith("VMD:")
    rows = [r.split() for r in open(folder / "m3c2.txt").read().splitlines()]
    assert [r[0] for r in rows[:7]] == ["normal_radius", "normal_min_points", "projection_radius", "max_depth", "min_points", "reg_error",
                                        "core_every"]
    assert [float(r[1]) for r in rows[:7]] == [NR, 6, RP, L, MINP, REG, EVERY]
    k = 7
    for s, tag in enumerate(("est", "gt")):
        d = res[s]
        assert rows[k] == [tag, "normals", str(rn[s]["n"]), str(rn[s]["n_valid"]), str(rn[s]["sum_k"])]
        r = rows[k + 1]
        assert r[0] == tag and [int(v) for v in r[1:5]] == [d["n_core"], d["n_no_normal"], d["n_valid"], d["n_significant"]]
        assert [int(r[9]), int(r[10])] == [d["sum_n_own"], d["sum_n_other"]]
        # (%.17g) the host and Engine make the same calls on the same data, but a sum is formed in the order of the slot's index: any
        # order of n terms agrees within n 2^-52 of the sum of their magnitudes (sum_abs_dist bounds that of sum_dist)
        n = d["n_valid"]
        for v, key, scale in zip(r[5:9], ("sum_dist", "sum_abs_dist", "sum_dist2", "sum_lod"),
                                 (d["sum_abs_dist"], d["sum_abs_dist"], d["sum_dist2"], d["sum_lod"])):
            assert abs(float(v) - d[key]) <= n * 2.0 ** -52 * scale, key
        w = rows[k + 2]
        assert w[:2] == [tag, "worst"] and int(w[3]) == d["argmax"] and float(w[2]) == d["max_abs_dist"]
        k += 3
    assert k == len(rows)


def test_line_and_file_equal_engine(scene, engine_result, tmp_path):
    est, gt = scene
    res, rn = engine_result
    assert res[0]["n_core"] == (5000 + EVERY - 1) // EVERY and res[0]["n_valid"] > 1000 and res[1]["n_valid"] > 1000
    _check(_run(tmp_path, "alone", est, gt, "evaluate_m3c2: true\n" + KEYS), res, rn)
    # next to the surface-error stage, which estimates normals of its own afterwards: neither clobbers the other
    both = _run(tmp_path, "both", est, gt, "evaluate_m3c2: true\nevaluate_surface_error: true\nnormal_radius: 0.3\n" + KEYS)
    _check(both, res, rn)
    surf = _run(tmp_path, "surf", est, gt, "evaluate_surface_error: true\nnormal_radius: 0.3\n" + KEYS)
    assert (both / "surface_error.txt").read_bytes() == (surf / "surface_error.txt").read_bytes()


_SKIP = ("Time", "Path:", "=====")  # (timings, the run's own paths, the dated header)


def test_without_the_key_nothing_changes(scene, tmp_path):
    """a run without the key equals, byte for byte, a run that sets it to false; a run with the key differs from both by exactly its
    line and its file"""
    est, gt = scene
    off = _run(tmp_path, "off", est, gt, KEYS)
    false = _run(tmp_path, "false", est, gt, "evaluate_m3c2: false\n" + KEYS)
    on = _run(tmp_path, "on", est, gt, "evaluate_m3c2: true\n" + KEYS)
    names_off = sorted(p.name for p in off.iterdir())
    assert "m3c2.txt" not in names_off and sorted(p.name for p in false.iterdir()) == names_off
    assert sorted(p.name for p in on.iterdir()) == sorted(names_off + ["m3c2.txt"])
    lo = [ln for ln in _lines(off) if not any(s in ln for s in _SKIP)]
    lf = [ln for ln in _lines(false) if not any(s in ln for s in _SKIP)]
    ln_on = [ln for ln in _lines(on) if not any(s in ln for s in _SKIP)]
    assert lf == lo and not any(ln.startswith("M3C2") for ln in lo)
    assert [ln for ln in ln_on if not ln.startswith("M3C2 est-gt:")] == lo and len(ln_on) == len(lo) + 1
    for name in names_off:
        if name != "map_results.txt":
            assert (false / name).read_bytes() == (off / name).read_bytes(), name
            assert (on / name).read_bytes() == (off / name).read_bytes(), name
