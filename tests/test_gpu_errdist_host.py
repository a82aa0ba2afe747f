"""The C++ host's evaluate_error_distribution stage on the MI355X: the three lines of map_results.txt and error_distribution.txt equal
Engine.error_report on the same file-loaded clouds to the last digit, on both metric paths' resident 1-NN results, and without the key
nothing changes."""
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
QS = [0.5, 0.9, 1.0]
T = np.eye(4)
T[0, 3] = 0.05
KEYS = "error_quantiles: [0.5, 0.9, 1.0]\nerror_cdf_bins: 50\nerror_cdf_max: 0.5\n"


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
  - [1.0, 0.0, 0.0, 0.05]
  - [0.0, 1.0, 0.0, 0.0]
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
    return np.ascontiguousarray(est.numpy()[:5000]), np.ascontiguousarray(gt.numpy())


@pytest.fixture(scope="module")
def report(scene):
    """Engine.error_report on the clouds as the host holds them at its metric phase: ungated, and with the initial-matrix path's gate"""
    from cloud_map_evaluation_amd.engine import ME_GATE_LE_UNSQUARED, Engine

    est, gt = scene
    with Engine(0) as e:
        e.upload(0, est, T=T, cell_size=0.5)
        e.upload(1, gt, cell_size=0.5)
        e.nn1(0, 1, fetch=False)
        e.nn1(1, 0, fetch=False)
        moved = e.download(0)
        return (e.error_report(TAUS, QS, 50, 0.5 / 50), e.error_report(TAUS, QS, 50, 0.5 / 50, gate=1.0, gate_mode=ME_GATE_LE_UNSQUARED),
                moved)


def _lines(folder):
    return open(folder / "map_results.txt").read().splitlines()


def _check(folder, rep, clouds, gate):
    lines = _lines(folder)
    i = next(j for j, ln in enumerate(lines) if ln.startswith("FULL CD:"))
    est, gt = rep["est"], rep["gt"]
    assert lines[i + 1] == f"Hausdorff est-gt-sym: {est['max_d']:.5f} {gt['max_d']:.5f} {rep['hausdorff']:.5f}"
    assert lines[i + 2] == ("Error quantiles est|gt: " + " ".join(f"{q:.5f}" for q in QS) + " | " + " ".join(f"{v:.5f}" for v in est["quantile_d"])
                            + " | " + " ".join(f"{v:.5f}" for v in gt["quantile_d"]))
    assert lines[i + 3] == "Fscore P-R-F @t: " + " ".join(
        f"{t:.5f} {rep['precision'][k]:.5f} {rep['recall'][k]:.5f} {rep['fscore'][k]:.5f}" for k, t in enumerate(TAUS))
    assert lines[i + 4].startswith("VMD:")
    rows = [r.split() for r in open(folder / "error_distribution.txt").read().splitlines()]
    assert rows[0][0] == "gate" and float(rows[0][1]) == gate and rows[1] == ["gate_mode", "0"]
    assert rows[2][0] == "quantiles" and [float(v) for v in rows[2][1:]] == QS
    assert rows[3][0] == "thresholds" and [float(v) for v in rows[3][1:]] == TAUS
    assert rows[4] == ["cdf_bins", "50"] and rows[5][0] == "cdf_bin_width" and float(rows[5][1]) == 0.5 / 50
    k = 6
    for tag, d, xyz in (("est", est, clouds[0]), ("gt", gt, clouds[1])):
        r = rows[k]
        k += 1
        assert r[0] == tag and [int(r[1]), int(r[2]), int(r[7])] == [d["n_query"], d["n_used"], d["argmax"]]
        assert [float(v) for v in r[3:7]] == [d["sum_d"], d["sum_d2"], d["min_d"], d["max_d"]]  # (%.17g)
        assert [float(v) for v in r[8:11]] == list(xyz[d["argmax"]])
        for j, q in enumerate(QS):
            r = rows[k]
            k += 1
            assert r[:2] == [tag, "q"] and [float(r[2]), int(r[3]), float(r[4]), float(r[5])] == [q, d["rank"][j], d["quantile_d"][j], d["quantile_d2"][j]]
        for j, t in enumerate(TAUS):
            r = rows[k]
            k += 1
            assert r[:2] == [tag, "t"] and [float(r[2]), int(r[3])] == [t, d["n_within"][j]]
        cum = 0
        for j in range(50):
            r = rows[k]
            k += 1
            cum += int(d["hist"][j])
            assert r[:2] == [tag, "c"] and float(r[2]) == float(j + 1) * (0.5 / 50) and [int(r[3]), int(r[4])] == [int(d["hist"][j]), cum]
            assert float(r[5]) == cum / d["n_used"]
        assert rows[k] == [tag, "overflow", str(d["n_overflow"])]
        k += 1
    assert k == len(rows)


def test_lines_and_file_equal_engine_to_the_last_digit(scene, report, tmp_path):
    est, gt = scene
    ungated, gated, moved = report
    assert ungated["est"]["n_used"] == 5000 and ungated["gt"]["n_used"] == 6000 and ungated["hausdorff"] > 0
    # the one-call metric phase (the initial matrix, one GPU)
    _check(_run(tmp_path, "one", est, gt, "evaluate_error_distribution: true\n" + KEYS), ungated, (moved, gt), -1.0)
    # the separate calls (a stage that keeps the clouds resident before the metric phase switches the one call off)
    _check(_run(tmp_path, "sep", est, gt, "evaluate_error_distribution: true\nevaluate_mpv: true\n" + KEYS), ungated, (moved, gt), -1.0)
    # with the metric path's own gate
    _check(_run(tmp_path, "gated", est, gt, "evaluate_error_distribution: true\nerror_gated: true\n" + KEYS), gated, (moved, gt), 1.0)


_SKIP = ("Time", "Path:", "=====")  # (timings, the run's own paths, the dated header)
_NEW = ("Hausdorff est-gt-sym:", "Error quantiles est|gt:", "Fscore P-R-F @t:")


def test_without_the_key_nothing_changes(scene, tmp_path):
    """a run without the key equals, byte for byte, a run that sets it to false; a run with the key differs from both by exactly its three
    lines and its file"""
    est, gt = scene
    off = _run(tmp_path, "off", est, gt, KEYS)
    false = _run(tmp_path, "false", est, gt, "evaluate_error_distribution: false\n" + KEYS)
    on = _run(tmp_path, "on", est, gt, "evaluate_error_distribution: true\n" + KEYS)
    names_off = sorted(p.name for p in off.iterdir())
    assert "error_distribution.txt" not in names_off and sorted(p.name for p in false.iterdir()) == names_off
    assert sorted(p.name for p in on.iterdir()) == sorted(names_off + ["error_distribution.txt"])
    lo = [ln for ln in _lines(off) if not any(s in ln for s in _SKIP)]
    lf = [ln for ln in _lines(false) if not any(s in ln for s in _SKIP)]
    ln_on = [ln for ln in _lines(on) if not any(s in ln for s in _SKIP)]
    assert lf == lo and not any(ln.startswith(_NEW) for ln in lo)
    assert [ln for ln in ln_on if not ln.startswith(_NEW)] == lo and len(ln_on) == len(lo) + 3
    for name in names_off:
        if name != "map_results.txt":
            assert (false / name).read_bytes() == (off / name).read_bytes(), name
            assert (on / name).read_bytes() == (off / name).read_bytes(), name
