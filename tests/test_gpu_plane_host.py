"""The C++ host's segment_planes stage and remove_outliers: plane on the MI355X: plane_segmentation.txt equals Engine.segment_planes on
the same file-loaded clouds to the last digit, the `Planes est-gt:` line follows the MPV lines, and removing the largest plane changes
the evaluated point count by exactly its inlier count."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _globreg_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
KEYS = "plane_distance_threshold: 0.06\nplane_num_iterations: 200\nplane_max_planes: 4\nplane_min_inliers: 300\nplane_seed: 5\n"


def _write_pcd(path, pts):  # binary, 8-byte fields: the values survive exactly
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


def _run(base, name, est, gt, extra="", gt_mme=True):
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
scene_name: planes
save_immediate_result: true
evaluate_mme: true
evaluate_gt_mme: {'true' if gt_mme else 'false'}
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
    est = G.three_planes(1500, seed=21)
    gt = G.three_planes(1200, seed=22, noise=0.01)
    rng = np.random.default_rng(4)
    return np.ascontiguousarray(est[rng.permutation(len(est))]), np.ascontiguousarray(gt[rng.permutation(len(gt))])


def _engine_planes(xyz, max_planes=4):
    from cloud_map_evaluation_amd.engine import Engine

    with Engine(0) as e:
        e.upload(0, xyz)
        return e.segment_planes(0, 0.06, 200, max_planes, 300, refit=True, seed=5)[1]


def _lines(folder):
    return open(folder / "map_results.txt").read().splitlines()


def _mean_rms(planes):
    return sum(p["count"] * p["rms"] for p in planes) / sum(p["count"] for p in planes) if planes else 0.0


def test_rows_equal_engine_to_the_last_digit(scene, tmp_path):
    est, gt = scene
    f = _run(tmp_path, "on", est, gt, "segment_planes: true\nevaluate_mpv: true\n" + KEYS)
    want = [("est", _engine_planes(est)), ("gt", _engine_planes(gt))]
    assert len(want[0][1]) == 3 and len(want[1][1]) == 3
    rows = open(f / "plane_segmentation.txt").read().splitlines()
    assert rows[:6] == ["distance_threshold 0.059999999999999998", "num_iterations 200", "max_planes 4", "min_inliers 300", "seed 5", "refit true"]
    body = [r.split() for r in rows[6:]]
    assert len(body) == 6
    k = 0
    for tag, planes in want:
        for i, p in enumerate(planes):
            r = body[k]
            k += 1
            assert r[0] == tag and [int(v) for v in r[1:4]] == [i, p["count"], p["h"]] and int(r[11]) == p["refit_degenerate"]
            assert [float(v) for v in r[4:11]] == list(p["plane"]) + [p["rms"], p["mean_abs"], p["max_abs"]]  # (%.17g: exact)
    lines = _lines(f)
    i = next(j for j, ln in enumerate(lines) if ln.startswith("LocalGeometry"))
    assert lines[i + 1] == f"Planes est-gt: 3 3 rms {_mean_rms(want[0][1]):.5f} {_mean_rms(want[1][1]):.5f}"


def test_gt_follows_evaluate_gt_mme_and_the_key_off_writes_nothing(scene, tmp_path):
    est, gt = scene
    f = _run(tmp_path, "nogt", est, gt, "segment_planes: true\n" + KEYS, gt_mme=False)
    rows = open(f / "plane_segmentation.txt").read().splitlines()[6:]
    assert len(rows) == 3 and all(r.startswith("est ") for r in rows)
    assert any(ln.startswith("Planes est-gt: 3 rms ") for ln in _lines(f))
    off = _run(tmp_path, "off", est, gt)
    assert not (off / "plane_segmentation.txt").exists() and not any(ln.startswith("Planes") for ln in _lines(off))


def test_remove_outliers_plane_drops_exactly_plane_zero(scene, tmp_path):
    est, gt = scene
    f = _run(tmp_path, "rm", est, gt, "remove_outliers: plane\noutlier_filter_gt: true\n" + KEYS)
    pe, pg = _engine_planes(est, 1)[0], _engine_planes(gt, 1)[0]
    rows = open(f / "outlier_removal.txt").read().splitlines()
    assert rows[0] == "method plane" and rows[-3] == "filter_gt true"
    for row, tag, n, p in ((rows[-2], "est", len(est), pe), (rows[-1], "gt", len(gt), pg)):
        r = row.split()
        assert r[0] == tag and [int(v) for v in r[1:5]] == [n, n - p["count"], p["count"], p["h"]]
        assert [float(v) for v in r[5:]] == list(p["plane"]) + [p["rms"]]
    line = next(ln for ln in _lines(f) if ln.startswith("Estimated-Ground Truth point count:"))
    assert line.split(":")[1].split() == [str(len(est) - pe["count"]), "/", str(len(gt) - pg["count"])]
