"""The C++ host's remove_outliers: cluster on the MI355X: a run on PCD files of a map with ghosts writes the result files of a run
without the key on a PCD of the model's kept points (tests/_cluster_ref.py), and outlier_removal.txt carries the model's counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _cluster_ref as R

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


def _run(base, name, est, gt, extra=""):
    d = base / name
    d.mkdir()
    _write_pcd(d / "map.pcd", est)
    _write_pcd(d / "gt.pcd", gt)
    cfg = d / "config.yaml"
    cfg.write_text(f"""registration_methods: 2
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix:
  - [1.0, 0.0, 0.0, 0.0]
  - [0.0, 1.0, 0.0, 0.0]
  - [0.0, 0.0, 1.0, 0.0]
  - [0.0, 0.0, 0.0, 1.0]
estimate_map_path: {d}
gt_map_path: {d / 'gt.pcd'}
scene_name: ghosts
save_immediate_result: true
evaluate_mme: true
evaluate_gt_mme: true
nn_radius: 0.1
evaluate_using_initial: true
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


def _with_ghosts(xyz, rng, n_blobs):
    lo, hi = xyz.min(0), xyz.max(0)
    parts = [xyz]
    for _ in range(n_blobs):
        c = np.array([rng.uniform(lo[0], hi[0]), rng.uniform(lo[1], hi[1]), hi[2] + rng.uniform(2.0, 5.0)])
        parts.append(c + rng.normal(0.0, 0.05, (int(rng.integers(200, 2001)), 3)))
    out = np.concatenate(parts)
    return out[rng.permutation(len(out))]


def _line(lines, who):
    return [ln.split() for ln in lines if ln.startswith(who + " ")][0]


def test_cluster_equals_a_run_on_the_models_kept_points(tmp_path):
    from cloud_map_evaluation_amd import synth

    est, gt = synth.scan_pair(200_000, density=2500.0, seed=61, outlier_ratio=0.003)
    rng = np.random.default_rng(78)
    est, gt = _with_ghosts(est.numpy(), rng, 8), _with_ghosts(gt.numpy(), rng, 3)
    eps, mp, size = 0.1, 10, 5000
    kept, rows = [], []
    for xyz in (est, gt):
        labels, counts, m = R.dbscan(xyz, eps, mp)
        keep = R.cluster_keep(labels, m, size)
        core = counts >= mp
        rows.append([len(xyz), m, int(core.sum()), int(((labels >= 0) & ~core).sum()), int((labels < 0).sum()),
                     int(R.cluster_sizes(labels, m).max()), int(keep.sum())])
        kept.append(xyz[keep])
    assert 0 < len(kept[0]) < len(est) - 1600 and 0 < len(kept[1]) < len(gt) - 600  # the ghosts are gone
    f1 = _run(tmp_path, "filtered", est, gt, f"remove_outliers: cluster\noutlier_eps: {eps}\noutlier_min_points: {mp}\n"
                                              f"outlier_min_cluster_size: {size}\noutlier_filter_gt: true\n")
    f0 = _run(tmp_path, "kept", kept[0], kept[1])
    _same_results(f1, f0)
    lines = open(f1 / "outlier_removal.txt").read().splitlines()
    assert lines[:6] == ["method cluster", "eps 0.10000000000000001", "min_points 10", "min_cluster_size 5000", "keep_largest 0",
                         "filter_gt true"]
    assert [int(v) for v in _line(lines, "est")[1:]] == rows[0]
    assert [int(v) for v in _line(lines, "gt")[1:]] == rows[1]
    assert len(lines) == 8 and not (f0 / "outlier_removal.txt").exists()
    # the map alone, the largest cluster only
    f2 = _run(tmp_path, "largest", est, gt, f"remove_outliers: cluster\noutlier_eps: {eps}\noutlier_keep_largest: 1\n")
    lines = open(f2 / "outlier_removal.txt").read().splitlines()
    assert len(lines) == 7 and lines[4] == "keep_largest 1" and lines[5] == "filter_gt false"
    assert int(_line(lines, "est")[7]) == rows[0][5]  # kept = the largest cluster's size
