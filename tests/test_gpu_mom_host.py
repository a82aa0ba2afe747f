"""The C++ host's evaluate_mom stage on the MI355X: the `MOM est-gt:` line and mom.txt equal Engine.mom on the same file-loaded clouds
to the last digit, the stage runs its two inputs itself without adding their lines or files, and without the key nothing changes."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _globreg_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
PLANE = dict(distance_threshold=0.06, num_iterations=200, max_planes=4, min_inliers=300, refit=True, seed=5)
KEYS = ("plane_distance_threshold: 0.06\nplane_num_iterations: 200\nplane_max_planes: 4\nplane_min_inliers: 300\nplane_seed: 5\n"
        "mpv_radius: 1.5\nmpv_min_points: 6\nmom_parallel_deg: 8\nmom_orthogonal_deg: 12\nmom_min_axis_points: 400\n")
MOM = dict(radius=1.5, min_k=6, parallel_deg=8.0, orthogonal_deg=12.0, min_axis_points=400)


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


@pytest.fixture(scope="module")
def engine_mom(scene):
    from cloud_map_evaluation_amd.engine import Engine

    out = []
    with Engine(0) as e:
        for xyz in scene:
            e.upload(0, xyz, cell_size=0.5)
            out.append(e.mom(0, plane_kwargs=PLANE, **MOM))
    return out


def _lines(folder):
    return open(folder / "map_results.txt").read().splitlines()


def _check(folder, want):
    """want: Engine.mom's dicts, est first, gt when the stage ran on it"""
    line = next(ln for ln in _lines(folder) if ln.startswith("MOM"))
    assert line == ("MOM est-gt: " + " ".join(f"{o['mom_median']:.5f}" for o in want) + " n_axes " + " ".join(str(o["n_axes"]) for o in want))
    rows = open(folder / "mom.txt").read().splitlines()
    assert rows[:5] == ["parallel_deg 8", "orthogonal_deg 12", "min_axis_points 400", "radius 1.5", "min_points 6"]
    body = [r.split() for r in rows[5:]]
    assert len(body) == sum(o["n_axes"] for o in want)
    k = 0
    for tag, o in zip(("est", "gt"), want):
        for a, d in enumerate(o["axes"]):
            r = body[k]
            k += 1
            assert r[0] == tag and [int(v) for v in r[1:6]] == [a, d["direction"], d["n_planes"], d["n_points"], d["n_valid"]]
            assert [float(v) for v in r[6:]] == list(d["rep"]) + [d[f] for f in ("sum_l3", "min", "max", "lower", "upper", "median")]  # (%.17g)


def test_line_and_file_equal_engine_to_the_last_digit(scene, engine_mom, tmp_path):
    est, gt = scene
    assert [o["n_axes"] for o in engine_mom] == [3, 3] and all(o["mom_median"] > 0 for o in engine_mom)
    # with the two input stages on: the MOM line follows the Planes line
    f = _run(tmp_path, "all", est, gt, "evaluate_mom: true\nevaluate_mpv: true\nsegment_planes: true\n" + KEYS)
    _check(f, engine_mom)
    lines = _lines(f)
    i = next(j for j, ln in enumerate(lines) if ln.startswith("Planes est-gt:"))
    assert lines[i + 1].startswith("MOM est-gt: ")
    # alone: it runs both inputs itself and leaves none of their lines or files
    f = _run(tmp_path, "alone", est, gt, "evaluate_mom: true\n" + KEYS)
    _check(f, engine_mom)
    assert not any(ln.startswith(("MPV:", "LocalGeometry", "Planes")) for ln in _lines(f))
    assert not (f / "local_geometry.txt").exists() and not (f / "plane_segmentation.txt").exists()
    # the ground truth follows evaluate_gt_mme, or its own key
    f = _run(tmp_path, "nogt", est, gt, "evaluate_mom: true\n" + KEYS, gt_mme=False)
    _check(f, engine_mom[:1])
    f = _run(tmp_path, "nogt2", est, gt, "evaluate_mom: true\nevaluate_gt_mom: false\nsegment_planes: true\n" + KEYS)
    _check(f, engine_mom[:1])


_SKIP = ("Time", "Path:", "=====")  # (timings, the run's own paths, the dated header)


def test_without_the_key_nothing_changes(scene, tmp_path):
    """a run without the key writes no MOM line and no mom.txt, and a run with the key differs from it by exactly that line and that
    file: every other line and file is byte-identical"""
    est, gt = scene
    off = _run(tmp_path, "off", est, gt, KEYS)
    on = _run(tmp_path, "on", est, gt, "evaluate_mom: true\n" + KEYS)
    names_off = sorted(p.name for p in off.iterdir())
    assert "mom.txt" not in names_off and sorted(p.name for p in on.iterdir()) == sorted(names_off + ["mom.txt"])
    lo = [ln for ln in _lines(off) if not any(s in ln for s in _SKIP)]
    ln_on = [ln for ln in _lines(on) if not any(s in ln for s in _SKIP)]
    assert not any(ln.startswith("MOM") for ln in lo)
    assert [ln for ln in ln_on if not ln.startswith("MOM")] == lo and len(ln_on) == len(lo) + 1
    for name in names_off:
        if name != "map_results.txt":
            assert (on / name).read_bytes() == (off / name).read_bytes(), name
