"""The C++ host's evaluate_mpv stage on the MI355X: the `MPV:` / `LocalGeometry` lines and local_geometry.txt agree with Engine to the
printed precision, on the one-call path and on the registration path, and a config without the key gives exactly the lines and files
it gave before the stage existed."""
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


def _run(base, name, est, gt, extra="", using_initial=True, gt_mme=True):
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
scene_name: mpv
save_immediate_result: true
evaluate_mme: true
evaluate_gt_mme: {'true' if gt_mme else 'false'}
nn_radius: 0.1
evaluate_using_initial: {'true' if using_initial else 'false'}
vmd_voxel_size: 0.5
downsample_size: 0.0
enable_debug: false
{extra}""")
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return d / "map_results"


@pytest.fixture(scope="module")
def scene():
    from cloud_map_evaluation_amd import synth

    est, gt = synth.scan_pair(100_000, density=2500.0, seed=81)
    return est.numpy(), gt.numpy()


def _engine_info(xyz, r, min_k):
    from cloud_map_evaluation_amd.engine import Engine

    with Engine(0) as e:
        e.upload(0, xyz, cell_size=0.1)
        return e.local_geometry(0, r, min_k)


def _lines(folder):
    return open(folder / "map_results.txt").read().splitlines()


_FEAT = ("linearity", "planarity", "sphericity", "surface_variation")


def _check(folder, infos, r, min_k):
    """infos: Engine's dicts, est first, gt when the stage ran on it"""
    lines = _lines(folder)
    i = next(j for j, ln in enumerate(lines) if ln.startswith("MME: "))
    assert lines[i + 1] == "MPV: " + " ".join(f"{o['mpv']:.5f}" for o in infos)
    assert lines[i + 2] == "LocalGeometry lin-plan-sph-sv: " + " ".join(f"{o[f]:.5f}" for o in infos for f in _FEAT)
    rows = open(folder / "local_geometry.txt").read().splitlines()
    assert rows[0].split()[0] == "radius" and float(rows[0].split()[1]) == r
    assert rows[1] == f"min_points {min_k}"
    assert len(rows) == 2 + len(infos)
    for row, o, tag in zip(rows[2:], infos, ("est", "gt")):
        f = row.split()
        assert f[0] == tag and int(f[1]) == o["n"] and int(f[2]) == o["n_valid"]
        want = [o["mean_k"], o["mpv"]] + [o[x] for x in _FEAT]
        assert [float(v) for v in f[3:]] == want  # (%.17g: the doubles survive exactly)


def test_one_call_path_matches_engine(scene, tmp_path):
    est, gt = scene
    f = _run(tmp_path, "on", est, gt, "evaluate_mpv: true\n")
    # the stage runs on the clouds as loaded (before initial_matrix moves the map)
    _check(f, [_engine_info(est, 0.1, 5), _engine_info(gt, 0.1, 5)], 0.1, 5)


def test_keys_and_the_registration_path(scene, tmp_path):
    est, gt = scene
    f = _run(tmp_path, "reg", est, gt, "evaluate_mpv: true\nmpv_radius: 0.15\nmpv_min_points: 8\nevaluate_gt_mpv: false\n", using_initial=False)
    _check(f, [_engine_info(est, 0.15, 8)], 0.15, 8)
    f = _run(tmp_path, "nogt", est, gt, "evaluate_mpv: true\n", gt_mme=False)  # evaluate_gt_mpv follows evaluate_gt_mme
    _check(f, [_engine_info(est, 0.1, 5)], 0.1, 5)


_SKIP = ("Time", "Path:", "=====")  # (timings, the run's own paths, the dated header)


def test_without_the_key_nothing_changes(scene, tmp_path):
    """a run without the key writes no MPV / LocalGeometry line and no local_geometry.txt, and a run with the key differs from it by
    exactly those two lines and that one file: every other line and file is byte-identical"""
    est, gt = scene
    off = _run(tmp_path, "off", est, gt)
    on = _run(tmp_path, "on", est, gt, "evaluate_mpv: true\n")
    names_off = sorted(p.name for p in off.iterdir())
    assert "local_geometry.txt" not in names_off
    assert sorted(p.name for p in on.iterdir()) == sorted(names_off + ["local_geometry.txt"])
    lo = [ln for ln in _lines(off) if not any(s in ln for s in _SKIP)]
    ln_on = [ln for ln in _lines(on) if not any(s in ln for s in _SKIP)]
    assert not any(ln.startswith(("MPV:", "LocalGeometry")) for ln in lo)
    assert [ln for ln in ln_on if not ln.startswith(("MPV:", "LocalGeometry"))] == lo
    assert len(ln_on) == len(lo) + 2
    for name in names_off:
        if not name.endswith(".txt"):
            assert open(off / name, "rb").read() == open(on / name, "rb").read(), name
        elif name != "map_results.txt":
            assert open(off / name).read() == open(on / name).read(), name
