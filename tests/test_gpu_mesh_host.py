"""The C++ host's evaluate_mesh_distance stage on the MI355X: the two lines of map_results.txt carry the Python face's numbers at the
printed precision, mesh_distance.txt carries the counts, quantiles and F-scores of Engine.mesh_report on the same files, and without
the keys nothing changes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _mesh_ref as R
import _ply_mesh_files as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
T = np.eye(4)
T[0, 3] = 0.05
T[:2, :2] = [[0.8, -0.6], [0.6, 0.8]]
THS, MAXD, NS, SEED = [0.1, 0.03, 0.01], 0.03, 5000, 9  # (noise of 0.02 per axis: the gate bites)
KEYS = f"gt_mesh_path: MESH\nmesh_thresholds: {THS}\nmesh_max_distance: {MAXD}\nmesh_sample_points: {NS}\nmesh_seed: {SEED}\n"


def _write_pcd(path, pts):  # binary, 8-byte fields: the values survive exactly
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


def _run(base, name, scene, extra=""):
    v, tri, est, gt = scene
    d = base / name
    d.mkdir()
    _write_pcd(d / "map.pcd", est)
    _write_pcd(d / "gt.pcd", gt)
    F.write_ply_mesh(d / "gt_mesh.ply", v, [tuple(t) for t in tri], binary=True)
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
scene_name: field
save_immediate_result: true
evaluate_mme: true
evaluate_gt_mme: true
nn_radius: 0.5
evaluate_using_initial: true
vmd_voxel_size: 2.0
downsample_size: 0.0
enable_debug: false
{extra.replace('MESH', str(d / 'gt_mesh.ply'))}""")
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return d / "map_results"


@pytest.fixture(scope="module")
def scene():
    from cloud_map_evaluation_amd import synth

    v, tri = synth.heightfield_mesh(24, 20, 0.5, 0.6, seed=21)
    rng = np.random.default_rng(22)
    on_mesh = R.sample(v, tri, 6000, 1)[0] + rng.normal(0, 0.02, (6000, 3))
    est = (on_mesh - T[:3, 3]) @ T[:3, :3]  # the map as loaded: the initial matrix brings it back onto the mesh
    gt = R.sample(v, tri, 5000, 2)[0]
    return v, tri, np.ascontiguousarray(est), np.ascontiguousarray(gt)


def _lines(folder):
    return open(folder / "map_results.txt").read().splitlines()


def test_lines_and_file_equal_engine(scene, tmp_path):
    from cloud_map_evaluation_amd.engine import Engine

    v, tri, est, gt = scene
    with Engine(0) as e:
        e.upload(0, est, cell_size=0.5)
        e.upload(1, gt, cell_size=0.5)
        e.transform_cloud(0, T)  # (the host's calls, in the host's order)
        e.mesh_upload(v, tri)
        info = e.mesh_info()
        rep = e.mesh_report(THS, sample_points=NS, seed=SEED, max_distance=MAXD)
    assert 0 < rep["n_matched"] < rep["n_query"] == 6000
    out = _run(tmp_path, "on", scene, "evaluate_mesh_distance: true\n" + KEYS)
    lines = _lines(out)
    err = [ln for ln in lines if ln.startswith("MeshError mean-rmse-max:")]
    ac = [ln for ln in lines if ln.startswith("MeshAC @t:")]
    assert err == [f"MeshError mean-rmse-max: {rep['mean']:.5f} {rep['rmse']:.5f} {rep['max']:.5f}"]
    assert ac == ["MeshAC @t:" + "".join(f" {t:.5f} {n / rep['n_matched']:.5f}" for t, n in zip(THS, rep["n_within"]))]
    order = [ln.split(":")[0] for ln in lines]
    assert order.index("MeshError mean-rmse-max") + 1 == order.index("MeshAC @t") < order.index("VMD")
    assert order.index("FULL CD") < order.index("MeshError mean-rmse-max")
    rows = [r.split() for r in open(out / "mesh_distance.txt").read().splitlines()]
    by = {}
    for r in rows:
        by.setdefault(r[0], []).append(r[1:])
    assert (int(by["vertices"][0][0]), int(by["triangles"][0][0]), int(by["degenerate"][0][0]), int(by["depth"][0][0])) == (
        info["vertices"], info["triangles"], 0, info["depth"])
    assert float(by["area"][0][0]) == info["area"] and [float(x) for x in by["bbox"][0]] == info["bbox_lo"].tolist() + info["bbox_hi"].tolist()
    t = by["totals"][0]
    assert [int(t[0]), int(t[1]), int(t[2]), int(t[6])] == [rep["n_query"], rep["n_matched"], rep["n_face"], rep["worst_index"]]
    assert float(t[5]) == rep["max"]
    # (a sum is formed in the order of the slot's index: any order of n terms agrees within n 2^-52 of the sum of the magnitudes)
    n = rep["n_matched"]
    assert abs(float(t[3]) - rep["sum_d"]) <= n * 2.0 ** -52 * rep["sum_d"] and abs(float(t[4]) - rep["sum_d2"]) <= n * 2.0 ** -52 * rep["sum_d2"]
    s = by["signed"][0]
    assert abs(float(s[0]) - rep["sum_signed"]) <= n * 2.0 ** -52 * rep["sum_abs_signed"]
    assert [int(r[1]) for r in by["t"]] == rep["n_within"].tolist() and [float(r[0]) for r in by["t"]] == THS
    assert [float(r[0]) for r in by["q"]] == [0.5, 0.9, 0.95, 0.99] and [int(r[1]) for r in by["q"]] == rep["rank"].tolist()
    assert [float(r[2]) for r in by["q"]] == rep["quantile_d"].tolist()
    sm = rep["sampled"]
    assert [[float(x) for x in r[1:]] for r in by["f"]] == [[sm["precision"][k], sm["recall"][k], sm["fscore"][k]] for k in range(len(THS))]
    assert [int(by["sampled"][0][1]), int(by["sampled"][1][1])] == [6000, NS]


_SKIP = ("Time", "Path:", "=====")  # (timings, the run's own paths, the dated header)


def test_without_the_keys_nothing_changes(scene, tmp_path):
    """a run without the keys equals, byte for byte, a run that sets the stage to false; a run with the stage differs from both by
    exactly its two lines and its file"""
    off = _run(tmp_path, "off", scene)
    false = _run(tmp_path, "false", scene, "evaluate_mesh_distance: false\n" + KEYS)
    on = _run(tmp_path, "on", scene, "evaluate_mesh_distance: true\n" + KEYS)
    names_off = sorted(p.name for p in off.iterdir())
    assert "mesh_distance.txt" not in names_off and sorted(p.name for p in false.iterdir()) == names_off
    assert sorted(p.name for p in on.iterdir()) == sorted(names_off + ["mesh_distance.txt"])
    keep = lambda folder: [ln for ln in _lines(folder) if not any(s in ln for s in _SKIP)]
    lo, lf, ln_on = keep(off), keep(false), keep(on)
    assert lf == lo and not any(ln.startswith("Mesh") for ln in lo)
    assert [ln for ln in ln_on if not ln.startswith(("MeshError", "MeshAC"))] == lo and len(ln_on) == len(lo) + 2
    for name in names_off:
        if name != "map_results.txt":
            assert (false / name).read_bytes() == (off / name).read_bytes(), name
            assert (on / name).read_bytes() == (off / name).read_bytes(), name
