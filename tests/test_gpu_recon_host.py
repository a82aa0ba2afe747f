"""The C++ host's evaluate_mesh stage on the MI355X: both PLY files are written under the reference's names and read back by
--mesh-info with the counts of reconstruction.txt, which are the Python face's on the same clouds; the map is measured against the
reconstructed ground truth when no mesh file is given; without the key every output file keeps its bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
H, NR = 0.2, 0.5
KEYS = f"mesh_voxel_size: {H}\nmesh_normal_radius: {NR}\nmesh_viewpoint: [2.5, 2.0, 40.0]\n"


def _write_pcd(path, pts):  # binary, 8-byte fields: the values survive exactly
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


def _run(base, name, scene, extra=""):
    est, gt = scene
    d = base / name
    d.mkdir()
    _write_pcd(d / "map.pcd", est)
    _write_pcd(d / "gt.pcd", gt)
    cfg = d / "config.yaml"
    cfg.write_text(f"""registration_methods: 0
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix:
  - [1.0, 0.0, 0.0, 0.0]
  - [0.0, 1.0, 0.0, 0.0]
  - [0.0, 0.0, 1.0, 0.02]
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
{extra}""")
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return d / "map_results"


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(41)

    def surf(n, noise):
        xy = rng.random((n, 2)) * [5.0, 4.0]
        z = 0.3 * np.sin(xy[:, 0]) * np.cos(0.7 * xy[:, 1]) + rng.normal(0, noise, n)
        return np.ascontiguousarray(np.column_stack([xy, z]))

    return surf(7000, 0.004), surf(6000, 0.0)


def _table(path):
    by = {}
    for r in (ln.split() for ln in open(path).read().splitlines()):
        if r[0] in ("est", "gt"):
            by[(r[0], r[1])] = r[2:]
        else:
            by[r[0]] = r[1:]
    return by


def test_both_meshes_are_written_and_counted(scene, tmp_path):
    from cloud_map_evaluation_amd.engine import Engine

    est, gt = scene
    out = _run(tmp_path, "on", scene, "evaluate_mesh: true\nevaluate_mesh_distance: true\n" + KEYS)
    by = _table(out / "reconstruction.txt")
    assert float(by["voxel"][0]) == H and float(by["radius"][0]) == 3.0 * H and (int(by["min_points"][0]), int(by["band"][0])) == (8, 1)
    with Engine(0) as e:
        for slot, tag, pts in ((0, "est", est), (1, "gt", gt)):
            e.upload(slot, pts, cell_size=0.5)
            e.radius_normals(slot, NR, 5, viewpoint=[2.5, 2.0, 40.0])
            d = e.reconstruct(slot, H)
            assert d["n_triangles"] > 500
            for k in ("n_occupied_cells", "n_active_cells", "n_nodes", "n_valid_nodes", "n_cells_extracted", "n_vertices", "n_triangles",
                      "n_degenerate", "sum_k"):
                assert int(by[(tag, k)][0]) == d[k], (tag, k)
            r = subprocess.run([EXE, "--mesh-info", str(out / f"{tag}_mesh.ply")], capture_output=True, text=True, timeout=60)
            assert r.returncode == 0, r.stderr
            info = json.loads(r.stdout)
            assert (info["vertices"], info["triangles"], info["degenerate"]) == (d["n_vertices"], d["n_triangles"], d["n_degenerate"])
            body = (out / f"{tag}_mesh.ply").read_bytes().split(b"end_header\n", 1)[1]
            assert body[:d["n_vertices"] * 24] == d["vertices"].tobytes()  # the file holds the fetched arrays
            if tag == "gt":  # normals towards +z: the surface's upper side is outside
                v, t = d["vertices"], d["triangles"]
                nz = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])[:, 2]
                assert (nz >= 0).mean() > 0.99
    # the map, lifted by 0.02, against the reconstructed ground truth
    lines = open(out / "map_results.txt").read().splitlines()
    err = [ln for ln in lines if ln.startswith("MeshError mean-rmse-max:")]
    assert len(err) == 1 and 0.005 < float(err[0].split()[2]) < 0.04
    md = _table(out / "mesh_distance.txt")
    assert int(md["triangles"][0]) == int(by[("gt", "n_triangles")][0])


_SKIP = ("Time", "Path:", "=====")  # (timings, the run's own paths, the dated header)


def test_without_the_key_nothing_changes(scene, tmp_path):
    off = _run(tmp_path, "off", scene)
    false = _run(tmp_path, "false", scene, "evaluate_mesh: false\n" + KEYS)
    on = _run(tmp_path, "on", scene, "evaluate_mesh: true\n" + KEYS)
    names_off = sorted(p.name for p in off.iterdir())
    assert sorted(p.name for p in false.iterdir()) == names_off
    assert sorted(p.name for p in on.iterdir()) == sorted(names_off + ["est_mesh.ply", "gt_mesh.ply", "reconstruction.txt"])
    keep = lambda folder: [ln for ln in open(folder / "map_results.txt").read().splitlines() if not any(s in ln for s in _SKIP)]
    assert keep(false) == keep(off) == keep(on)
    for name in names_off:
        if name != "map_results.txt":
            assert (false / name).read_bytes() == (off / name).read_bytes(), name
            assert (on / name).read_bytes() == (off / name).read_bytes(), name
