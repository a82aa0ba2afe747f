"""The C++ host's mesh keys through --parse-config (defaults, values read, refusals that name the key) and the PLY mesh reader through
--mesh-info on files written here: ascii and binary, uchar and int list counts, a quad, an extra face property, an edge element after
the faces, and the three malformed files.  No GPU needed."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import _mesh_ref as R
import _ply_mesh_files as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")

_BASE = """registration_methods: 2
icp_max_distance: 1.5
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
save_immediate_result: false
evaluate_mme: true
evaluate_gt_mme: true
evaluate_using_initial: true
nn_radius: 0.15
vmd_voxel_size: 3.0
downsample_size: 0.0
estimate_map_path: /nonexistent/est
gt_map_path: /nonexistent/gt.pcd
scene_name: s
enable_debug: false
"""


def _parse(tmp_path, extra):
    cfg = tmp_path / "c.yaml"
    cfg.write_text(_BASE + extra)
    return subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)


def test_defaults():
    import tempfile, pathlib

    with tempfile.TemporaryDirectory() as d:
        r = _parse(pathlib.Path(d), "")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["evaluate_mesh_distance"] is False and p["gt_mesh_path"] == ""
    assert p["mesh_thresholds"] == p["accuracy_level"] == [0.2, 0.1, 0.08, 0.05, 0.01]
    assert p["mesh_max_distance"] == math.inf and p["mesh_sample_points"] == 0 and p["mesh_seed"] == 0


def test_keys_are_read(tmp_path):
    r = _parse(tmp_path, "evaluate_mesh_distance: true\ngt_mesh_path: /data/gt.ply\nmesh_thresholds: [0.5, 0.25]\nmesh_max_distance: 2.5\n"
                         "mesh_sample_points: 100000\nmesh_seed: 7\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["evaluate_mesh_distance"], p["gt_mesh_path"], p["mesh_thresholds"], p["mesh_max_distance"], p["mesh_sample_points"],
            p["mesh_seed"]) == (True, "/data/gt.ply", [0.5, 0.25], 2.5, 100000, 7)
    for v in ("0", "-1"):  # <= 0 means every point
        r = _parse(tmp_path, f"evaluate_mesh_distance: true\ngt_mesh_path: /data/gt.ply\nmesh_max_distance: {v}\n")
        assert r.returncode == 0 and json.loads(r.stdout)["mesh_max_distance"] == math.inf


def test_seed_and_count_are_whole_numbers_and_the_path_is_escaped(tmp_path):
    ok = "evaluate_mesh_distance: true\n"
    big = 2 ** 63 + 12345  # (above 2^53: a double would round it)
    r = _parse(tmp_path, ok + f"gt_mesh_path: /data/a\\b.ply\nmesh_seed: {big}\nmesh_sample_points: 2147483647\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["mesh_seed"], p["mesh_sample_points"], p["gt_mesh_path"]) == (big, 2 ** 31 - 1, "/data/a\\b.ply")
    for extra, key in (("mesh_seed: -1\n", "mesh_seed"), ("mesh_seed: 1.5\n", "mesh_seed"), ("mesh_seed: 1e3\n", "mesh_seed"),
                       (f"mesh_seed: {2 ** 64}\n", "mesh_seed"), ("mesh_sample_points: -5\n", "mesh_sample_points"),
                       ("mesh_sample_points: 10.5\n", "mesh_sample_points"), ("mesh_sample_points: 2147483648\n", "mesh_sample_points")):
        r = _parse(tmp_path, ok + "gt_mesh_path: /data/gt.ply\n" + extra)
        assert r.returncode != 0 and key in r.stderr, (extra, r.stderr)


def test_refusals_name_the_key(tmp_path):
    ok = "evaluate_mesh_distance: true\ngt_mesh_path: /data/gt.ply\n"
    for extra, key in ((ok + "num_gpus: 2\n", "evaluate_mesh_distance: single GPU only (num_gpus must be 1)"),
                       ("evaluate_mesh_distance: true\n", "gt_mesh_path"),
                       (ok + "mesh_thresholds: [0.1, -0.2]\n", "mesh_thresholds"),
                       (ok + "mesh_thresholds: [1, 2, 3, 4, 5, 6, 7, 8, 9]\n", "mesh_thresholds: at most 8")):
        r = _parse(tmp_path, extra)
        assert r.returncode != 0 and key in r.stderr, (extra, r.stderr)
    # with the stage off nothing of it is judged
    assert _parse(tmp_path, "evaluate_mesh_distance: false\nnum_gpus: 2\nmesh_thresholds: [-1]\n").returncode == 0


def _info(path):
    return subprocess.run([EXE, "--mesh-info", str(path)], capture_output=True, text=True, timeout=60)


V = np.array([[0.0, 0, 0], [2, 0, 0], [2, 1, 0.5], [0, 1, 0.5], [1, 3, 1], [9, 9, 9]])  # (vertex 5 is unreferenced)
FACES = [(0, 1, 2, 3), (3, 2, 4), (0, 0, 1)]  # a quad, a triangle, a degenerate one


@pytest.mark.parametrize("binary,count_type,index_type,list_name,extra,edges",
                         [(False, "uchar", "int", "vertex_indices", False, 0), (True, "uchar", "int", "vertex_indices", False, 0),
                          (True, "int", "uint", "vertex_index", False, 0), (False, "int", "int", "vertex_index", True, 2),
                          (True, "uchar", "ushort", "vertex_indices", True, 3), (True, "ushort", "int", "vertex_indices", False, 1)])
def test_mesh_info(tmp_path, binary, count_type, index_type, list_name, extra, edges):
    path = F.write_ply_mesh(tmp_path / "m.ply", V, FACES, binary, count_type, index_type, list_name, "double", extra, edges)
    r = _info(path)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    tri = F.fan(FACES)
    assert tri.tolist() == [[0, 1, 2], [0, 2, 3], [3, 2, 4], [0, 0, 1]]
    area, deg = R.areas(V, tri)
    ref = V[np.unique(tri)]
    assert got == {"vertices": 6, "triangles": 4, "degenerate": int(deg.sum()), "area": float(np.cumsum(area)[-1]),
                   "bbox": ref.min(0).tolist() + ref.max(0).tolist()}


def test_float_vertices(tmp_path):
    r = _info(F.write_ply_mesh(tmp_path / "f.ply", V, FACES[:2], True, vertex_type="float"))
    assert r.returncode == 0 and json.loads(r.stdout)["triangles"] == 3


def test_malformed_files_fail_with_a_message(tmp_path):
    good = F.write_ply_mesh(tmp_path / "good.ply", V, FACES, True)
    data = open(good, "rb").read()
    cut = tmp_path / "cut.ply"
    cut.write_bytes(data[:-5])  # ends inside the last face
    r = _info(cut)
    assert r.returncode != 0 and "truncated" in r.stderr
    cutv = tmp_path / "cutv.ply"
    cutv.write_bytes(data[:data.index(b"end_header\n") + 11 + 40])  # ends inside the vertices
    r = _info(cutv)
    assert r.returncode != 0 and "truncated" in r.stderr
    for binary in (True, False):
        r = _info(F.write_ply_mesh(tmp_path / "range.ply", V, [(0, 1, 6)], binary))  # an index equal to n_vertices
        assert r.returncode != 0 and "outside" in r.stderr
        r = _info(F.write_ply_mesh(tmp_path / "two.ply", V, [(0, 1, 2), (0, 1)], binary))  # a list count of 2
        assert r.returncode != 0 and "fewer than 3" in r.stderr
    r = _info(F.write_ply_mesh(tmp_path / "neg.ply", V, [(0, 1, -1)], True))
    assert r.returncode != 0
    acut = tmp_path / "acut.ply"
    text = open(F.write_ply_mesh(tmp_path / "a.ply", V, FACES, False)).read()
    acut.write_text(text[:text.rindex("3 ")])
    r = _info(acut)
    assert r.returncode != 0 and "truncated" in r.stderr
    word = tmp_path / "word.ply"  # a token that is not a number is refused, not read as 0
    word.write_text(text.replace("3 3 2 4", "3 3 two 4"))
    assert "3 3 two 4" in word.read_text()
    r = _info(word)
    assert r.returncode != 0 and "'two'" in r.stderr and "not a number" in r.stderr
    assert _info(tmp_path / "missing.ply").returncode != 0
