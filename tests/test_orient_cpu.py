"""me_orient_normals without a GPU: the numpy model (tests/_orient_ref.py) against hand-worked cases and against two analytic scenes,
the bindings, and the C++ host's three keys through --parse-config."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np

import _orient_ref as R
from test_mesh_host_cpu import _BASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
Z = (0.0, 0.0, 1.0)

# the scenes that the GPU tests use: the model alone orients 100 % of them (asserted below)
TORUS_N, TORUS_SEED, TORUS_K = 12_000, 5, 12
SHELL_N, SHELL_SEED, SHELL_K = 2_500, 6, 12


def _line(n):
    return np.stack([np.arange(n, dtype=np.float64), np.zeros(n), np.zeros(n)], axis=1)


def _check(o, **want):
    for k, v in want.items():
        got = o[k].tolist() if isinstance(o[k], np.ndarray) else o[k]
        assert got == v, (k, got, v)


def test_chain_of_five_with_alternating_signs():
    # lists (k + 1 = 2): 0:[0,1] 1:[1,0] (0 and 2 tie, the lower index wins) 2:[2,1] 3:[3,2] 4:[4,3]; every c = -1
    nrm = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, 1]], np.float64)
    o = R.orient(_line(5), nrm, 1, Z)
    _check(o, n=5, n_valid=5, n_components=1, largest_component=5, n_tree_edges=4, n_graph_edges=4, n_flipped=2, n_inconsistent_edges=0,
           tree=[(0, 1), (1, 2), (2, 3), (3, 4)], roots=[0], component=[0] * 5, flipped=[False, True, False, True, False])
    assert np.array_equal(o["normals"], np.tile([0.0, 0.0, 1.0], (5, 1)))


def test_two_separated_triples():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [100, 0, 5], [101, 0, 5], [102, 0, 5]], np.float64)
    nrm = np.array([[0, 0, 1], [0, 0, -1], [0, 0.6, 0.8], [0, 0, -1], [0, 0, -1], [0, 0, 1]], np.float64)
    # c01 = -1, c02 = 0.8, c12 = -0.8; c34 = 1, c35 = -1, c45 = -1.  Order: |c| = 1 by (lo, hi): (0,1) (3,4) (3,5) (4,5); then (0,2) (1,2)
    o = R.orient(xyz, nrm, 2, Z)
    _check(o, n=6, n_valid=6, n_components=2, largest_component=3, n_tree_edges=4, n_graph_edges=6, n_flipped=3, n_inconsistent_edges=0,
           tree=[(0, 1), (3, 4), (3, 5), (0, 2)], roots=[0, 3], component=[0, 0, 0, 1, 1, 1],
           flipped=[False, True, False, True, True, False])


def test_root_tie_and_inward():
    xyz = np.array([[0, 0, 0], [1, 0, 2], [2, 0, 2]], np.float64)  # 1 and 2 share the top projection: the root is 1
    nrm = np.array([[0, 0, 1], [0, 0, -1], [0, 0, -1]], np.float64)
    o = R.orient(xyz, nrm, 2, Z)
    _check(o, roots=[1], tree=[(0, 1), (0, 2)], flipped=[False, True, True], n_flipped=2, n_inconsistent_edges=0)
    o = R.orient(xyz, nrm, 2, Z, inward=True)
    _check(o, roots=[1], flipped=[True, False, False], n_flipped=1)
    # -0.0 and +0.0 are one value: the tie goes to the lower index
    o = R.orient(np.array([[0, 0, 0.0], [1, 0, -0.0]]), np.array([[0, 0, 1.0], [0, 0, 1.0]]), 1, Z)
    _check(o, roots=[0])


def test_c_equal_zero_does_not_flip_and_a_zero_root_product():
    xyz = np.array([[0, 0, 1], [1, 0, 0]], np.float64)
    nrm = np.array([[1, 0, 0], [0, 1, 0]], np.float64)
    o = R.orient(xyz, nrm, 1, Z)  # root 0, n . d = 0: not flipped
    _check(o, roots=[0], tree=[(0, 1)], flipped=[False, False], n_inconsistent_edges=0)
    o = R.orient(xyz, nrm, 1, Z, inward=True)  # a product of exactly 0 counts as flipped with inward set
    _check(o, flipped=[True, True], n_flipped=2, n_inconsistent_edges=0)
    # c = -0.0: |c| = 0, not negative
    o = R.orient(xyz, np.array([[-1, 0, 0], [0, -1, -1]], np.float64), 1, (0.0, 0.0, -1.0))
    _check(o, roots=[1], flipped=[False, False])


def test_invalid_point_in_the_middle_of_a_chain():
    nrm = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 0], [0, 0, -1], [0, 0, 1]], np.float64)
    # k = 1: 1 lists 0 (tie with 2), 3 lists the invalid 2 — skipped, not replaced —, 4 lists 3
    o = R.orient(_line(5), nrm, 1, Z)
    _check(o, n=5, n_valid=4, n_components=2, largest_component=2, n_tree_edges=2, n_graph_edges=2, n_flipped=2, n_inconsistent_edges=0,
           tree=[(0, 1), (3, 4)], roots=[0, 3], component=[0, 0, -1, 1, 1], flipped=[False, True, False, True, False])
    assert np.array_equal(o["normals"][2], [0, 0, 0])


def test_duplicates_beyond_the_list_and_the_list_order():
    xyz = np.zeros((5, 3))
    lists = R.knn_lists(xyz, 3)
    assert lists.tolist() == [[0, 1, 2]] * 5  # (d2, index): point 4 is not in its own list
    assert R.knn_lists(_line(2), 4).tolist() == [[0, 1, -1, -1], [1, 0, -1, -1]]
    o = R.orient(xyz, np.tile([0.0, 0.0, 1.0], (5, 1)), 2, Z)
    _check(o, n_graph_edges=9, n_tree_edges=4, tree=[(0, 1), (0, 2), (0, 3), (0, 4)])  # 3 and 4 have k + 1 = 3 edges each


def test_torus_is_oriented_completely():
    xyz, true, nrm = R.torus(TORUS_N, TORUS_SEED)
    o = R.orient(xyz, nrm, TORUS_K, Z)
    assert o["n_components"] == 1 and o["n_inconsistent_edges"] == 0
    assert np.all(R.dot3(o["normals"], true) > 0)  # the top of a torus about z has an outward normal along +z
    assert np.array_equal(np.abs(o["normals"]), np.abs(nrm))


def test_shell_pair_has_two_components_and_inward_roots():
    xyz, true, nrm = R.shells(SHELL_N, SHELL_SEED)
    o = R.orient(xyz, nrm, SHELL_K, Z)
    assert o["n_components"] == 2 and o["largest_component"] == SHELL_N and o["n_inconsistent_edges"] == 0
    assert np.all(R.dot3(o["normals"], true) > 0)
    assert np.array_equal(o["component"], np.repeat([0, 1], SHELL_N).astype(np.int32))
    i = R.orient(xyz, nrm, SHELL_K, Z, inward=True)
    assert np.all(R.dot3(i["normals"], true) < 0) and i["n_inconsistent_edges"] == 0
    assert np.array_equal(i["flipped"], ~o["flipped"])


def test_bindings_and_struct_layout():
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import Engine

    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mapeval_hip.h")).read()
    for s in ("me_orient_normals", "me_orient_fetch"):
        assert s in _lib.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr)
    assert C.sizeof(_lib.OrientParams) == 32 and C.sizeof(_lib.OrientOut) == 64
    assert [k for k, _ in _lib.OrientOut._fields_] == list(R.FIELDS)
    assert callable(Engine.orient_normals) and callable(Engine.orient_fetch)
    assert "orient_k" in Engine.reconstruct.__code__.co_varnames


def _parse(tmp_path, extra):
    cfg = tmp_path / "c.yaml"
    cfg.write_text(_BASE + extra)
    return subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)


def test_host_keys(tmp_path):
    ok = "evaluate_mesh: true\nmesh_voxel_size: 0.1\n"
    for extra in ("", ok):  # without the keys: the defaults
        r = _parse(tmp_path, extra)
        assert r.returncode == 0, r.stderr
        p = json.loads(r.stdout)
        assert (p["mesh_orient"], p["mesh_orient_k"], p["mesh_orient_inward"]) == ("viewpoint", 12, False)
    r = _parse(tmp_path, ok + "mesh_orient: propagate\nmesh_orient_k: 39\nmesh_orient_inward: true\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["mesh_orient"], p["mesh_orient_k"], p["mesh_orient_inward"], p["mesh_viewpoint"]) == ("propagate", 39, True, None)
    assert _parse(tmp_path, ok + "mesh_orient: viewpoint\nmesh_viewpoint: [1, 2, 3]\nmesh_orient_k: 1\n").returncode == 0
    for extra, words in ((ok + "mesh_orient: tangent\n", ("mesh_orient",)),
                         (ok + "mesh_orient_k: 0\n", ("mesh_orient_k",)),
                         (ok + "mesh_orient_k: 40\n", ("mesh_orient_k",)),
                         (ok + "mesh_orient_k: 2.5\n", ("mesh_orient_k",)),
                         (ok + "mesh_orient_inward: maybe\n", ("mesh_orient_inward",)),
                         (ok + "mesh_orient: propagate\nmesh_viewpoint: [1, 2, 3]\n", ("mesh_viewpoint", "mesh_orient")),
                         (ok + "mesh_orient: propagate\nnum_gpus: 2\n", ("evaluate_mesh: single GPU only",))):
        r = _parse(tmp_path, extra)
        assert r.returncode != 0 and all(w in r.stderr for w in words), (extra, r.stderr)
    # with the stage off nothing of it is judged
    assert _parse(tmp_path, "evaluate_mesh: false\nmesh_orient: tangent\nmesh_orient_k: 99\n").returncode == 0
