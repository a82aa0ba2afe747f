"""The numpy models of tests/_surface_ref.py against hand-computed cases, the Rayleigh bound the GPU test relies on, and the ctypes
layouts of the new structs against include/mapeval_hip.h.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np

import _surface_ref as R
from cloud_map_evaluation_amd import _lib


def _grid(nx, ny, h):
    g = np.stack(np.meshgrid(np.arange(nx) * h, np.arange(ny) * h, indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g, np.zeros((len(g), 1))], 1)


def test_known_plane():
    xyz = _grid(9, 9, 0.05)
    m = R.radius_normals(xyz, 0.11, 5)
    mid = 4 * 9 + 4
    assert m["k"][mid] == 12  # the 4 + 4 + 4 lattice points at 0.05, 0.0707 and 0.1 (0.1118 is outside)
    assert m["valid"].all()
    assert np.all(np.abs(m["eig"][:, 0]) <= 1e-18) and np.all(np.abs(np.abs(m["normal"][:, 2]) - 1.0) <= 1e-15)


def test_known_tilt():
    a, c = np.array([0.8, 0.0, 0.6]), np.array([0.0, 1.0, 0.0])
    g = _grid(9, 9, 0.05)
    xyz = g[:, :1] * a + g[:, 1:2] * c
    m = R.radius_normals(xyz, 0.11, 5)
    want = np.array([-0.6, 0.0, 0.8])
    assert m["valid"].all()
    assert np.all(R.cross_norm(m["normal"], np.broadcast_to(want, m["normal"].shape)) <= 1e-12)
    assert np.all(np.abs(R.norm_ld(m["normal"]) - 1.0) <= 4 * R.EPS)


def test_collinear_points_are_valid_with_two_zero_eigenvalues():
    xyz = np.zeros((40, 3))
    xyz[:, 0] = np.arange(40) * 0.02
    m = R.radius_normals(xyz, 0.11, 5)
    assert m["valid"].all() and np.all(m["k"][5:-5] == 10)
    assert np.all(np.abs(m["eig"][:, :2]) <= 1e-18) and np.all(m["eig"][:, 2] > 1e-4)
    assert np.all(np.abs(m["normal"][:, 0]) <= 1e-12)  # any unit vector across the line


def test_neighbour_rule_is_strict_and_keeps_duplicates():
    xyz = np.array([[0.0, 0, 0], [0.5, 0, 0], [np.nextafter(0.5, 0), 0, 0], [0.0, 0, 0], [0.0, 0, 0]])
    assert R.neighbours(xyz, 0, 0.5).tolist() == [2, 3, 4]


def test_surface_error_by_hand():
    r_xyz = np.array([[0.0, 0, 0], [10.0, 0, 0], [20.0, 0, 0], [30.0, 0, 0]])
    r_nrm = np.array([[0.0, 0, 1], [0.6, 0, 0.8], [0.0, 0, 0], [0.0, 1, 0]])
    q_xyz = np.array([[0.0, 0, 1], [11.0, 0, 0], [20.0, 0, 0.5], [30.0, 2, 0], [30.0, -3, 4], [0.0, 0, 0.25]])
    idx = np.array([0, 1, 2, 3, 3, 0])
    d = q_xyz - r_xyz[idx]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    d2[5] = -1.0  # no neighbour
    q_nrm = np.array([[0.0, 0, 1], [0.0, 0, 1], [0.0, 0, 1], [0.0, 0, 0], [0.0, -1, 0], [0.0, 0, 1]])
    e, c, o = R.surface_error(q_xyz, r_xyz, idx, d2, r_nrm, q_nrm, taus=(0.6, 1.0, 2.9), cos_min=(0.8, 0.9, 1.0))
    assert e.tolist() == [1.0, 0.6, -1.0, 2.0, 3.0, -1.0]  # the zero reference normal and the missing neighbour are unused
    assert c.tolist() == [1.0, 0.8, -1.0, -1.0, 1.0, -1.0]  # the zero query normal is used but not normal-used
    assert (o["n_query"], o["n_used"], o["n_normal_used"]) == (5, 4, 3)
    assert o["t2"][:2].tolist() == [0.0, 1.0 - 0.6 * 0.6] and o["t2"][4] == 25.0 - 9.0
    assert (o["max_e"], o["argmax"]) == (3.0, 4)
    assert o["n_within"].tolist() == [1, 2, 3] and o["n_angle"].tolist() == [3, 2, 2]  # both rules are inclusive
    assert o["sum_e"] == 6.6 and o["sum_c"] == 2.8
    assert math.isclose(o["sum_e2_within"][2], 1.0 + 0.36 + 4.0, rel_tol=1e-15)
    # the gate, both modes (d2 of the pairs: 1, 1, 0.25, 4, 25)
    assert R.surface_error(q_xyz, r_xyz, idx, d2, r_nrm, None, gate=4.0, gate_mode=0)[2]["n_used"] == 3
    assert R.surface_error(q_xyz, r_xyz, idx, d2, r_nrm, None, gate=2.0, gate_mode=1)[2]["n_used"] == 2
    none = R.surface_error(q_xyz, r_xyz, idx, d2, r_nrm, None, gate=0.5, gate_mode=1)[2]
    assert (none["n_used"], none["max_e"], none["argmax"], none["sum_e"]) == (0, 0.0, -1, 0.0)
    # ties of max_e go to the smallest index
    tie = R.surface_error(q_xyz[[4, 4, 0]], r_xyz, idx[[4, 4, 0]], d2[[4, 4, 0]], r_nrm)[2]
    assert (tie["max_e"], tie["argmax"]) == (3.0, 0)


def test_rayleigh_bound_on_perturbed_matrices():
    """n = the exact minimiser of C + E with |E|_2 <= B: n^T C n <= l3(C) + 2 B, gap or no gap (the GPU test allows 4 B)"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for trial in range(2000):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        lam = np.sort(rng.uniform(0, 1, 3))
        if trial % 3 == 0:
            lam[1] = lam[0] + rng.uniform(0, 1e-9)  # near-degenerate smallest pair
        if trial % 7 == 0:
            lam[1] = lam[0]
        cm = (q * lam) @ q.T
        cm = (cm + cm.T) / 2
        bnd = 10.0 ** rng.uniform(-12, -2)
        e = rng.standard_normal((3, 3))
        e = (e + e.T) / 2
        e *= bnd / np.linalg.norm(e, 2)
        w, v = np.linalg.eigh(cm + e)
        n = v[:, 0]
        l3 = np.linalg.eigvalsh(cm)[0]
        excess = float(n @ cm @ n) - l3
        worst = max(worst, excess / bnd)
        assert excess <= 2 * bnd * (1 + 1e-9) + 1e-15
    assert worst > 0.1  # the perturbations were felt


def test_struct_sizes_follow_the_header():
    assert C.sizeof(_lib.RadiusNormalsOut) == 3 * 8
    assert C.sizeof(_lib.SurfaceParams) == 8 + 4 + 4 + 8 * 8 + 4 + 4 + 8 * 8
    assert C.sizeof(_lib.SurfaceOut) == 8 * (3 + 5 + 1 + 8 + 8 + 8)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mapeval_hip.h")).read()
    assert re.search(r"#define\s+ME_SURFACE_MAX_ANGLES\s+8\b", hdr) and _lib.ME_SURFACE_MAX_ANGLES == 8
    # the field order of the header's structs is the field order of the ctypes classes
    for cname, cls in (("me_radius_normals_out", _lib.RadiusNormalsOut), ("me_surface_params", _lib.SurfaceParams), ("me_surface_out", _lib.SurfaceOut)):
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.sub(r"\[.*", "", tok.strip()) for decl in body.split(";") if decl.strip()
                 for tok in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f for f, _ in cls._fields_], cname
    for sym in ("me_radius_normals", "me_nn_surface_error", "me_nn_surface_fetch"):
        assert sym in _lib.SYMBOLS and re.search(r"\bint " + sym + r"\(", hdr)
