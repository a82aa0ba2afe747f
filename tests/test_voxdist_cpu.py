"""me_voxel_distances without a GPU: the entry points are declared, exported and bound; the numpy model's Gaussian row
(tests/_voxdist_ref.py, the restatement of k_vd_gauss) against a formula-level numpy evaluation; the model's MMD properties and the
stride rule; the host's configuration keys."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import _voxdist_ref as ref  # noqa: E402
from test_mesh_host_cpu import _BASE  # noqa: E402

EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
U = 2.0 ** -53


def test_entry_points_are_declared_exported_and_bound():
    """fails on a tree without the feature"""
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import Engine

    hdr = open(os.path.join(ROOT, "include", "mapeval_hip.h")).read()
    assert "int me_voxel_distances(me_ctx *ctx, const me_voxdist_params *p, int32_t *keys /*V x 3*/, int32_t *n_pop /*V x 2*/, int32_t *n_used /*V x 2*/," in hdr
    assert "me_voxel_distances" in _lib.SYMBOLS
    L = _lib.load()
    assert L.me_voxel_distances.restype is ctypes.c_int and len(L.me_voxel_distances.argtypes) == 10
    # the struct sizes follow from the header's member lists
    sizes = {"double": 8, "int32_t": 4, "int64_t": 8}
    for name, struct in (("me_voxdist_params", _lib.VoxDistParams), ("me_voxdist_out", _lib.VoxDistOut)):
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
        total, fields = 0, []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            ty, rest = decl.split(None, 1)
            for member in rest.split(","):
                m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", member)
                total += sizes[ty] * int(m.group(2) or 1)
                fields.append(m.group(1))
        assert ctypes.sizeof(struct) == total and [f for f, _ in struct._fields_] == fields, name
    assert ctypes.sizeof(_lib.VoxDistParams) == 64 and ctypes.sizeof(_lib.VoxDistOut) == 120
    assert callable(getattr(Engine, "voxel_distances", None))
    names = Engine.voxel_distances.__code__.co_varnames[:Engine.voxel_distances.__code__.co_argcount]
    assert names == ("self", "voxel_size", "sigmas", "min_pts", "max_points", "eig_floor", "fetch")
    assert Engine.voxel_distances.__defaults__ == (100, 2048, 1e-6, True)


def _spd(rng, cond=1e3):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    lam = 10.0 ** rng.uniform(-2.0, 1.0, 3)
    lam = np.maximum(lam, lam.max() / cond)
    return (Q * lam) @ Q.T


def test_model_gaussian_row_against_numpy_linear_algebra():
    """200 random SPD pairs with condition number <= 1e3 (no eigenvalue near the floor): 1e-9 relative, the project's bar"""
    rng = np.random.default_rng(11)
    for _ in range(200):
        Ce, Cg = _spd(rng), _spd(rng)
        mu_e, mu_g = rng.normal(size=3), rng.normal(size=3)
        ne, ng = int(rng.integers(11, 500)), int(rng.integers(11, 500))
        got = ref.gauss_row(ne, mu_e, Ce / (ne - 1), ng, mu_g, Cg / (ng - 1), 1e-6)["values"]
        want = ref.gauss_formula(mu_e, Ce, mu_g, Cg)
        for a, b in zip(got, want):
            assert abs(a - b) <= 1e-9 * abs(b)


def test_equal_gaussians_give_zero_in_all_four_columns():
    rng = np.random.default_rng(12)
    for _ in range(20):
        Cm, mu = _spd(rng), rng.normal(size=3)
        got = ref.gauss_row(60, mu, Cm / 59, 60, mu, Cm / 59, 1e-6)
        tr = np.trace(Cm)
        assert all(abs(v) <= 1e-12 * tr for v in got["values"][:3])
        assert abs(got["D"]) <= 1e-12 * tr  # (W2 itself is the square root of this residue)
    # swapping the roles swaps the two KL columns and keeps the symmetric ones
    Ce, Cg, me_, mg = _spd(rng), _spd(rng), rng.normal(size=3), rng.normal(size=3)
    a = ref.gauss_row(40, me_, Ce / 39, 70, mg, Cg / 69)["values"]
    b = ref.gauss_row(70, mg, Cg / 69, 40, me_, Ce / 39)["values"]
    assert (a[0], a[1]) == (b[1], b[0]) and a[2] == b[2] and abs(a[3] - b[3]) <= 1e-12


def test_model_mmd_properties():
    rng = np.random.default_rng(13)
    X, Y = rng.random((40, 3)), 0.2 + rng.random((57, 3))
    for sigma in (0.05, 0.3, 2.0):
        m = ref.mmd_row(X, Y, sigma)
        tol = (max(m["terms"]) + 16) * U * m["b_abs"]
        assert m["b"] >= -tol and m["u"] <= m["b"]
        s = ref.mmd_row(Y, X, sigma)  # swapping the clouds swaps Sxx / Syy
        assert (s["ksum"][0], s["ksum"][1], s["ksum"][2]) == (m["ksum"][1], m["ksum"][0], m["ksum"][2])
        assert abs(s["b"] - m["b"]) <= tol and abs(s["u"] - m["u"]) <= tol
        same = ref.mmd_row(X, X[rng.permutation(40)], sigma)  # X = Y as the same multiset
        assert abs(same["b"]) <= (max(same["terms"]) + 16) * U * same["b_abs"]
    far = ref.mmd_row(X[:12], 100.0 + X[:12], 0.05)  # disjoint supports: the cross term underflows, mmd2_b = 1/n + 1/m + 2 Sxx / n^2 + ...
    assert far["ksum"][2] == 0.0 and far["b"] > 0.0


def test_stride_rule_and_rows():
    mp = 64
    assert ref.stride_rule(mp, mp) == (1, 64) and ref.stride_rule(mp + 1, mp) == (2, 33) and ref.stride_rule(2 * mp + 1, mp) == (3, 43)
    assert ref.stride_rule(10 ** 6, 0) == (1, 10 ** 6) and ref.stride_rule(2 * mp, mp) == (2, 64)
    for n in range(12, 400):
        for m in (11, 12, 64):
            s, used = ref.stride_rule(n, m)
            assert 6 <= used <= max(m, n if n <= m else 0) and used == len(range(0, n, s))
    est, gt, keys = ref.scene()
    rows = ref.rows(est, gt, ref.VS, ref.MIN_PTS, 0)
    assert [r[0] for r in rows] == keys and len(keys) == 8
    assert all(a == sorted(a) and b == sorted(b) for _, a, b, _, _ in rows)  # ascending original index
    sub = ref.rows(est, gt, ref.VS, ref.MIN_PTS, 64)
    assert [(r[3], r[4]) for r in sub] == [(r[3], r[4]) for r in rows]  # the gate looks at the full population
    assert all(set(sa) <= set(a) and sa[0] == a[0] for (_, sa, _, _, _), (_, a, _, _, _) in zip(sub, rows))


def _parse(tmp_path, extra):
    cfg = tmp_path / "c.yaml"
    cfg.write_text(_BASE + extra)
    return subprocess.run([EXE, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)


NEW = ("evaluate_voxel_distances", "mmd_sigmas", "mmd_max_points", "voxel_distance_eig_floor")


def test_host_keys(tmp_path):
    r = _parse(tmp_path, "")
    assert r.returncode == 0, r.stderr
    base = json.loads(r.stdout)
    assert (base["evaluate_voxel_distances"], base["mmd_sigmas"], base["mmd_max_points"], base["voxel_distance_eig_floor"]) == \
        (False, [base["nn_radius"]], 2048, 1e-6)
    r = _parse(tmp_path, "evaluate_voxel_distances: true\nmmd_sigmas: [0.1, 0.4, 1.6]\nmmd_max_points: 512\nvoxel_distance_eig_floor: 1e-5\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["evaluate_voxel_distances"], p["mmd_sigmas"], p["mmd_max_points"], p["voxel_distance_eig_floor"]) == (True, [0.1, 0.4, 1.6], 512, 1e-5)
    assert {k: v for k, v in p.items() if k not in NEW} == {k: v for k, v in base.items() if k not in NEW}  # nothing else moves
    for bad in ("mmd_sigmas: [0.1, 0.2, 0.3, 0.4, 0.5]\n", "mmd_sigmas: []\n", "mmd_sigmas: [0.0]\n", "mmd_sigmas: 0.3\n", "mmd_max_points: 5\n",
                "mmd_max_points: -1\n", "voxel_distance_eig_floor: 0\n", "num_gpus: 2\n"):
        assert _parse(tmp_path, "evaluate_voxel_distances: true\n" + bad).returncode != 0, bad
