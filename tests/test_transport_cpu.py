"""me_voxel_transport without a GPU: the entry points are declared, exported and bound; the numpy model (tests/_transport_ref.py) against
the exact optimal transport of an equal-size pair (scipy.optimize.linear_sum_assignment) on the doubled-wall voxel:
    sw2_sq <= max_sw2_sq <= W2^2_exact                 (by definition; projection on a unit vector is 1-Lipschitz)
    W2^2_exact <= OT_eps <= W2^2_exact + eps ln n      (OT_eps is the minimum of cost plus a non-negative KL term; the permutation
                                                        plan has KL = ln n)
    S_eps >= 0 and S_eps(X, X) = 0
each within slack = marginal_err max C + 1e-12.  n = m = 64 in a 1 m voxel, blur 0.2, 400 plain iterations."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _transport_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_and_bound():
    from cloud_map_evaluation_amd import _lib, synth
    from cloud_map_evaluation_amd.engine import Engine, TRANSPORT_N_FINAL, transport_schedule

    hdr = open(os.path.join(ROOT, "include", "mapeval_hip.h")).read()
    assert "int me_voxel_transport(me_ctx *ctx, const me_voxtrans_params *p, const double *directions" in hdr
    assert "me_voxel_transport" in _lib.SYMBOLS
    L = _lib.load()
    assert L.me_voxel_transport.restype is ctypes.c_int and len(L.me_voxel_transport.argtypes) == 13
    assert ctypes.sizeof(_lib.VoxTransParams) == 8 + 4 * 4 + 8 and ctypes.sizeof(_lib.VoxTransOut) == 12 * 8
    code = Engine.voxel_transport.__code__
    assert code.co_varnames[:code.co_argcount] == ("self", "voxel_size", "blur", "directions", "min_pts", "max_points", "scaling", "n_final",
                                                   "eps_schedule", "fetch")
    assert Engine.voxel_transport.__defaults__ == (None, 32, 100, 512, 0.5, TRANSPORT_N_FINAL, None, True)
    assert TRANSPORT_N_FINAL in (8, 16, 32, 64, 128)
    eps = transport_schedule(1.0, 0.2)
    assert np.array_equal(eps, T.schedule(1.0, 0.2, 0.5, TRANSPORT_N_FINAL))
    assert eps[0] == 3.0 and eps[-1] == 0.2 * 0.2 and (np.diff(eps) <= 0).all() and (eps[1:4] == 3.0 * 0.25 ** np.arange(1, 4)).all()
    assert (eps == eps[-1]).sum() == TRANSPORT_N_FINAL + 1
    for n in (1, 32, 64):
        d = synth.fibonacci_directions(n)
        assert d.shape == (n, 3) and (d[:, 2] > 0).all()
        assert np.abs(np.sqrt((d * d).sum(1)) - 1.0).max() <= 2.0 ** -52
    for bad in (0, 65):
        with pytest.raises(ValueError):
            synth.fibonacci_directions(bad)


def test_model_helpers():
    rng = np.random.default_rng(1)
    v = rng.random(256)
    assert abs(T.block_sum(v) - math.fsum(v)) <= 256 * 2.0 ** -53 * math.fsum(v)
    x = rng.random(700)
    assert abs(T.lane_sum(x) - math.fsum(x)) <= 700 * 2.0 ** -53 * math.fsum(x)
    for n, m in ((11, 63), (64, 64), (257, 255), (5, 1)):
        i, j, w = T.overlaps(n, m)
        assert w.sum() == n * m and (w > 0).all()
        assert np.array_equal(np.bincount(i, w), np.full(n, m)) and np.array_equal(np.bincount(j, w), np.full(m, n))
    # equal sizes: the sorted values pair off one to one
    X, Y = rng.random((40, 3)), rng.random((40, 3))
    u = np.array([0.0, 0.6, 0.8])
    exact, ordered, a, b = T.sliced_dir(X, Y, u)
    assert abs(exact - np.mean((a - b) ** 2)) <= 1e-15 and abs(ordered - exact) <= 96 * 2.0 ** -53 * exact


def test_overlap_count():
    """n + m - gcd(n, m) pairs overlap (n + m - 1 for coprime sizes); the kernel and the model walk exactly those"""
    for n, m in ((11, 63), (64, 65), (64, 64), (12, 18)):
        i, _, _ = T.overlaps(n, m)
        assert len(i) == n + m - math.gcd(n, m)


@pytest.fixture(scope="module")
def W():
    from scipy.optimize import linear_sum_assignment

    n = 64
    X, Y = T.doubled_wall(n, n, 1.0, 0.05, 0)
    C = T.cost(X, Y)
    r, c = linear_sum_assignment(C)
    w2_exact = C[r, c].sum() / n
    from cloud_map_evaluation_amd import synth

    eps = np.full(400, 0.2 * 0.2)
    return dict(X=X, Y=Y, n=n, w2_exact=w2_exact, eps=eps, sl=T.sliced_row(X, Y, synth.fibonacci_directions(32)),
                sk=T.sinkhorn_row(X, Y, eps), same=T.sinkhorn_row(X, X, eps))


def test_the_doubled_wall_is_invisible_to_the_mean_and_visible_to_both_distances(W):
    X, Y = W["X"], W["Y"]
    assert abs(X[:, 0].mean() - Y[:, 0].mean()) <= 1e-15  # the centroid across the wall does not move
    assert W["sl"]["by_exact"]["max_sw2_sq"] > 0.5 * 0.05 ** 2 and W["sk"]["sinkhorn"] > 0.0


def test_sliced_is_below_the_exact_w2(W):
    s = W["sl"]["by_exact"]
    print(f"sw2_sq {s['sw2_sq']:.6g} <= max_sw2_sq {s['max_sw2_sq']:.6g} <= W2^2 exact {W['w2_exact']:.6g}")
    assert s["sw2_sq"] <= s["max_sw2_sq"] * (1 + 1e-15) and s["max_sw2_sq"] <= W["w2_exact"] + 1e-12
    o = W["sl"]["by_order"]
    assert o["max_dir"] == s["max_dir"] and abs(o["sw2_sq"] - s["sw2_sq"]) <= 160 * 2.0 ** -53 * s["sw2_sq"]


def test_entropic_ot_sandwich_and_debiasing(W):
    sk, n, eps = W["sk"], W["n"], W["eps"][-1]
    slack = sk["marginal_err"] * sk["max_cost"] + 1e-12
    print(f"W2^2 exact {W['w2_exact']:.6g} <= OT_eps {sk['ot_xy']:.6g} <= {W['w2_exact'] + eps * math.log(n):.6g}; marginal_err "
          f"{sk['marginal_err']:.3g}; S {sk['s']:.6g}; S(X, X) {W['same']['s']:.3g}")
    assert sk["marginal_err"] < 1e-12  # 400 iterations have converged
    assert W["w2_exact"] <= sk["ot_xy"] + slack
    assert sk["ot_xy"] <= W["w2_exact"] + eps * math.log(n) + slack
    assert sk["s"] >= -slack
    same = W["same"]
    assert abs(same["s"]) <= same["marginal_err"] * same["max_cost"] + 1e-12


def test_float64_model_against_its_long_double_twin(W):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is double here")
    hi = T.sinkhorn_row(W["X"], W["Y"], W["eps"][:40], np.longdouble)
    lo = T.sinkhorn_row(W["X"], W["Y"], W["eps"][:40])
    assert np.abs(lo["f"] - hi["f"]).max() <= 1e-12 * np.abs(hi["f"]).max()
    assert abs(lo["s"] - hi["s"]) <= 1e-12 * float(hi["s_abs"])


def _parse(tmp_path, extra):
    import subprocess

    from test_mesh_host_cpu import _BASE

    cfg = tmp_path / "c.yaml"
    cfg.write_text(_BASE + extra)
    exe = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")
    return subprocess.run([exe, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=60)


def test_host_keys(tmp_path):
    import json

    new = ("evaluate_voxel_transport", "transport_blur", "transport_directions", "transport_max_points", "transport_scaling")
    r = _parse(tmp_path, "")
    assert r.returncode == 0, r.stderr
    base = json.loads(r.stdout)
    assert tuple(base[k] for k in new) == (False, base["nn_radius"], 32, 512, 0.5)
    r = _parse(tmp_path, "evaluate_voxel_transport: true\ntransport_blur: 0.25\ntransport_directions: 0\ntransport_max_points: 1024\ntransport_scaling: 0.7\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert tuple(p[k] for k in new) == (True, 0.25, 0, 1024, 0.7)
    assert {k: v for k, v in p.items() if k not in new} == {k: v for k, v in base.items() if k not in new}  # nothing else moves
    for bad in ("transport_blur: 0\n", "transport_blur: -0.1\n", "transport_directions: 65\n", "transport_directions: -1\n", "transport_max_points: 10\n",
                "transport_max_points: 1025\n", "transport_scaling: 0\n", "transport_scaling: 1\n", "num_gpus: 2\n"):
        assert _parse(tmp_path, "evaluate_voxel_transport: true\n" + bad).returncode != 0, bad
        assert _parse(tmp_path, "evaluate_voxel_transport: false\n" + bad).returncode == 0 or bad == "num_gpus: 2\n", bad
