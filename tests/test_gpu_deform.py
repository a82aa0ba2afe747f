"""me_voxel_deformation on the GPU: accuracy of the residuals formed from moments, a known rigid motion, determinism and lifetimes,
argument errors.  The checks every case shares are in tests/_deform_checks.py, the model in tests/_deform_ref.py."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _deform_checks as dc  # noqa: E402
import _deform_ref as ref  # noqa: E402
from _globreg_ref import rotation  # noqa: E402

pytestmark = pytest.mark.gpu
EST, GT = dc.EST, dc.GT


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _drifting_pair(n, seed, box=2.0, noise=0.004):
    """est = gt under a drift that differs from voxel to voxel (a slow rotation about a far axis) + noise, then shuffled."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(-box / 2, box / 2, (n, 3))
    est = gt @ rotation(math.radians(0.15), math.radians(-0.1)).T + [0.004, -0.003, 0.002] + noise * rng.standard_normal((n, 3))
    return est[rng.permutation(n)], gt


@pytest.mark.parametrize("vs,max_d", [(1.0, 0.1), (0.5, math.inf), (0.3, 0.02)])
def test_residuals_against_the_sums_over_the_points(eng, vs, max_d):
    """e_t and e_R (moments; the cancellation of sum d2 - n |t0|^2) against the residuals summed pair by pair, within
    64 n 2^-53 (1.5 vs + max_distance)^2.  Largest ratio to that bound observed on an MI355X: see DESIGN.md 4.22."""
    est, gt = _drifting_pair(20_000, 1)
    got, m, idx, d2 = dc.run(eng, est, gt, vs, max_d, cell_size=0.1)
    md = max_d if math.isfinite(max_d) else math.sqrt(d2.max())  # (every pair is within the largest distance there is)
    o = got["keys"].astype(np.float64) * vs + 0.5 * vs
    worst = 0.0
    assert got["n_fit"] > 0 and got["n_rot"] > 0
    for v in range(got["n_voxels"]):
        n = int(got["n_pairs"][v])
        if n == 0:
            continue
        rows = np.flatnonzero((m["point_voxel"] == v) & m["pair"])
        a, b = est[rows] - o[v], m["q"][rows] - o[v]
        dt, dR = ref.direct_residuals(a, b, got["R"][v])
        bound = 64 * n * 2.0 ** -53 * (1.5 * vs + md) ** 2
        worst = max(worst, abs(got["e_t"][v] - dt) / bound, abs(got["e_R"][v] - dR) / bound)
    print(f"deformation residuals vs={vs} max_d={max_d}: largest |moments - direct| / bound = {worst:.3g}")
    assert worst <= 1.0
    assert 0.0 < got["share_translation"] < 1.0 and 0.0 < got["share_rigid"] < 1.0


def _known_motion(noise: float):
    """One voxel of 200 jittered lattice points (spacing 5 cm, jitter 1 cm: every spacing >= 3 cm, far above the motion) as the query;
    the reference is the same points moved by R0 about the voxel centre and t0 (|t0| = 1 mm): the fit a -> b is (R0, t0) itself."""
    rng = np.random.default_rng(7)
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3)[:200]
    pts = 0.3 + 0.05 * g + rng.uniform(-0.01, 0.01, (200, 3))
    R0 = rotation(math.radians(0.2))
    t0 = np.array([0.0006, -0.0006, 0.00052915026221291817])
    moved = (pts - 0.5) @ R0.T + 0.5 + t0 + noise * rng.standard_normal((200, 3))
    return pts, moved, R0, t0


def test_known_rigid_motion(eng):
    pts, moved, R0, t0 = _known_motion(0.0)
    got, m, idx, d2 = dc.run(eng, pts, moved, 1.0, 0.05)
    assert np.array_equal(idx, np.arange(200)), "every pair must be its own point"
    assert got["n_voxels"] == 1 and got["n_pairs"][0] == 200 and got["flags"][0] == ref.FIT | ref.ROT_OK
    assert np.abs(got["R"][0] - R0).max() <= 1e-9
    assert np.abs(got["u"][0] - t0).max() <= 1e-9  # the fit's displacement at the voxel centre
    assert abs(got["angle"][0] - math.radians(0.2)) <= 1e-9
    assert got["share_rigid"] >= 1.0 - 1e-9
    assert 0.0 < got["share_translation"] < 1.0


def test_known_motion_with_noise_is_partly_drift(eng):
    pts, moved, R0, t0 = _known_motion(0.001)
    got, m, idx, d2 = dc.run(eng, pts, moved, 1.0, 0.05)
    assert np.array_equal(idx, np.arange(200))
    assert 0.0 < got["share_rigid"] < 1.0 and 0.0 < got["share_translation"] < got["share_rigid"]


def _bytes(d):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else (dc.bits(v)[0] if isinstance(v, float) else v)) for k, v in d.items()}


def test_determinism_and_lifetimes(eng):
    """Identical bytes over two calls and after a re-sort that does not change the points (the index rebuilt on another cell size:
    another sorted order): the sums are added in the points' own order, by voxel and original index."""
    from cloud_map_evaluation_amd.engine import MapEvalError

    est, gt = _drifting_pair(30_000, 3)
    got, _, idx, _ = dc.run(eng, est, gt, 0.5, 0.1, cell_size=0.1)
    first = _bytes(got)
    assert _bytes(eng.deformation_field(EST, 0.5, 0.1)) == first                      # two calls
    assert _bytes(eng.deformation_fetch(EST)) == {k: first[k] for k in eng.deformation_fetch(EST)}
    eng.upload(EST, est, cell_size=0.3)                                              # the same points in another sorted order
    eng.upload(GT, gt, cell_size=0.3)
    with pytest.raises(MapEvalError, match=r"^\[-3\]"):
        eng.deformation_fetch(EST)
    eng.nn1(EST, GT, fetch=False)
    assert np.array_equal(eng.nn_fetch(EST)[0], idx)  # (the same pairs: no tie between two neighbours was broken the other way)
    assert _bytes(eng.deformation_field(EST, 0.5, 0.1)) == first
    eng.nn1(EST, GT, fetch=False)                                                    # a new search discards the rows
    with pytest.raises(MapEvalError, match=r"^\[-3\]"):
        eng.deformation_fetch(EST)
    T = np.eye(4)
    T[0, 3] = 0.001
    for disturb in (lambda: eng.transform_cloud(EST, T), lambda: eng.transform_cloud(GT, T),
                    lambda: eng.upload(EST, est, cell_size=0.1), lambda: eng.upload(GT, gt, cell_size=0.1)):
        eng.nn1(EST, GT, fetch=False)
        eng.deformation_field(EST, 0.5, 0.1, fetch=False)
        disturb()
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            eng.deformation_field(EST, 0.5, 0.1)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            eng.deformation_fetch(EST)


def test_argument_and_state_errors():
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import Engine, MapEvalError

    rng = np.random.default_rng(5)
    est, gt = rng.uniform(-3, 3, (5000, 3)), rng.uniform(-3, 3, (5000, 3))
    nan = float("nan")
    with Engine(0) as e:
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):  # not uploaded
            e.deformation_field(EST, 1.0, 0.5)
        e.upload(EST, est, cell_size=0.5)
        e.upload(GT, gt, cell_size=0.5)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):  # no me_nn1 with this slot as the query
            e.deformation_field(EST, 1.0, 0.5)
        e.nn1(EST, GT, fetch=False)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e.deformation_field(GT, 1.0, 0.5)
        for kw in (dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=nan),
                   dict(min_pairs=2), dict(min_spread=-0.1), dict(min_spread=nan), dict(voxel_size=1e-6)):  # (1e-6: keys outside 2^20)
            a = dict(voxel_size=1.0, max_distance=0.5, min_pairs=30, min_spread=0.05)
            a.update(kw)
            with pytest.raises(MapEvalError, match=r"^\[-1\]"):
                e.deformation_field(EST, a["voxel_size"], a["max_distance"], a["min_pairs"], a["min_spread"])
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):  # (a failed call leaves no rows)
            e.deformation_fetch(EST)
        V = e.deformation_field(EST, 1.0, 0.5, min_pairs=3)["n_voxels"]
        assert V == 216
        keys = np.empty((V, 3), np.int32)
        nv = C.c_int64(V - 1)
        rc = _lib.load().me_voxel_deformation_fetch(e._ctx, EST, keys.ctypes.data, 0, 0, 0, 0, 0, 0, 0, C.byref(nv))
        assert rc == _lib.ME_ERR_CAPACITY and nv.value == V
    with Engine(0) as e:
        e.set_slab(0, -1.0, 1.0, 0.5)
        e.upload(EST, est, cell_size=0.5)
        e.upload(GT, gt, cell_size=0.5)
        e.nn1(EST, GT, fetch=False)
        with pytest.raises(MapEvalError, match=r"^\[-3\].*slab"):
            e.deformation_field(EST, 1.0, 0.5)
    with Engine(0) as e:
        e.upload(EST, est, cell_size=0.5)
        e.upload(GT, gt, cell_size=0.5)
        e.nn1(EST, GT, fetch=False)
        e.set_shard(0, 2)
        with pytest.raises(MapEvalError, match=r"^\[-3\].*shard"):
            e.deformation_field(EST, 1.0, 0.5)
