"""The numpy expectation of me_voxel_metrics (include/mapeval_hip.h): per-point products grouped by the voxel lattice of
getVoxelIndex (floor(p / voxel_size), voxel_calculator.cpp:241-245) with the per-point predicate of the AC / COM / CD sums
(map_eval.cpp:1069-1145, 1416) and the valid entropies of MME (:1692-1697)."""
import math

import numpy as np

GATE_LE_UNSQUARED, GATE_LT_SQUARED = 0, 1


def t2max(t: float) -> float:
    """Largest d2 whose correctly rounded square root is <= t (the library compares d2 against it)."""
    if not t >= 0:
        return -1.0
    x = t * t
    while math.sqrt(np.nextafter(x, np.inf)) <= t:
        x = float(np.nextafter(x, np.inf))
    while x > 0 and math.sqrt(x) > t:
        x = float(np.nextafter(x, -np.inf))
    return float(x)


def gate_mask(d2, gate: float, gate_mode: int):
    if gate < 0:
        return np.ones(d2.shape, bool)
    return d2 < gate * gate if gate_mode == GATE_LT_SQUARED else d2 <= gate


def group(xyz, d2, voxel_size: float, gate: float, gate_mode: int, trunc, ent=None, valid=None) -> dict:
    """-> dict in the layout of Engine.voxel_metrics, plus abs_H (the summed |entropy| of a voxel: the scale of sum_H)."""
    xyz = np.asarray(xyz, np.float64)
    d2 = np.asarray(d2, np.float64)
    k3 = np.floor(xyz / voxel_size).astype(np.int64) + (1 << 20)  # (|index| < 2^20, as the library requires)
    packed, inv = np.unique((k3[:, 0] << 42) | (k3[:, 1] << 21) | k3[:, 2], return_inverse=True)  # ascending (ix, iy, iz)
    inv = np.asarray(inv).reshape(-1)
    keys = np.stack([(packed >> 42) & 0x1fffff, (packed >> 21) & 0x1fffff, packed & 0x1fffff], axis=1) - (1 << 20)
    V = keys.shape[0]

    def cnt(m):
        return np.bincount(inv[m], minlength=V).astype(np.int64)

    def tot(w, m):
        return np.bincount(inv[m], weights=w[m], minlength=V)

    d = np.sqrt(d2)
    g = gate_mask(d2, gate, gate_mode)
    inl = [g & (d2 <= t2max(float(t))) for t in trunc]
    out = dict(keys=keys.astype(np.int32), n_query=cnt(np.ones(len(d2), bool)), n_corr=cnt(g),
               n_inl=np.stack([cnt(m) for m in inl], axis=1), sum_d=np.stack([tot(d, m) for m in inl], axis=1),
               sum_d2=np.stack([tot(d2, m) for m in inl], axis=1), sum_sqrt_all=tot(d, np.ones(len(d2), bool)))
    if ent is None:
        out.update(n_H=np.zeros(V, np.int64), sum_H=np.zeros(V), abs_H=np.zeros(V))
    else:
        v = np.asarray(valid).astype(bool)
        ent = np.asarray(ent, np.float64)
        out.update(n_H=cnt(v), sum_H=tot(ent, v), abs_H=tot(np.abs(ent), v))
    return out


def brute_force(xyz, d2, voxel_size: float, gate: float, gate_mode: int, trunc, ent=None, valid=None) -> dict:
    """The same table with a plain loop over the points (what group() is checked against)."""
    rows = {}
    t2 = [t2max(float(t)) for t in trunc]
    for i in range(len(d2)):
        k = tuple(math.floor(float(xyz[i][a]) / voxel_size) for a in range(3))
        r = rows.setdefault(k, dict(n_query=0, n_corr=0, n_inl=[0] * 5, sum_d=[0.0] * 5, sum_d2=[0.0] * 5, sum_sqrt_all=0.0,
                                    n_H=0, sum_H=0.0))
        q = float(d2[i])
        r["n_query"] += 1
        r["sum_sqrt_all"] += math.sqrt(q)
        passed = True if gate < 0 else (q < gate * gate if gate_mode == GATE_LT_SQUARED else q <= gate)
        if passed:
            r["n_corr"] += 1
            for k5 in range(5):
                if q <= t2[k5]:
                    r["n_inl"][k5] += 1
                    r["sum_d"][k5] += math.sqrt(q)
                    r["sum_d2"][k5] += q
        if ent is not None and valid[i]:
            r["n_H"] += 1
            r["sum_H"] += float(ent[i])
    keys = sorted(rows)
    out = dict(keys=np.array(keys, np.int32).reshape(-1, 3))
    for f in ("n_query", "n_corr", "n_H"):
        out[f] = np.array([rows[k][f] for k in keys], np.int64)
    out["n_inl"] = np.array([rows[k]["n_inl"] for k in keys], np.int64).reshape(-1, 5)
    for f in ("sum_d", "sum_d2"):
        out[f] = np.array([rows[k][f] for k in keys], np.float64).reshape(-1, 5)
    for f in ("sum_sqrt_all", "sum_H"):
        out[f] = np.array([rows[k][f] for k in keys], np.float64)
    return out


INT_FIELDS = ("n_query", "n_corr", "n_inl", "n_H")
FLOAT_FIELDS = ("sum_d", "sum_d2", "sum_sqrt_all")


def assert_rows_equal(got: dict, want: dict, rtol: float = 1e-12):
    """Keys and counts exact, sums to rtol of their scale (sum_H: of the voxel's summed |entropy|)."""
    np.testing.assert_array_equal(got["keys"], want["keys"])
    for f in INT_FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    for f in FLOAT_FIELDS:
        np.testing.assert_allclose(got[f], want[f], rtol=rtol, atol=0, err_msg=f)
    scale = want.get("abs_H", np.abs(want["sum_H"]))
    assert np.all(np.abs(got["sum_H"] - want["sum_H"]) <= rtol * scale), "sum_H"
