"""What every GPU case of me_voxel_deformation is held to (tests/test_gpu_deform.py, tests/test_gpu_deform_edges.py): run() uploads a
pair, searches, calls Engine.deformation_field and checks the result against tests/_deform_ref.py."""
from __future__ import annotations

import numpy as np

import _deform_ref as ref

EST, GT = 0, 1
U = 2.0 ** -53
FLOATS = ("sums", "t0", "u", "R", "e0", "e_t", "e_R")


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def check(eng, est, gt, idx, d2, got, vs, max_d, min_pairs, min_spread, searched=True) -> dict:
    """The common checks on `got` = deformation_field(EST, ..) for the resident pair; idx / d2 = nn_fetch(EST).  -> the model's sums."""
    ms = vs / 20.0 if min_spread is None else min_spread
    V = got["n_voxels"]
    # keys and row order equal me_voxel_gaussians
    vk = eng.voxel_gaussians(EST, vs)
    assert np.array_equal(got["keys"], vk[0]) and V == len(vk[0])
    # n_pairs exact, the 23 sums within the summation bound of the voxel's point count
    pair = ref.pair_mask(d2, idx, len(gt), max_d)
    q = gt[np.clip(idx, 0, len(gt) - 1)]
    m = ref.voxel_sums(est, q, d2, pair, vs)
    assert np.array_equal(m["keys"], got["keys"]) and np.array_equal(m["n_points"], vk[1])
    assert np.array_equal(m["n_pairs"], got["n_pairs"])
    if searched:
        assert int(got["n_pairs"].sum()) == eng.icp_p2p_sums(EST, max_d).n_corr
    bound = m["n_points"][:, None] * U * m["scale"]
    err = np.abs(got["sums"] - m["sums"])
    assert (err <= bound).all(), f"sums off by up to {np.max(err / np.maximum(bound, 1e-300)):.3g} of the summation bound"
    # the fit: bit-identical to the model fed the device's own sums; flags exact
    f = ref.fit_rows(got["n_pairs"], got["sums"], min_pairs, ms)
    assert np.array_equal(f["flags"], got["flags"])
    for k in ("t0", "u", "R", "e0", "e_t", "e_R"):
        assert np.array_equal(bits(f[k]), bits(got[k])), k
    # the totals: the same fixed-order reduction of the fetched rows
    t = ref.totals(got["n_pairs"], got["flags"], got["t0"], got["e0"], got["e_t"], got["e_R"])
    for k in ("n_voxels", "n_with_pairs", "n_fit", "n_rot", "max_row"):
        assert t[k] == got[k], k
    assert t["n_pairs"] == got["n_pairs_total"]
    for k in ("sum_n_t0", "sum_n_t0sq", "sum_e0", "sum_e_t", "sum_e0_fit", "sum_e_R"):
        assert bits(t[k])[0] == bits(got[k])[0], (k, t[k], got[k])
    assert bits(t["max_disp"])[0] == bits(got["max_disp"])[0]
    assert got["max_key"] == (tuple(int(x) for x in got["keys"][t["max_row"]]) if t["max_row"] >= 0 else None)
    m["pair"], m["q"] = pair, q
    return m


def run(eng, est, gt, vs, max_d, min_pairs=30, min_spread=None, cell_size=0.0):
    """-> (got, model, idx, d2)"""
    est, gt = np.ascontiguousarray(est, np.float64), np.ascontiguousarray(gt, np.float64)
    eng.upload(EST, est, cell_size=cell_size)
    eng.upload(GT, gt, cell_size=cell_size)
    eng.nn1(EST, GT, fetch=False)
    idx, d2 = eng.nn_fetch(EST)
    got = eng.deformation_field(EST, vs, max_d, min_pairs=min_pairs, min_spread=min_spread)
    return got, check(eng, est, gt, idx, d2, got, vs, max_d, min_pairs, min_spread), idx, d2
