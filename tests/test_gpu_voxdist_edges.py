"""me_voxel_distances at its edges on the MI355X, against the numpy model of tests/_voxdist_ref.py, on clouds built voxel by voxel.

The scene (_voxdist_ref.scene): 13 voxels at voxel_size 1 with negative keys among them, 8 of which give a row; used counts drawn from
{11, 63, 64, 65, 255, 256, 257, 1025} with n != m (the tile is 256 wide: T - 1, T, T + 1 and more than one tile per side are among
them, and 63 / 64 / 65 the wave's edge); keys in one cloud only and populations below min_pts = 11 give no row; the points are filed
in shuffled order.
TOLERANCES.  A sum of N non-negative doubles added in any order is within N 2^-53 (relative) of the exact sum, which the model forms
with math.fsum; 16 more cover two exp implementations a few ulp apart: (N + 16) 2^-53 for Sxx, Syy and Sxy, N that sum's term count.
mmd2_u and mmd2_b: the same factor (N the largest of the three counts) times the sum of the absolute values of their three terms.  The
Gaussian columns run the model's own arithmetic; only log may differ by an ulp or two: 4 2^-52 times the sum of the absolute terms of
the column (W2: of D, under the square root)."""
import ctypes as C
import math

import numpy as np
import pytest

import _voxdist_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
N_ROWS = 8
ARG, STATE, CAP = -1, -3, -4


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


_MMD = ("keys", "n_pop", "n_used", "ksum", "mmd2_u", "mmd2_b", "mean_mmd", "mean_mmd2_u")
_GAUSS = ("kl_est_gt", "kl_gt_est", "bhattacharyya", "w2")


def _bytes_mmd(res):
    """the rows' keys, counts, kernel sums and estimates: summed in the points' own order, a function of the points alone"""
    return b"".join(np.ascontiguousarray(res[k]).tobytes() for k in _MMD) + np.array([res["n_rows"], res["n_pairs_total"]], np.int64).tobytes()


def _bytes(res):
    """... and the Gaussian columns, a function of the two slots' voxel tables (which a slot keeps across every re-sort)"""
    return _bytes_mmd(res) + b"".join(np.ascontiguousarray(res[k]).tobytes() for k in _GAUSS) + \
        np.array([res["mean_kl_est_gt"], res["mean_kl_gt_est"], res["mean_bhattacharyya"], res["mean_w2"]], np.float64).tobytes()


@pytest.fixture(scope="module")
def S():
    """the scene, one device run at four bandwidths without sub-sampling, the voxel Gaussians, and the model's rows: made once, shared"""
    est, gt, want_keys = R.scene()
    with _engine() as e:
        e.upload(0, est)
        e.upload(1, gt)
        got = e.voxel_distances(R.VS, R.SIGMAS, min_pts=R.MIN_PTS, max_points=0)
        again = e.voxel_distances(R.VS, R.SIGMAS, min_pts=R.MIN_PTS, max_points=0)
        one = e.voxel_distances(R.VS, R.SIGMAS[:1], min_pts=R.MIN_PTS, max_points=0)
        sub = e.voxel_distances(R.VS, R.SIGMAS[:2], min_pts=R.MIN_PTS, max_points=64)
        vg = [e.voxel_gaussians(s, R.VS) for s in (0, 1)]
        awd = e.calculateVMD(R.VS, R.MIN_PTS, 5)
    rows = R.rows(est, gt, R.VS, R.MIN_PTS, 0)
    model = [[R.mmd_row(est[a], gt[b], s) for s in R.SIGMAS] for _, a, b, _, _ in rows]
    return dict(est=est, gt=gt, want_keys=want_keys, got=got, again=again, one=one, sub=sub, vg=vg, awd=awd, rows=rows, model=model)


def _check_mmd(got, rows, model, est, gt, sigmas):
    for r, (key, a, b, _, _) in enumerate(rows):
        for s in range(len(sigmas)):
            m = model[r][s]
            for k in range(3):
                want, n_terms = m["ksum"][k], m["terms"][k]
                have = got["ksum"][r, s, k]
                print(f"row {key} sigma {sigmas[s]} sum {k}: device {have!r} model {want!r} rel {abs(have - want) / want if want else 0.0:.3e}"
                      f" bound {(n_terms + 16) * U:.3e}")
                assert abs(have - want) <= (n_terms + 16) * U * want, (key, sigmas[s], k)
            f = (max(m["terms"]) + 16) * U
            assert abs(got["mmd2_u"][r, s] - m["u"]) <= f * m["u_abs"], (key, sigmas[s])
            assert abs(got["mmd2_b"][r, s] - m["b"]) <= f * m["b_abs"], (key, sigmas[s])


def test_rows_and_integer_outputs(S):
    got, rows = S["got"], S["rows"]
    assert got["n_rows"] == N_ROWS == len(rows)  # (an empty table cannot pass)
    assert [tuple(k) for k in got["keys"].tolist()] == S["want_keys"] == [r[0] for r in rows]
    assert (got["keys"] < 0).any()
    assert got["n_pop"].tolist() == [[r[3], r[4]] for r in rows] == got["n_used"].tolist()
    assert got["n_rows_subsampled"] == 0
    assert got["n_pairs_total"] == sum(n * (n - 1) // 2 + m * (m - 1) // 2 + n * m for _, _, _, n, m in rows)
    used = set(got["n_used"].ravel().tolist())
    assert used == {11, 63, 64, 65, 255, 256, 257, 1025} and (got["n_used"][:, 0] != got["n_used"][:, 1]).all()


def test_sums_and_both_estimates_against_the_exact_model(S):
    _check_mmd(S["got"], S["rows"], S["model"], S["est"], S["gt"], R.SIGMAS)
    got = S["got"]
    assert (got["mmd2_b"] >= -1e-12).all()
    assert np.array_equal(got["mmd"], np.sqrt(np.maximum(0.0, got["mmd2_b"])))
    # the means over the rows: a fixed-order sum of 8 values, within 8 u of the plain mean
    for s in range(4):
        assert abs(got["mean_mmd"][s] - got["mmd"][:, s].mean()) <= 16 * U * got["mmd"][:, s].mean()
        assert abs(got["mean_mmd2_u"][s] - got["mmd2_u"][:, s].mean()) <= 16 * U * np.abs(got["mmd2_u"][:, s]).mean()


def test_kernel_edges_duplicate_underflow_denormal(S):
    """the EDGE voxel: a point present in both clouds (d2 = 0, k = 1), a map point whose every cross pair underflows at sigma = 0.0125
    (d2 g > 745), and one whose cross pairs fall into the denormal range (d2 g near 720)"""
    est, gt = S["est"], S["gt"]
    r = S["want_keys"].index(R.EDGE)
    _, a, b, _, _ = S["rows"][r]
    g = 1.0 / (2.0 * R.SIGMAS[2] ** 2)
    X, Y = est[a], gt[b]
    d2 = ((X[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    with np.errstate(under="ignore"):
        k = np.exp(-(d2 * g))
    assert (d2 == 0.0).sum() == 1 and (k == 1.0).sum() == 1                      # the duplicate
    assert ((d2 * g > 745.2).all(axis=1)).any() and (k == 0.0).any()             # a point all of whose pairs underflow
    assert ((k > 0.0) & (k < np.finfo(np.float64).tiny)).any()                   # denormal terms
    have, want = S["got"]["ksum"][r, 2, 2], S["model"][r][2]["ksum"][2]
    assert want >= 1.0 and abs(have - want) <= (d2.size + 16) * U * want
    assert np.isfinite(S["got"]["ksum"]).all() and np.isfinite(S["got"]["mmd2_u"]).all()


def test_one_bandwidth_and_four_give_the_shared_column_bit_for_bit(S):
    got, one = S["got"], S["one"]
    assert one["ksum"].shape == (N_ROWS, 1, 3)
    assert one["ksum"][:, 0, :].tobytes() == np.ascontiguousarray(got["ksum"][:, 0, :]).tobytes()
    assert one["mmd2_u"][:, 0].tobytes() == np.ascontiguousarray(got["mmd2_u"][:, 0]).tobytes()
    assert one["mmd2_b"][:, 0].tobytes() == np.ascontiguousarray(got["mmd2_b"][:, 0]).tobytes()
    assert one["mean_mmd"][0] == got["mean_mmd"][0] and one["w2"].tobytes() == got["w2"].tobytes()


def test_subsampling_against_the_models_subset(S):
    """max_points = 64: 255 -> every 4th (64 used), 256 -> every 4th (64), 257 -> every 5th (52), 1025 -> every 17th (61), 65 -> every 2nd (33);
    the gate still looks at the full population"""
    sub, est, gt = S["sub"], S["est"], S["gt"]
    rows = R.rows(est, gt, R.VS, R.MIN_PTS, 64)
    assert sub["n_rows"] == N_ROWS and sub["n_pop"].tolist() == S["got"]["n_pop"].tolist()
    assert sub["n_used"].tolist() == [[len(a), len(b)] for _, a, b, _, _ in rows]
    assert {255: 64, 256: 64, 257: 52, 1025: 61, 65: 33, 64: 64, 63: 63, 11: 11} == \
        {int(p): int(u) for p, u in zip(sub["n_pop"].ravel(), sub["n_used"].ravel())}
    assert sub["n_rows_subsampled"] == sum(1 for _, _, _, n, m in rows if n > 64 or m > 64) == 6
    model = [[R.mmd_row(est[a], gt[b], s) for s in R.SIGMAS[:2]] for _, a, b, _, _ in rows]
    _check_mmd(sub, rows, model, est, gt, R.SIGMAS[:2])
    # the Gaussian columns do not depend on the sub-sample
    assert sub["w2"].tobytes() == S["got"]["w2"].tobytes() and sub["kl_est_gt"].tobytes() == S["got"]["kl_est_gt"].tobytes()


def test_gaussian_columns_against_the_operation_by_operation_model(S):
    got = S["got"]
    (ke, ne, mue, sge, _), (kg, ng, mug, sgg, _) = S["vg"]
    le = {tuple(k): i for i, k in enumerate(ke.tolist())}
    lg = {tuple(k): i for i, k in enumerate(kg.tolist())}
    floor_bit = False
    for r, key in enumerate(S["want_keys"]):
        i, j = le[key], lg[key]
        m = R.gauss_row(int(ne[i]), mue[i], sge[i], int(ng[j]), mug[j], sgg[j], 1e-6)
        have = (got["kl_est_gt"][r], got["kl_gt_est"][r], got["bhattacharyya"][r], got["w2"][r])
        print(f"row {key}: device {have!r} model {m['values']!r}")
        for c in range(3):
            assert abs(have[c] - m["values"][c]) <= 4 * 2.0 ** -52 * m["abs"][c], (key, c)
        assert abs(have[3] - m["values"][3]) * (have[3] + m["values"][3]) <= 4 * 2.0 ** -52 * m["abs"][3], key
        if key == R.PLANAR:
            Ce = np.asarray(sge[i]).reshape(3, 3) * (int(ne[i]) - 1)
            floor_bit = np.linalg.eigvalsh(0.5 * (Ce + Ce.T)).min() < 1e-6
            assert have[1] > 1000.0  # KL(gt || est) against a plane: tr(S~e^-1 S~g) ~ l_gt / floor
    assert floor_bit
    g4 = np.stack([got["kl_est_gt"], got["kl_gt_est"], got["bhattacharyya"], got["w2"]], 1)
    for c, name in enumerate(("mean_kl_est_gt", "mean_kl_gt_est", "mean_bhattacharyya", "mean_w2")):
        assert abs(got[name] - g4[:, c].mean()) <= 16 * U * np.abs(g4[:, c]).mean()


def _resort_both(e):
    for slot, radius in ((0, 0.31), (1, 0.17)):  # (a radius pass re-indexes a slot whose cell does not fit its radius)
        m0 = e.timer("morton")[1]
        e.local_geometry(slot, radius, 5)
        assert e.timer("morton")[1] > m0, "the slot was not re-sorted"


def test_two_calls_and_every_re_index_give_identical_bytes(S):
    assert _bytes(S["got"]) == _bytes(S["again"])
    run = dict(min_pts=R.MIN_PTS, max_points=0)
    with _engine() as e:
        e.upload(0, S["est"])
        e.upload(1, S["gt"])
        e.timers_enable(True)
        assert _bytes(e.voxel_distances(R.VS, R.SIGMAS, **run)) == _bytes(S["got"])
        _resort_both(e)
        assert _bytes(e.voxel_distances(R.VS, R.SIGMAS, **run)) == _bytes(S["got"])
        e.transform_cloud(0, np.eye(4))
        e.transform_cloud(1, np.eye(4))
        assert _bytes(e.voxel_distances(R.VS, R.SIGMAS, **run)) == _bytes(S["got"])
    # the sums are added in the points' own order: a slot first re-sorted, then evaluated, gives the same kernel sums bit for bit
    with _engine() as e:
        e.upload(0, S["est"])
        e.upload(1, S["gt"])
        e.timers_enable(True)
        _resort_both(e)
        assert _bytes_mmd(e.voxel_distances(R.VS, R.SIGMAS, **run)) == _bytes_mmd(S["got"])


def test_no_side_effects_on_the_resident_results(S):
    with _engine() as e:
        e.upload(0, S["est"])
        e.upload(1, S["gt"])
        e.mme(0, 0.3, 5)
        e.mme(1, 0.3, 5)
        e.nn1(0, 1, fetch=False)
        e.nn1(1, 0, fetch=False)

        def state():
            out = b""
            for s in (0, 1):
                idx, d2 = e.nn_fetch(s)
                ent, val = e.mme_fetch(s)
                out += idx.tobytes() + d2.tobytes() + ent.tobytes() + val.tobytes() + e.download(s).tobytes()
            v = e.calculateVMD(R.VS, R.MIN_PTS, 5)
            return out + v["rows"].tobytes() + v["w_sorted"].tobytes() + np.array([v["awd"], v["scs"]]).tobytes()

        before = state()
        res = e.voxel_distances(R.VS, R.SIGMAS, min_pts=R.MIN_PTS, max_points=0)
        assert state() == before
        assert _bytes_mmd(res) == _bytes_mmd(S["got"])


def test_count_only_call_and_every_refusal(S):
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import _addr

    def params(**kw):
        p = _lib.VoxDistParams()
        p.voxel_size, p.min_pts, p.n_sigma, p.max_points, p.eig_floor = 1.0, 11, 2, 0, 1e-6
        p.sigma[0], p.sigma[1] = 0.25, 0.05
        for k, v in kw.items():
            if k == "sigma1":
                p.sigma[1] = v
            else:
                setattr(p, k, v)
        return p

    with _engine() as e:
        L = e._L
        n = C.c_int64(0)
        assert L.me_voxel_distances(e._ctx, C.byref(params()), 0, 0, 0, 0, 0, 0, C.byref(n), None) == STATE  # nothing uploaded
        e.upload(0, S["est"])
        assert L.me_voxel_distances(e._ctx, C.byref(params()), 0, 0, 0, 0, 0, 0, C.byref(n), None) == STATE  # one slot only
        e.upload(1, S["gt"])
        e.timers_enable(True)
        n.value = 0
        assert L.me_voxel_distances(e._ctx, C.byref(params()), 0, 0, 0, 0, 0, 0, C.byref(n), None) == 0
        assert n.value == N_ROWS and e.timer("voxel_distances")[1] == 0  # the count alone: no kernel of the feature ran
        good = e.voxel_distances(1.0, (0.25, 0.05), min_pts=11, max_points=0)
        before = _bytes(good)
        keys, ks = np.full((N_ROWS, 3), -7, np.int32), np.full((N_ROWS, 2, 3), -7.0)
        bad = [dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(min_pts=10), dict(n_sigma=0), dict(n_sigma=5), dict(sigma1=0.0),
               dict(sigma1=-0.1), dict(sigma1=float("nan")), dict(max_points=-1), dict(max_points=1), dict(max_points=10),
               dict(eig_floor=0.0), dict(eig_floor=-1e-6), dict(voxel_size=1e-7)]  # (the last: a voxel index out of range)
        for kw in bad:
            n.value = N_ROWS
            rc = L.me_voxel_distances(e._ctx, C.byref(params(**kw)), _addr(keys), 0, 0, _addr(ks), 0, 0, C.byref(n), None)
            assert rc == ARG, kw
            assert (keys == -7).all() and (ks == -7.0).all()
        n.value = N_ROWS - 1
        assert L.me_voxel_distances(e._ctx, C.byref(params()), _addr(keys), 0, 0, _addr(ks), 0, 0, C.byref(n), None) == CAP
        assert n.value == N_ROWS and (keys == -7).all() and (ks == -7.0).all()
        assert L.me_voxel_distances(e._ctx, None, 0, 0, 0, 0, 0, 0, C.byref(n), None) == ARG
        e.voxel_distances(1.0, (0.25, 0.05), min_pts=11, max_points=11)  # the smallest max_points that is accepted
        assert _bytes(e.voxel_distances(1.0, (0.25, 0.05), min_pts=11, max_points=0)) == before  # a refused call changed nothing
        # no rows: the count is 0 and the means are NaN, as AWD's
        none = e.voxel_distances(1.0, (0.25,), min_pts=5000, max_points=0)
        assert none["n_rows"] == 0 and none["keys"].shape == (0, 3) and np.isnan(none["mean_mmd"]).all() and math.isnan(none["mean_w2"])
        # slab mode is refused
        e.set_slab(0, -1.0, 1.0, 0.5)
        e.upload(0, S["est"])
        assert L.me_voxel_distances(e._ctx, C.byref(params()), 0, 0, 0, 0, 0, 0, C.byref(n), None) == STATE


def test_the_rows_are_the_rows_of_awd(S):
    awd = S["awd"]
    assert awd["n_rows"] == N_ROWS
    keys = np.rint(awd["rows"][:, 0:3] / R.VS).astype(np.int32)
    assert np.array_equal(keys, S["got"]["keys"])
    assert np.array_equal(awd["rows"][:, 10:12].astype(np.int32), S["got"]["n_pop"][:, ::-1])  # (voxel_errors.txt lists gt first)
    # swapping the clouds swaps Sxx / Syy and the two KL columns
    with _engine() as e:
        e.upload(0, S["gt"])
        e.upload(1, S["est"])
        sw = e.voxel_distances(R.VS, R.SIGMAS[:1], min_pts=R.MIN_PTS, max_points=0)
    assert sw["ksum"][:, 0, 0].tobytes() == S["one"]["ksum"][:, 0, 1].tobytes() and sw["ksum"][:, 0, 1].tobytes() == S["one"]["ksum"][:, 0, 0].tobytes()
    assert np.array_equal(sw["kl_est_gt"], S["one"]["kl_gt_est"]) and np.array_equal(sw["kl_gt_est"], S["one"]["kl_est_gt"])
