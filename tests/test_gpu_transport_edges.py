"""me_voxel_transport at its edges on the MI355X, against the numpy model of tests/_transport_ref.py, on the scene of _voxdist_ref
(13 voxels, 8 rows, used counts from {11, 63, 64, 65, 255, 256, 257, 1025} with n != m, negative keys, shuffled filing), run with
max_points = 1024 (1025 becomes 513: the sub-sample path) and with max_points = 64.
TOLERANCES.  Sliced: the model forms the same float64 terms w (d d); their sum in any order is within N 2^-53 (relative) of math.fsum,
16 more for the division: (n + m + 16) 2^-53.  The sum in the kernel's stated order is restated too and must match bit for bit.
Sinkhorn: the project's bar, 1e-9: a potential relative to max |f|, an OT value relative to the largest potentials it averages, S
relative to the sum of the absolute values of its three terms, marginal_err (a share of the unit mass) 1e-9 + (n + 16) 2^-53.  The
device's exp / log are not libm's, so no tighter bound is fixed; each LSE update is non-expansive in the sup norm, so T iterations add
their rounding and do not amplify it.  The test prints, per row, device minus model and model minus its long-double twin.
RE-INDEXING.  A row's points are taken in ascending ORIGINAL index, so the results are a function of the uploaded arrays: identical
bytes from call to call, after every re-sort of a slot and on a slot re-sorted before its first evaluation."""
import ctypes as C
import math

import numpy as np
import pytest

import _transport_ref as T
import _voxdist_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BAR = 1e-9
N_ROWS = 8
ARG, STATE, CAP = -1, -3, -4
EPS3 = (0.5, 0.1, 0.02)  # three iterations: nothing has converged
BLUR = R.VS / 5
FLAT_DIR = 63            # directions[63] = +z: the est points of the PLANAR voxel all project to one value

_ROWS = ("keys", "n_pop", "n_used")
_SLICED = ("sw2_sq", "sw2", "max_sw2_sq", "max_dir", "per_direction")
_SINK = ("ot_xy", "ot_xx", "ot_yy", "s", "sinkhorn", "marginal_err")


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _part(res, names, scalars):
    return b"".join(np.ascontiguousarray(res[k]).tobytes() for k in names) + np.array([res[k] for k in scalars], np.float64).tobytes()


def _bytes_sliced(res):
    return _part(res, _ROWS + _SLICED, ("n_rows", "n_pairs_total", "mean_sw2", "mean_max_sw2"))


def _bytes_sink(res):
    return _part(res, _ROWS + _SINK, ("n_rows", "mean_s", "mean_sinkhorn", "mean_marginal_err", "max_marginal_err", "max_marginal_row")) + \
        b"".join(a.tobytes() for a in res["f"] + res["g"])


def _bytes(res):
    return _bytes_sliced(res) + _bytes_sink(res)


def _dirs():
    from cloud_map_evaluation_amd import synth

    d = synth.fibonacci_directions(64)
    d[FLAT_DIR] = (0.0, 0.0, 1.0)
    return d


def _models(est, gt, rows, dirs, eps, long_double=True):
    out = []
    for _, a, b, _, _ in rows:
        X, Y = est[a], gt[b]
        out.append(dict(sl=T.sliced_row(X, Y, dirs), sk=T.sinkhorn_row(X, Y, eps),
                        hi=T.sinkhorn_row(X, Y, eps, np.longdouble) if long_double else None))
    return out


@pytest.fixture(scope="module")
def S():
    """the scene, every device run on it, and the model's rows: made once, shared"""
    from cloud_map_evaluation_amd.engine import transport_schedule

    est, gt, want_keys = R.scene()
    dirs = _dirs()
    dflt = transport_schedule(R.VS, BLUR)
    kw = dict(directions=dirs, min_pts=R.MIN_PTS)
    with _engine() as e:
        e.upload(0, est)
        e.upload(1, gt)
        got = e.voxel_transport(R.VS, eps_schedule=EPS3, max_points=1024, **kw)
        again = e.voxel_transport(R.VS, eps_schedule=EPS3, max_points=1024, **kw)
        full = e.voxel_transport(R.VS, blur=BLUR, max_points=1024, **kw)
        sub = e.voxel_transport(R.VS, blur=BLUR, max_points=64, **kw)
        sub3 = e.voxel_transport(R.VS, eps_schedule=EPS3, max_points=64, **kw)
        one = e.voxel_transport(R.VS, eps_schedule=EPS3, max_points=1024, directions=dirs[5:6], min_pts=R.MIN_PTS)
        no_l = e.voxel_transport(R.VS, eps_schedule=EPS3, max_points=1024, directions=0, min_pts=R.MIN_PTS)
        no_t = e.voxel_transport(R.VS, eps_schedule=(), max_points=1024, **kw)
        huge = e.voxel_transport(R.VS, eps_schedule=(1e6,), max_points=64, **kw)
        tiny = e.voxel_transport(R.VS, eps_schedule=((R.VS / 200) ** 2,) * 3, max_points=64, **kw)
        vd = [e.voxel_distances(R.VS, (0.25,), min_pts=R.MIN_PTS, max_points=mp) for mp in (1024, 64)]
    rows = R.rows(est, gt, R.VS, R.MIN_PTS, 1024)
    rows64 = R.rows(est, gt, R.VS, R.MIN_PTS, 64)
    return dict(est=est, gt=gt, want_keys=want_keys, dirs=dirs, dflt=dflt, got=got, again=again, full=full, sub=sub, sub3=sub3, one=one,
                no_l=no_l, no_t=no_t, huge=huge, tiny=tiny, vd=vd, rows=rows, rows64=rows64,
                m_got=_models(est, gt, rows, dirs, EPS3), m_sub=_models(est, gt, rows64, dirs, dflt),
                m_full=_models(est, gt, rows, dirs[:1], dflt, long_double=False))


def test_rows_and_integer_outputs(S):
    for res, rows, k in ((S["got"], S["rows"], 0), (S["sub"], S["rows64"], 1)):
        assert res["n_rows"] == N_ROWS == len(rows)
        assert [tuple(x) for x in res["keys"].tolist()] == S["want_keys"] == [r[0] for r in rows]
        assert res["n_pop"].tolist() == [[r[3], r[4]] for r in rows]
        assert res["n_used"].tolist() == [[len(r[1]), len(r[2])] for r in rows]
        vd = S["vd"][k]
        assert np.array_equal(res["keys"], vd["keys"]) and np.array_equal(res["n_pop"], vd["n_pop"]) and np.array_equal(res["n_used"], vd["n_used"])
        assert res["n_rows_subsampled"] == vd["n_rows_subsampled"]
        assert res["n_pairs_total"] == sum(len(r[1]) * len(r[2]) for r in rows)
        assert (res["n_used_est"], res["n_used_gt"]) == (sum(len(r[1]) for r in rows), sum(len(r[2]) for r in rows))
        assert [len(a) for a in res["f"]] == [len(r[1]) for r in rows] and [len(a) for a in res["g"]] == [len(r[2]) for r in rows]
    assert (S["got"]["keys"] < 0).any() and 513 in S["got"]["n_used"] and S["got"]["n_rows_subsampled"] == 2
    assert S["sub"]["n_used"].max() == 64 and S["sub"]["n_rows_subsampled"] == 6


def _check_sliced(res, rows, models, n_dir):
    for r, (key, a, b, _, _) in enumerate(rows):
        sl = models[r]["sl"]
        n, m = len(a), len(b)
        for l in range(n_dir):
            have, want = res["per_direction"][r, l], sl["exact"][l]
            print(f"row {key} dir {l}: device {have!r} fsum {want!r} rel {abs(have - want) / want if want else 0.0:.3e} bound {(n + m + 16) * U:.3e}")
            assert abs(have - want) <= (n + m + 16) * U * want, (key, l)
        # the stated order, restated: the same bytes (sorted projections that differed from numpy's would show here)
        assert res["per_direction"][r, :n_dir].tobytes() == sl["ordered"][:n_dir].tobytes(), key


def test_sliced_against_the_exact_model_and_the_stated_order(S):
    for res, rows, models in ((S["got"], S["rows"], S["m_got"]), (S["sub"], S["rows64"], S["m_sub"])):
        _check_sliced(res, rows, models, 64)
        for r, (key, _, _, _, _) in enumerate(rows):
            o, x = models[r]["sl"]["by_order"], models[r]["sl"]["by_exact"]
            assert res["max_dir"][r] == o["max_dir"] == x["max_dir"], key
            assert res["sw2_sq"][r] == o["sw2_sq"] and res["max_sw2_sq"][r] == o["max_sw2_sq"], key
            assert abs(res["sw2"][r] - o["sw2"]) <= 4 * U * o["sw2"], key
            assert res["sw2_sq"][r] <= res["max_sw2_sq"][r]
        sw, mx = res["sw2"], np.sqrt(res["max_sw2_sq"])
        assert abs(res["mean_sw2"] - sw.mean()) <= 16 * U * sw.mean() and abs(res["mean_max_sw2"] - mx.mean()) <= 16 * U * mx.mean()


def test_sliced_edges_flat_direction_duplicates_one_and_sixty_four(S):
    # the PLANAR voxel along +z: every est projection is the same double
    r = S["want_keys"].index(R.PLANAR)
    _, a, b, _, _ = S["rows"][r]
    pa = T.project(S["est"][a], S["dirs"][FLAT_DIR])
    assert (pa == pa[0]).all() and len(pa) == 64
    want = math.fsum((T.project(S["gt"][b], S["dirs"][FLAT_DIR]) - pa[0]) ** 2) / len(b)  # every atom of X at one place
    have = S["got"]["per_direction"][r, FLAT_DIR]
    assert abs(have - want) <= (len(a) + len(b) + 16) * U * want
    # L = 1 gives the bytes L = 64 gives for that direction
    assert S["one"]["per_direction"].shape == (N_ROWS, 1)
    assert S["one"]["per_direction"][:, 0].tobytes() == np.ascontiguousarray(S["got"]["per_direction"][:, 5]).tobytes()
    assert (S["one"]["max_dir"] == 0).all() and S["one"]["sw2_sq"].tobytes() == S["one"]["max_sw2_sq"].tobytes()
    # duplicates inside both clouds and across them
    X, Y = T.doubled_wall(40, 37, 1.0, 0.05, 3)
    X[1] = X[0]
    Y[5] = Y[4] = Y[3]
    X[2] = Y[3]
    with _engine() as e:
        e.upload(0, X)
        e.upload(1, Y)
        res = e.voxel_transport(1.0, eps_schedule=EPS3, directions=S["dirs"][56:], min_pts=11, max_points=64)
    assert res["n_rows"] == 1 and res["n_used"].tolist() == [[40, 37]]
    model = [dict(sl=T.sliced_row(X, Y, S["dirs"][56:]))]
    _check_sliced(res, [((0, 0, 0), list(range(40)), list(range(37)), 40, 37)], model, 8)
    sk = T.sinkhorn_row(X, Y, EPS3)
    assert np.abs(res["f"][0] - sk["f"]).max() <= BAR * np.abs(sk["f"]).max() and abs(res["s"][0] - sk["s"]) <= BAR * sk["s_abs"]


def test_sliced_direction_flat_on_both_sides():
    """both clouds in planes z = const, the direction +z: every projection of a side is one double (p = ((x 0) + (y 0)) + (z 1) = z), both
    sorts see nothing but ties, and W2^2 is the square of the one difference: exactly for n = m = 16 (16 equal terms 16 (d d), every partial
    sum a power-of-two multiple of d d), within the sum's bound for 40 x 37"""
    rng = np.random.default_rng(5)
    za, zb = 0.3, 0.7
    d2 = (za - zb) * (za - zb)
    u = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    for n, m in ((16, 16), (40, 37)):
        X, Y = 0.05 + 0.9 * rng.random((n, 3)), 0.05 + 0.9 * rng.random((m, 3))
        X[:, 2], Y[:, 2] = za, zb
        with _engine() as e:
            e.upload(0, X)
            e.upload(1, Y)
            res = e.voxel_transport(1.0, eps_schedule=(), directions=u, min_pts=11, max_points=64)
        assert res["n_rows"] == 1 and res["n_used"].tolist() == [[n, m]]
        have = res["per_direction"][0, 0]
        assert abs(have - d2) <= (n + m + 16) * U * d2 and (have == d2 or n != m)
        assert res["per_direction"][0].tobytes() == T.sliced_row(X, Y, u)["ordered"].tobytes()
        assert res["max_dir"][0] == 0 and res["max_sw2_sq"][0] == have  # (0.16 across the planes; along x two uniform samples)


def _check_sinkhorn(name, res, rows, models):
    worst = dict(dev=0.0, model=0.0)
    for r, (key, a, b, _, _) in enumerate(rows):
        sk, hi = models[r]["sk"], models[r]["hi"]
        n = len(a)
        fs, gs = np.abs(sk["f"]).max(), np.abs(sk["g"]).max()
        df, dg = np.abs(res["f"][r] - sk["f"]).max() / fs, np.abs(res["g"][r] - sk["g"]).max() / gs
        ds = abs(res["s"][r] - sk["s"]) / sk["s_abs"]
        line = f"{name} row {key}: device - model: f {df:.3e} g {dg:.3e} S {ds:.3e} marginal {res['marginal_err'][r] - sk['marginal_err']:.3e}"
        worst["dev"] = max(worst["dev"], df, dg, ds)
        if hi is not None:
            mf = float(np.abs(sk["f"] - hi["f"]).max() / fs)
            ms = float(abs(sk["s"] - hi["s"]) / sk["s_abs"])
            worst["model"] = max(worst["model"], mf, ms)
            line += f" | model - long double: f {mf:.3e} S {ms:.3e}"
        print(line)
        assert df <= BAR and dg <= BAR, key
        assert abs(res["ot_xy"][r] - sk["ot_xy"]) <= BAR * (fs + gs), key
        for c in ("ot_xx", "ot_yy"):
            assert abs(res[c][r] - sk[c]) <= BAR * sk[c + "_scale"], (key, c)
        assert ds <= BAR, key
        assert abs(res["marginal_err"][r] - sk["marginal_err"]) <= BAR + (n + 16) * U, key
        root = math.sqrt(max(0.0, res["s"][r]))
        assert abs(res["sinkhorn"][r] - root) <= 4 * U * root, key
    print(f"{name}: largest device - model {worst['dev']:.3e}, largest model - long double {worst['model']:.3e} (the bar: {BAR})")
    for k in ("s", "sinkhorn", "marginal_err"):
        assert abs(res["mean_" + k] - res[k].mean()) <= 16 * U * np.abs(res[k]).mean()
    assert res["max_marginal_err"] == res["marginal_err"].max() and res["max_marginal_row"] == int(np.argmax(res["marginal_err"]))


def test_sinkhorn_three_iterations_against_the_float64_model(S):
    _check_sinkhorn("3 iterations, max_points 1024", S["got"], S["rows"], S["m_got"])


def test_sinkhorn_default_schedule_against_the_float64_model(S):
    assert len(S["dflt"]) == 4 + 1 + 128 and S["sub"]["eps_schedule"].tobytes() == S["dflt"].tobytes()
    _check_sinkhorn("default schedule, max_points 64", S["sub"], S["rows64"], S["m_sub"])
    _check_sinkhorn("default schedule, max_points 1024", S["full"], S["rows"], S["m_full"])
    assert (S["sub"]["s"] >= -1e-12).all() and (S["full"]["s"] >= -1e-12).all()


def test_sinkhorn_huge_and_tiny_eps(S):
    huge, tiny, rows = S["huge"], S["tiny"], S["rows64"]
    n_under = n_terms = 0
    for r, (key, a, b, _, _) in enumerate(rows):
        X, Y = S["est"][a], S["gt"][b]
        # T = 1 at eps = 1e6: every t_ij - M_i is 0 to 3e-6, so f_i = -eps log(sum_j b exp(-C_ij / eps)) is the mean cost of point i up
        # to C^2 / eps (the second cumulant) and eps times the rounding of a logarithm near log m; the plan is uniform to (C / eps)^2
        C = T.cost(X, Y)
        assert np.abs(huge["f"][r] - C.mean(1)).max() <= 1e-5, key
        assert huge["marginal_err"][r] <= 1e-9, key
        sk = T.sinkhorn_row(X, Y, tiny["eps_schedule"])
        t = (sk["g"][None, :] - C) / tiny["eps_schedule"][-1]
        with np.errstate(under="ignore"):
            under = np.exp(t - t.max(1)[:, None]) == 0.0
        n_under, n_terms = n_under + int(under.sum()), n_terms + under.size
        assert np.abs(tiny["f"][r] - sk["f"]).max() <= BAR * np.abs(sk["f"]).max() and abs(tiny["s"][r] - sk["s"]) <= BAR * sk["s_abs"], key
    assert n_under > 0.5 * n_terms  # most terms of the scene underflow (not in the EDGE voxel, whose ground truth is a 1 cm cluster)
    for res in (huge, tiny):
        for k in _SINK:
            assert np.isfinite(res[k]).all(), k
        assert all(np.isfinite(a).all() for a in res["f"] + res["g"])


def test_either_part_alone_gives_the_same_bytes(S):
    got, no_l, no_t = S["got"], S["no_l"], S["no_t"]
    assert _bytes_sink(no_l) == _bytes_sink(got) and _bytes_sliced(no_t) == _bytes_sliced(got)
    assert np.isnan(no_l["sw2_sq"]).all() and math.isnan(no_l["mean_sw2"]) and (no_l["max_dir"] == -1).all() and no_l["per_direction"].shape == (N_ROWS, 0)
    assert np.isnan(no_t["s"]).all() and math.isnan(no_t["mean_s"]) and no_t["max_marginal_row"] == -1 and no_t["f"] == []
    # the Sinkhorn part does not depend on the directions, the sliced part not on the schedule
    assert _bytes_sink(S["one"]) == _bytes_sink(got) and _bytes_sliced(S["sub3"]) == _bytes_sliced(S["sub"])


def _resort_both(e):
    for slot, radius in ((0, 0.31), (1, 0.17)):  # (a radius pass re-indexes a slot whose cell does not fit its radius)
        m0 = e.timer("morton")[1]
        e.local_geometry(slot, radius, 5)
        assert e.timer("morton")[1] > m0, "the slot was not re-sorted"


def test_two_calls_and_every_re_index_give_identical_bytes(S):
    assert _bytes(S["got"]) == _bytes(S["again"])
    run = dict(eps_schedule=EPS3, max_points=1024, directions=S["dirs"], min_pts=R.MIN_PTS)
    with _engine() as e:
        e.upload(0, S["est"])
        e.upload(1, S["gt"])
        e.timers_enable(True)
        _resort_both(e)  # re-sorted before the first evaluation
        assert _bytes(e.voxel_transport(R.VS, **run)) == _bytes(S["got"])
        assert e.timer("voxel_transport")[1] > 0
        e.transform_cloud(0, np.eye(4))
        e.transform_cloud(1, np.eye(4))
        assert _bytes(e.voxel_transport(R.VS, **run)) == _bytes(S["got"])


def test_count_only_call_and_every_refusal(S):
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import _addr

    dirs = np.ascontiguousarray(S["dirs"][:4])

    def call(e, n, eps=EPS3, dirs_addr=None, eps_addr=None, keys=0, sl=0, out=None, **kw):
        p = _lib.VoxTransParams()
        p.voxel_size, p.min_pts, p.n_dir, p.n_eps, p.reserved, p.max_points = 1.0, 11, 4, len(eps), 0, 64
        for k, v in kw.items():
            setattr(p, k, v)
        ea = np.array(eps, np.float64)
        return e._L.me_voxel_transport(e._ctx, C.byref(p), _addr(dirs) if dirs_addr is None else dirs_addr,
                                       _addr(ea) if eps_addr is None else eps_addr, keys, 0, 0, sl, 0, 0, 0, C.byref(n), out)

    with _engine() as e:
        n = C.c_int64(0)
        assert call(e, n) == STATE  # nothing uploaded
        e.upload(0, S["est"])
        assert call(e, n) == STATE  # one slot only
        e.upload(1, S["gt"])
        e.timers_enable(True)
        assert call(e, n) == 0 and n.value == N_ROWS and e.timer("voxel_transport")[1] == 0  # the count alone: no kernel of the feature ran
        run = dict(eps_schedule=EPS3, max_points=64, directions=dirs, min_pts=11)
        before = _bytes(e.voxel_transport(1.0, **run))
        keys, sl = np.full((N_ROWS, 3), -7, np.int32), np.full((N_ROWS, 4), -7.0)
        nan = float("nan")
        bad = [dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=nan), dict(min_pts=10), dict(n_dir=-1), dict(n_dir=65), dict(n_eps=-1),
               dict(n_eps=513), dict(n_dir=0, n_eps=0), dict(max_points=10), dict(max_points=0), dict(max_points=1025),
               dict(eps=(0.5, 0.0, 0.0)), dict(eps=(0.5, -0.1, -0.2)), dict(eps=(0.1, 0.2, 0.05)), dict(eps=(0.5, nan, 0.1)), dict(eps=(nan,)),
               dict(dirs_addr=0), dict(eps_addr=0), dict(voxel_size=1e-7)]  # (the last: a voxel index out of range)
        for kw in bad:
            n.value = N_ROWS
            assert call(e, n, keys=_addr(keys), sl=_addr(sl), **kw) == ARG, kw
            assert (keys == -7).all() and (sl == -7.0).all()
        n.value = N_ROWS - 1
        assert call(e, n, keys=_addr(keys), sl=_addr(sl)) == CAP and n.value == N_ROWS and (keys == -7).all() and (sl == -7.0).all()
        assert e._L.me_voxel_transport(e._ctx, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, C.byref(n), None) == ARG
        assert _bytes(e.voxel_transport(1.0, **run)) == before  # a refused call changed nothing
        e.voxel_transport(1.0, eps_schedule=(0.1,) * 512, max_points=11, directions=dirs[:1], min_pts=11, fetch=False)  # the largest T, smallest max_points
        assert _bytes(e.voxel_transport(1.0, **run)) == before
        none = e.voxel_transport(1.0, eps_schedule=EPS3, directions=dirs, min_pts=5000)
        assert none["n_rows"] == 0 and none["keys"].shape == (0, 3) and math.isnan(none["mean_sw2"]) and math.isnan(none["mean_s"])
        e.set_slab(0, -1.0, 1.0, 0.5)
        e.upload(0, S["est"])
        assert call(e, n) == STATE  # slab mode is refused


def test_model_inequalities_on_the_devices_own_numbers():
    """the 64-point doubled-wall pair of tests/test_transport_cpu.py: the sandwich around the exact W2^2 and S >= 0, from the device"""
    from scipy.optimize import linear_sum_assignment

    from cloud_map_evaluation_amd import synth

    n = 64
    X, Y = T.doubled_wall(n, n, 1.0, 0.05, 0)
    Cm = T.cost(X, Y)
    i, j = linear_sum_assignment(Cm)
    exact = Cm[i, j].sum() / n
    eps = 0.2 * 0.2
    with _engine() as e:
        e.upload(0, X)
        e.upload(1, Y)
        res = e.voxel_transport(1.0, eps_schedule=(eps,) * 400, directions=synth.fibonacci_directions(32), min_pts=11, max_points=64)
        e.upload(1, X)
        same = e.voxel_transport(1.0, eps_schedule=(eps,) * 400, directions=1, min_pts=11, max_points=64)
    assert res["n_rows"] == 1 and res["n_used"].tolist() == [[n, n]]
    slack = res["marginal_err"][0] * Cm.max() + 1e-12
    print(f"sw2_sq {res['sw2_sq'][0]:.6g} <= max {res['max_sw2_sq'][0]:.6g} <= exact {exact:.6g} <= OT_eps {res['ot_xy'][0]:.6g} <= "
          f"{exact + eps * math.log(n):.6g}; marginal_err {res['marginal_err'][0]:.3g}; S {res['s'][0]:.6g}; S(X, X) {same['s'][0]:.3g}")
    assert res["sw2_sq"][0] <= res["max_sw2_sq"][0] <= exact + 1e-12
    assert exact <= res["ot_xy"][0] + slack and res["ot_xy"][0] <= exact + eps * math.log(n) + slack
    assert res["s"][0] >= -slack
    assert abs(same["s"][0]) <= same["marginal_err"][0] * T.cost(X, X).max() + 1e-12 and same["sw2_sq"][0] == 0.0
