"""me_nn_error_distribution / Engine.error_report on the MI355X (csrc/me_errdist.hip) against the numpy model (tests/_errdist_ref.py).

Injected squared distances (Engine.set_nn_result) put an entry on every edge on purpose; every count, rank, quantile_d2, argmax and
histogram bin is compared with ==, quantile_d / min_d / max_d with the host sqrt of their d2, the two sums within the derived bound
(count - 1) 2^-53 sum (the device's sqrt is within one ulp of the model's: one more 2^-52 on sum_d)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _errdist_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TAUS = [0.2, 0.1, 0.08, 0.05, 0.01]
Q16 = [0.0, 1.0, 0.5, 0.5, 0.25, 0.9, 0.95, 0.99, 0.999, 0.01, 0.1, 0.3, 0.7, 1e-9, 0.75, 0.05]


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    with Engine(0) as e:
        yield e


def _compare(dev, ref, bins):
    for f in ("n_query", "n_used", "argmax", "n_overflow"):
        assert dev[f] == ref[f], (f, dev[f], ref[f])
    for f in ("rank", "n_within", "hist"):
        assert np.array_equal(dev[f], ref[f]), (f, dev[f], ref[f])
    assert len(dev["hist"]) == bins
    assert np.array_equal(R.bits(dev["quantile_d2"]), R.bits(ref["quantile_d2"]))
    assert np.array_equal(R.bits(dev["quantile_d"]), R.bits(np.sqrt(dev["quantile_d2"])))
    assert dev["min_d"] == math.sqrt(ref["min_d2"]) and dev["max_d"] == math.sqrt(ref["max_d2"])
    assert abs(dev["sum_d2"] - ref["sum_d2"]) <= R.sum_bound(ref["n_used"], ref["sum_d2"])
    assert abs(dev["sum_d"] - ref["sum_d"]) <= R.sum_bound(ref["n_used"], ref["sum_d"]) + 2 * R.EPS * ref["sum_d"]
    if ref["n_used"] == 0:
        assert (dev["sum_d"], dev["sum_d2"], dev["min_d"], dev["max_d"]) == (0.0, 0.0, 0.0, 0.0)


def _edge_d2(n, rng, bins, width):
    """n squared distances around a random body: the thresholds' t2max and their successors, bin edges, the last edge and beyond, zeros,
    and the maximum at several indices."""
    d2 = (rng.random(n) * 0.3) ** 2
    special = [0.0, 0.0]
    for t in TAUS:
        x = R.t2max(t)
        special += [x, float(np.nextafter(x, np.inf)), float(np.nextafter(x, 0.0))]
    if bins:
        E = R.edges(bins, width)
        for j in sorted({0, min(1, bins - 1), bins // 2, bins - 1}):
            special += [float(E[j]), float(np.nextafter(E[j], np.inf))]
        special += [float(E[-1]) * 4.0]
    top = max(max(special), float(d2.max())) * 2.0
    special += [top] * 3
    special = np.array(special[:n] if n < len(special) else special)
    pos = rng.permutation(n)[:len(special)]
    d2[pos] = special
    return d2


@pytest.mark.parametrize("n", [1, 2, 4097, 256 * R.STAT_BLOCKS + 1])
def test_injected_distances_on_every_edge(eng, n):
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3))
    eng.upload(0, pts)
    eng.upload(1, pts[: max(1, n // 2)])
    for bins, width in ((0, 0.0), (1, 0.25), (4096, 0.4 / 4096), (37, 0.01)):
        d2 = _edge_d2(n, rng, bins, width)
        eng.set_nn_result(0, 1, d2)
        for quantiles in ([0.5], Q16, []):
            for gate, mode in ((-1.0, 0), (0.15, R.GATE_LT_SQUARED), (0.15 * 0.15, R.GATE_LE_UNSQUARED), (0.0, R.GATE_LT_SQUARED)):
                dev = eng.nn_error_distribution(0, quantiles, TAUS, bins, width, gate, mode)
                ref = R.error_distribution(d2, quantiles, TAUS, bins, width, gate, mode)
                _compare(dev, ref, bins)
                if gate == 0.0:
                    assert dev["n_used"] == 0 and dev["argmax"] == -1 and np.all(dev["rank"] == -1) and not dev["quantile_d2"].any()


def test_ties_for_the_maximum_and_entries_that_are_no_query(eng):
    rng = np.random.default_rng(5)
    n = 3000
    pts = rng.random((n, 3))
    eng.upload(0, pts)
    eng.upload(1, pts[:10])
    d2 = rng.random(n)
    d2[[2999, 17, 1500, 18]] = 7.0
    d2[[3, 100]] = -1.0  # (what a slab's halo point carries: no query)
    eng.set_nn_result(0, 1, d2)
    dev = eng.nn_error_distribution(0, [0.5, 1.0], [0.5])
    assert dev["argmax"] == 17 and dev["n_query"] == dev["n_used"] == n - 2 and dev["quantile_d2"][1] == 7.0 and dev["max_d"] == math.sqrt(7.0)
    _compare(dev, R.error_distribution(d2, [0.5, 1.0], [0.5]), 0)
    # gated below the maximum: the worst of what is left
    dev = eng.nn_error_distribution(0, [1.0], gate=1.0, gate_mode=R.GATE_LE_UNSQUARED)
    _compare(dev, R.error_distribution(d2, [1.0], gate=1.0, gate_mode=R.GATE_LE_UNSQUARED), 0)
    assert dev["argmax"] == int(np.argmax(np.where(d2 <= 1.0, d2, -1.0)))


@pytest.fixture(scope="module")
def pair(eng):
    from cloud_map_evaluation_amd import synth

    est, gt = synth.cube_pair(20_000, seed=11)
    est, gt = est.numpy(), gt.numpy()

    import torch

    def brute(a, b):
        # the exhaustive minimum of ((dx dx + dy dy) + dz dz) over all 20 000 x 20 000 pairs: separate fp64 elementwise multiplications
        # and additions of torch (each correctly rounded, nothing contracted), in chunks of 1000 queries
        a, b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        out = torch.empty(len(a), dtype=torch.float64, device="cuda")
        for s in range(0, len(a), 1000):
            dx, dy, dz = (a[s:s + 1000, k:k + 1] - b[None, :, k] for k in range(3))
            out[s:s + 1000] = torch.add(torch.add(torch.mul(dx, dx), torch.mul(dy, dy)), torch.mul(dz, dz)).min(dim=1).values
        return out.cpu().numpy()

    return est, gt, brute(est, gt), brute(gt, est)


def test_end_to_end_against_brute_force(eng, pair):
    est, gt, d2_eg, d2_ge = pair
    eng.upload(0, est)
    eng.upload(1, gt)
    _, dev_eg = eng.nn1(0, 1)
    _, dev_ge = eng.nn1(1, 0)
    assert np.array_equal(dev_eg, d2_eg) and np.array_equal(dev_ge, d2_ge)
    width = float(np.sqrt(max(d2_eg.max(), d2_ge.max()))) / 100
    before = eng.nn_stats(0, 2.5, 0, TAUS)
    rep = eng.error_report(TAUS, bins=128, bin_width=width)
    after = eng.nn_stats(0, 2.5, 0, TAUS)
    for f in ("mean", "rmse", "fitness", "sigma", "number"):
        assert getattr(before, f).tobytes() == getattr(after, f).tobytes()
    assert np.array_equal(eng.nn_fetch(0)[1], d2_eg)  # the call left nn_d2 untouched
    refs = {"est": R.error_distribution(d2_eg, (0.5, 0.9, 0.95, 0.99), TAUS, 128, width),
            "gt": R.error_distribution(d2_ge, (0.5, 0.9, 0.95, 0.99), TAUS, 128, width)}
    for side in ("est", "gt"):
        _compare(rep[side], refs[side], 128)
        assert rep[side]["hist"].sum() + rep[side]["n_overflow"] == rep[side]["n_used"] == 20_000
    assert rep["hausdorff"] == max(math.sqrt(d2_eg.max()), math.sqrt(d2_ge.max()))
    for k in range(len(TAUS)):
        P, Rc, F = R.fscore(refs["est"]["n_within"][k], 20_000, refs["gt"]["n_within"][k], 20_000)
        assert (rep["precision"][k], rep["recall"][k], rep["fscore"][k]) == (P, Rc, F)
    # the threshold counts are the inlier counts of the ungated statistics, from the same rule
    assert [int(x) for x in eng.nn_stats(0, -1.0, 0, TAUS).number] == list(rep["est"]["n_within"])
    # twice the same, the sums included
    again = eng.error_report(TAUS, bins=128, bin_width=width)
    for side in ("est", "gt"):
        assert (again[side]["sum_d"], again[side]["sum_d2"]) == (rep[side]["sum_d"], rep[side]["sum_d2"])


def test_state_and_bad_parameters(pair):
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import Engine, MapEvalError

    est, gt = pair[0][:3000], pair[1][:3000]
    with Engine(0) as e:
        e.upload(0, est)
        e.upload(1, gt)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            e.nn_error_distribution(0)
        e.nn1(0, 1, fetch=False)
        e.nn1(1, 0, fetch=False)
        assert e.nn_error_distribution(0)["n_used"] == 3000 and e.error_report([0.1])["est"]["n_used"] == 3000
        T = np.eye(4)
        T[0, 3] = 0.125
        e.transform_cloud(0, T)
        for s in (0, 1):  # a transform of either slot drops both results
            with pytest.raises(MapEvalError, match=r"^\[-3\]"):
                e.nn_error_distribution(s)
        e.nn1(0, 1, fetch=False)
        e.nn1(1, 0, fetch=False)
        e.upload(1, gt)
        for s in (0, 1):
            with pytest.raises(MapEvalError, match=r"^\[-3\]"):
                e.nn_error_distribution(s)
        e.nn1(0, 1, fetch=False)
        bad = [dict(quantiles=[1.5]), dict(quantiles=[-0.1]), dict(quantiles=[float("nan")]), dict(quantiles=[0.5] * 17), dict(thresholds=[-0.1]),
               dict(thresholds=[0.1] * 9), dict(bins=4097, bin_width=0.1), dict(bins=-1, bin_width=0.1), dict(bins=10, bin_width=0.0),
               dict(bins=10, bin_width=-1.0), dict(gate_mode=2), dict(gate=float("nan"))]
        for kw in bad:
            with pytest.raises(MapEvalError, match=r"^\[-1\]"):
                e.nn_error_distribution(0, **kw)
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            e.nn_error_distribution(2)
        p, o = _lib.ErrDistParams(), _lib.ErrDistOut()
        p.gate, p.n_bins, p.bin_width = -1.0, 4, 0.1
        assert e._L.me_nn_error_distribution(e._ctx, 0, p, o, 0) == _lib.ME_ERR_ARG  # a histogram without its array
        for field, value in (("n_quantiles", 17), ("n_quantiles", -1), ("n_thresholds", 9), ("n_thresholds", -1)):  # the library's own count checks
            p = _lib.ErrDistParams()
            p.gate = -1.0
            setattr(p, field, value)
            assert e._L.me_nn_error_distribution(e._ctx, 0, p, o, 0) == _lib.ME_ERR_ARG, field
        assert e._L.me_nn_error_distribution(e._ctx, 0, None, o, 0) == _lib.ME_ERR_ARG
        assert e.nn_error_distribution(0, [0.5])["n_used"] == 3000  # the context stays usable
    with Engine(0) as e:  # slab mode: single GPU only
        e.set_slab(0, 0.0, 0.5, 0.1)
        e.upload(0, est)
        e.upload(1, gt)
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            e.nn_error_distribution(0)
