"""me_segment_planes / me_plane_fetch / me_plane_keep on the MI355X (csrc/me_plane.hip) against the numpy model (tests/_plane_ref.py).

Scores (every hypothesis, -1 included), winners, labels, counts and the info block are compared EXACTLY: the model restates every
operation of the definition in the library's order.  One block of k_plane_score holds R.TILE = 1024 points (256 lanes x 4 points) and
walks R.HYP_CHUNK = 256 hypotheses in groups of 64; above 2048 tiles a block walks several tiles.  The sizes below sit on both sides
of each of these edges.

The refit is compared within a DERIVED bound (test_refit_within_the_derived_bound)."""
import ctypes as C
import math

import numpy as np
import pytest

import _globreg_ref as G
import _plane_ref as R

pytestmark = pytest.mark.gpu

SIZES = [3, 4, 63, 64, 65, 255, 256, 257, 1023, R.TILE, 1025, 2 * R.TILE - 1, 2 * R.TILE, 2 * R.TILE + 1, 4097]
HYPS = [1, 63, 64, 65, 129, 1000]
U = 2.0 ** -53


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


_scene_cache = {}


def _scene(kind: str) -> np.ndarray:
    """4125+ points of each scene in a fixed shuffled order; a test takes the first N."""
    if kind not in _scene_cache:
        if kind == "planes":
            p = G.three_planes(1400, seed=5)
            p = p[np.random.default_rng(9).permutation(len(p))]
        else:
            p = R.lattice_planes(50, 35, 20, shuffle_seed=4)
        p.setflags(write=False)
        _scene_cache[kind] = p
    return _scene_cache[kind]


def _same(dev, model, refit0: bool = True):
    info, planes, labels, scores = dev
    assert info == model["info"]
    assert np.array_equal(scores, model["scores"])
    assert np.array_equal(labels, model["labels"])
    assert len(planes) == len(model["records"])
    for d, m in zip(planes, model["records"]):
        assert (d["count"], d["h"], d["score"]) == (m["count"], m["h"], m["score"])
        if refit0:
            assert np.array_equal(d["plane"], m["plane"]) and d["refit_degenerate"] == 0


@pytest.mark.parametrize("kind,t", [("planes", 0.05), ("lattice", 0.25)])
@pytest.mark.parametrize("n", SIZES)
def test_scores_winners_and_labels_are_exact(kind, t, n):
    xyz = np.ascontiguousarray(_scene(kind)[:n])
    with _engine() as e:
        e.upload(0, xyz)
        for H in HYPS:
            dev = e.segment_planes(0, t, H, 2, 3, refit=False, seed=H, fetch=True)
            _same(dev, R.segment(xyz, t, H, 2, 3, H))


def test_block_walks_several_tiles():
    """More than 2048 tiles: every block of k_plane_score walks two tiles, the last one a single tile with a one-point tail."""
    n = 2048 * R.TILE + R.TILE + 1
    p = G.three_planes((n + 2) // 3, seed=8)
    xyz = np.ascontiguousarray(p[np.random.default_rng(1).permutation(len(p))][:n])
    with _engine() as e:
        e.upload(0, xyz)
        _same(e.segment_planes(0, 0.05, 5, 1, 3, refit=False, seed=2, fetch=True), R.segment(xyz, 0.05, 5, 1, 3, 2))


def test_several_rounds_sample_the_remaining_list():
    xyz = np.ascontiguousarray(_scene("planes")[:3000])
    model = R.segment(xyz, 0.05, 300, 4, 400, 3)
    # three planes, then a fourth round that draws, scores and ends by min_inliers
    assert model["info"]["n_planes"] == 3 and model["info"]["rounds"] == 4 and 3 <= model["scores"][3].max() < 400
    with _engine() as e:
        e.upload(0, xyz)
        dev = e.segment_planes(0, 0.05, 300, 4, 400, refit=False, seed=3, fetch=True)
        _same(dev, model)
        # the labels and records the slot keeps are those it returned
        planes, labels = e.plane_fetch(0)
        assert np.array_equal(labels, dev[2]) and [p["h"] for p in planes] == [p["h"] for p in dev[1]]


def test_lattice_labelling_and_exact_axes():
    xyz = R.lattice_planes()
    with _engine() as e:
        e.upload(0, xyz)
        for refit in (False, True):
            info, planes, labels, scores = e.segment_planes(0, 0.25, 200, 4, 3, refit=refit, seed=1, fetch=True)
            _same((info, planes, labels, scores), R.segment(xyz, 0.25, 200, 4, 3, 1), refit0=not refit)
            assert np.array_equal(labels, R.lattice_expected_labels(xyz)) and info["n_planes"] == 3 and info["rounds"] == 4
            for r, axis in enumerate((2, 0, 1)):
                want = np.zeros(4)
                want[axis] = 1.0
                assert np.array_equal(planes[r]["plane"], want)  # exact inliers: the refit returns the same exact plane
                assert planes[r]["rms"] == 0.0 and planes[r]["max_abs"] == 0.0 and planes[r]["refit_degenerate"] == 0


def test_ties_at_the_threshold():
    g = R.lattice_planes(12, 2, 2, shuffle_seed=None)
    g = g[g[:, 2] == 0]
    below = np.nextafter(0.25, 0.0)
    at = np.array([[2.5, 3.5, 0.25], [7.5, 1.5, -0.25], [3.5, 8.5, 0.25], [9.5, 9.5, -0.25]])
    under = np.array([[4.5, 9.5, below], [10.5, 6.5, -below], [1.5, 1.5, below], [6.5, 11.5, -below]])
    xyz = np.concatenate([g, at, under])
    xyz = np.ascontiguousarray(xyz[np.random.default_rng(2).permutation(len(xyz))])
    is_at, is_under = np.abs(xyz[:, 2]) == 0.25, np.abs(xyz[:, 2]) == below
    with _engine() as e:
        e.upload(0, xyz)
        for seed in range(4):
            dev = e.segment_planes(0, 0.25, 96, 1, 3, refit=False, seed=seed, fetch=True)
            _same(dev, R.segment(xyz, 0.25, 96, 1, 3, seed))
            assert np.array_equal(dev[1][0]["plane"], [0, 0, 1, 0])
            assert np.all(dev[2][is_at] == -1) and np.all(dev[2][is_under] == 0) and dev[1][0]["count"] == len(g) + 4
            assert dev[1][0]["max_abs"] == below


def test_degenerate_inputs():
    with _engine() as e:
        line = R.collinear(50)
        e.upload(0, line)
        dev = e.segment_planes(0, 0.1, 100, 3, 3, seed=0, fetch=True)  # ME_OK, no plane
        _same(dev, R.segment(line, 0.1, 100, 3, 3, 0))
        assert dev[0]["n_planes"] == 0 and dev[0]["n_valid_hypotheses"] == 0 and np.all(dev[3] == -1) and np.all(dev[2] == -1)
        assert e.segment_plane(0, 0.1, 100)[0] is None

        tri = np.repeat(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, 0.25]]), 20, axis=0)
        tri = np.ascontiguousarray(tri[np.random.default_rng(3).permutation(60)])
        e.upload(0, tri)
        dev = e.segment_planes(0, 0.01, 64, 2, 3, refit=False, seed=1, fetch=True)
        model = R.segment(tri, 0.01, 64, 2, 3, 1)
        _same(dev, model)
        assert dev[0]["n_planes"] == 1 and dev[1][0]["count"] == 60 and dev[0]["rounds"] == 2 and set(np.unique(dev[3][0])) == {-1, 60}

        for n in (1, 2):
            pts = np.array([[0.5, 1.5, 2.5], [3.0, 1.0, 2.0]])[:n].copy()
            e.upload(0, pts)
            dev = e.segment_planes(0, 0.1, 16, 2, 3, seed=0, fetch=True)
            _same(dev, R.segment(pts, 0.1, 16, 2, 3, 0))
            assert dev[0]["n_planes"] == 0 and dev[0]["rounds"] == 1 and np.all(dev[3] == -1)

        # exactly one valid hypothesis out of H (the seed is found with the model)
        one = np.concatenate([R.collinear(40), [[3.0, -2.0, 5.0]]])
        H = 24
        seed = next(s for s in range(4000) if R.hypotheses(one, s, 0, H)[0].sum() == 1)
        e.upload(0, one)
        dev = e.segment_planes(0, 0.05, H, 1, 3, refit=False, seed=seed, fetch=True)
        _same(dev, R.segment(one, 0.05, H, 1, 3, seed))
        assert dev[0]["n_valid_hypotheses"] == 1 and np.count_nonzero(dev[3][0] >= 0) == 1 and dev[0]["n_planes"] == 1


def test_refit_within_the_derived_bound(capsys):
    """Device refit against numpy.linalg.eigh on the covariance formed exactly (R.refit_exact), on the device's own (= the model's)
    inlier set.

    The device accumulates M1 and M2 about o = the winner's p0 with |p - o| <= D.  A sum of k terms, each bounded by D^2 (M2) or D
    (M1), in any order has an error <= (k - 1) u sum|terms| <= k^2 u D^2 (resp. k^2 u D), u = 2^-53; each product adds u D^2 and each
    division a relative u.  Hence |d(M2 / k)| <= (k + 2) u D^2 per entry, |d(M1 / k)| <= (k + 1) u D per component and
    |d((M1 / k)(M1 / k)^T)| <= (2 k + 4) u D^2: every entry of C is within (3 k + 6) u D^2 of the exact one, and the Frobenius norm
    of the 3 x 3 difference within 3 (3 k + 6) u D^2 <= 13 k u D^2 for k >= 5.  The cyclic Jacobi and eigh are both backward
    stable: each returns the exact eigenvectors of a matrix within p u ||C||_F of its input, p a modest constant; ||C||_F <= 3 D^2
    and p <= 32 for either give another 200 u D^2.  So ||dC||_F <= c k u D^2 with c = 13 + 200 / k, and Davis-Kahan bounds the
    angle between the normals: sin(theta) <= 2 ||dC||_F / (l2 - l3), plus 8 u for the length of the device's eigenvector.
    d = -n . cen with cen = o + M1 / k: |d_dev - d_ref| <= 2 sin_bound |cen| + (k D + 8 |cen|) u."""
    xyz = np.ascontiguousarray(_scene("planes")[:3000])
    model = R.segment(xyz, 0.06, 200, 3, 100, 5)
    worst = 0.0
    with _engine() as e:
        e.upload(0, xyz)
        info, planes, labels, scores = e.segment_planes(0, 0.06, 200, 3, 100, refit=True, seed=5, fetch=True)
        _same((info, planes, labels, scores), model, refit0=False)
        assert info["n_planes"] == 3
        for r, (d, m) in enumerate(zip(planes, model["records"])):
            inl = xyz[labels == r]
            k = len(inl)
            assert k == d["count"] and d["refit_degenerate"] == 0
            ref, w, cen = R.refit_exact(inl)
            D = float(np.sqrt(((inl - xyz[m["k0"]]) ** 2).sum(axis=1).max()))
            c = 13.0 + 200.0 / k
            sin_bound = 2.0 * (c * k * U * D * D) / (w[1] - w[0]) + 8 * U
            nd, nr = d["plane"][:3], ref[:3]
            sin_t = float(np.linalg.norm(np.cross(nd, nr)))
            assert float(nd @ nr) > 0 and abs(float(nd @ nd) - 1.0) <= 8 * U  # the sign rule, a unit normal
            cn = float(np.linalg.norm(cen))
            d_bound = 2.0 * sin_bound * cn + (k * D + 8.0 * cn) * U
            d_err = abs(d["plane"][3] - ref[3])
            worst = max(worst, sin_t / sin_bound, d_err / d_bound)
            with capsys.disabled():
                print(f"\n  plane {r}: k={k} sin={sin_t:.3e} bound={sin_bound:.3e}  |dd|={d_err:.3e} bound={d_bound:.3e}")
            assert sin_t <= sin_bound and d_err <= d_bound
            # the residual statistics against math.fsum over the device's own plane: 1e-12 relative
            s = R.residuals(inl, d["plane"])
            assert math.isclose(d["rms"], math.sqrt(math.fsum(s * s) / k), rel_tol=1e-12)
            assert math.isclose(d["mean_abs"], math.fsum(np.abs(s)) / k, rel_tol=1e-12)
            assert d["max_abs"] == float(np.abs(s).max())
            # a least-squares plane fits its inliers no worse than the hypothesis it started from
            assert d["rms"] <= math.sqrt(math.fsum(R.residuals(inl, m["plane"]) ** 2) / k) * (1 + 1e-12)
    with capsys.disabled():
        print(f"  largest error / bound: {worst:.3e}")


def test_refit_degenerate_keeps_the_hypothesis_plane():
    """Four points around every lattice point of a line: the variances across the line are equal (l2 == l3), no normal is defined."""
    x = np.arange(20, dtype=np.float64)
    xyz = np.concatenate([np.column_stack([x, s * np.ones(20), np.zeros(20)]) for s in (1.0, -1.0)]
                         + [np.column_stack([x, np.zeros(20), s * np.ones(20)]) for s in (1.0, -1.0)])
    with _engine() as e:
        e.upload(0, xyz)
        hyp = e.segment_planes(0, 2.0, 64, 1, 3, refit=False, seed=0, fetch=True)
        assert hyp[1][0]["count"] == 80  # every point is within 2 of a plane through three of them that scores best
        info, planes, labels, _ = e.segment_planes(0, 2.0, 64, 1, 3, refit=True, seed=0, fetch=True)
        assert planes[0]["refit_degenerate"] == 1 and np.array_equal(planes[0]["plane"], hyp[1][0]["plane"])
        assert np.array_equal(labels, hyp[2]) and planes[0]["rms"] == hyp[1][0]["rms"]


def test_determinism_and_state():
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import MapEvalError

    xyz = np.ascontiguousarray(_scene("planes")[:2500])
    model = R.segment(xyz, 0.05, 150, 3, 50, 1)
    with _engine() as e, _engine() as e2:
        L, ctx = e._L, e._ctx
        e.upload(0, xyz)
        n64 = C.c_int64(0)
        assert L.me_plane_fetch(ctx, 0, None, 0, C.byref(n64), None) == -3  # ME_ERR_STATE: nothing yet
        with pytest.raises(MapEvalError, match="no plane labels"):
            e.plane_keep(0)
        a = e.segment_planes(0, 0.05, 150, 3, 50, refit=True, seed=1, fetch=True)
        b = e.segment_planes(0, 0.05, 150, 3, 50, refit=True, seed=1, fetch=True)
        assert a[0] == b[0] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        for pa, pb in zip(a[1], b[1]):  # bit-identical, the refit and the residual sums included
            assert pa["plane"].tobytes() == pb["plane"].tobytes() and (pa["rms"], pa["mean_abs"], pa["max_abs"]) == (pb["rms"], pb["mean_abs"], pb["max_abs"])
        _same(a, model, refit0=False)
        other = e.segment_planes(0, 0.05, 150, 3, 50, seed=2, fetch=True)
        assert not np.array_equal(other[3], a[3])  # another seed, other samples
        # segment_plane is segment_planes(max_planes = 1)
        one = e.segment_planes(0, 0.05, 150, 1, 50, seed=1, fetch=True)
        plane, idx = e.segment_plane(0, 0.05, 150, 50, seed=1)
        assert plane.tobytes() == one[1][0]["plane"].tobytes() and np.array_equal(idx, np.flatnonzero(one[2] == 0))
        assert np.array_equal(idx, np.flatnonzero(model["labels"] == 0))
        # capacity
        e.segment_planes(0, 0.05, 150, 3, 50, seed=1)
        rec = (_lib.PlaneRecord * 8)()
        assert L.me_plane_fetch(ctx, 0, C.addressof(rec), 2, C.byref(n64), None) == -4 and n64.value == 3  # ME_ERR_CAPACITY
        assert L.me_plane_fetch(ctx, 0, C.addressof(rec), 3, C.byref(n64), None) == 0
        with pytest.raises(MapEvalError, match="plane must be"):
            e.plane_keep(0, 3)
        # keep + select: exactly the model's points, in cloud order
        info, keep = e.plane_keep(0, 0, invert=True, fetch=True)
        want = model["labels"] != 0
        assert np.array_equal(keep.astype(bool), want) and info["n_kept"] == int(want.sum()) and info["n_in"] == len(xyz)
        assert e.select_kept_into(0, e2, 0) == int(want.sum())
        assert np.array_equal(e2.download(0), xyz[want])
        info, keep = e.plane_keep(0, -1, invert=False, fetch=True)
        want = model["labels"] >= 0
        assert np.array_equal(keep.astype(bool), want)
        assert e.select_kept_into(0, e2, 0) == int(want.sum()) and np.array_equal(e2.download(0), xyz[want])
        # remove_plane: ground removal in place
        assert L.me_plane_fetch(ctx, 0, None, 0, C.byref(n64), None) == 0  # (selecting into another engine leaves the source alone)
        n_kept, rinfo, rplanes = e.remove_plane(0, 0.05, 150, 50, seed=1)
        assert n_kept == int((model["labels"] != 0).sum()) and np.array_equal(e.download(0), xyz[model["labels"] != 0])
        assert L.me_plane_fetch(ctx, 0, None, 0, C.byref(n64), None) == -3  # the selection replaced the cloud
        # a transform and an upload discard the labels
        e.upload(0, xyz)
        e.segment_planes(0, 0.05, 150, 1, 50)
        T = np.eye(4)
        T[0, 3] = 1.0
        e.transform_cloud(0, T)
        assert L.me_plane_fetch(ctx, 0, None, 0, C.byref(n64), None) == -3
        e.segment_planes(0, 0.05, 150, 1, 50)
        assert L.me_plane_fetch(ctx, 0, None, 0, C.byref(n64), None) == 0
        e.upload(0, xyz)
        assert L.me_plane_fetch(ctx, 0, None, 0, C.byref(n64), None) == -3


def test_argument_errors():
    from cloud_map_evaluation_amd import _lib

    xyz = np.ascontiguousarray(_scene("planes")[:500])

    def rc(e, slot=0, t=0.05, H=10, P=1, min_inl=3, refit=1):
        prm = _lib.PlaneParams(t, H, P, refit, min_inl, 0)
        return e._L.me_segment_planes(e._ctx, slot, C.byref(prm), None, None, None, None)

    with _engine() as e:
        assert rc(e) == -3  # nothing uploaded
        e.upload(0, xyz)
        assert rc(e) == 0
        for t in (0.0, -0.1, float("nan"), float("inf")):
            assert rc(e, t=t) == -1, t  # ME_ERR_ARG
        assert rc(e, H=0) == -1 and rc(e, H=-5) == -1
        assert rc(e, P=0) == -1 and rc(e, P=65) == -1 and rc(e, P=64) == 0
        assert rc(e, min_inl=2) == -1
        assert rc(e, refit=2) == -1
        assert rc(e, slot=2) == -1 and rc(e, slot=1) == -3
        assert e._L.me_segment_planes(e._ctx, 0, None, None, None, None, None) == -1
    with _engine() as e:
        e.set_slab(0, float(xyz[:, 0].min()) - 1, float(np.median(xyz[:, 0])), 1.0)  # slab mode is refused
        e.upload(0, xyz)
        assert rc(e) == -1
