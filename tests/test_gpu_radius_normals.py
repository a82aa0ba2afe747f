"""me_radius_normals on the MI355X (csrc/me_localgeom.hip, k_local_geom_normals) against the numpy model (tests/_surface_ref.py).

With B = 8 k 2^-53 r^2 (DESIGN.md section 4.10's bound on the covariance perturbation) every valid point is judged, none excluded:
k and the validity exact (test_gpu_localgeom.py's rule), the stored eigenvalues bit-identical to me_local_geometry's,
| |n| - 1 | <= 8 2^-53, and the Rayleigh quotient n^T C_model n <= l3_model + 4 B.  Where 4 B / (l2 - l3) <= 1e-6 also
|n_dev x n_model| <= 4 B / (l2 - l3); the share of valid points that leg judges is computed on the model alone and asserted."""
import numpy as np
import pytest

import _surface_ref as R

pytestmark = pytest.mark.gpu

MIN_K = 5


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _lg_fetch(e, slot):
    from cloud_map_evaluation_amd.engine import _addr

    n = e.size(slot)
    eig, k, valid = np.empty((n, 3)), np.empty(n, np.int32), np.empty(n, np.uint8)
    e._ck(e._L.me_local_geometry_fetch(e._ctx, slot, _addr(eig), _addr(k), _addr(valid)))
    return eig, k, valid


def _run(xyz, r, min_k=MIN_K, **kw):
    """-> (info, normals, eig, k, valid) of me_radius_normals, and the eigenvalues me_local_geometry stores for the same arguments"""
    with _engine() as e:
        e.upload(0, xyz, cell_size=r)
        info_lg, eig_lg, k_lg, valid_lg = e.local_geometry(0, r, min_k, fetch=True)
        info, nrm = e.radius_normals(0, r, min_k, fetch=True, **kw)
        eig, k, valid = _lg_fetch(e, 0)
    assert eig.tobytes() == eig_lg.tobytes() and np.array_equal(k, k_lg) and np.array_equal(valid, valid_lg)
    assert (info["n"], info["n_valid"], info["sum_k"]) == (info_lg["n"], info_lg["n_valid"], info_lg["sum_k"])
    return info, nrm, eig, k, valid


def _judge(tag, xyz, r, dev, min_k=MIN_K, dk_share=None, invalid=(0.0, 0.0, 0.0)):
    info, nrm, eig, k, valid = dev
    m = R.radius_normals(xyz, r, min_k)
    assert np.array_equal(k, m["k"]), f"{tag}: neighbour counts differ"
    b = R.cov_bound(m["k"], r)
    l1 = np.maximum(m["eig"][:, 2], 0.0)
    excluded = m["have"] & (l1 <= b)
    assert not excluded.any(), f"{tag}: the scene has points whose model l1 is below the bound"
    v = valid.astype(bool)
    assert np.array_equal(v, m["valid"])
    assert info["n"] == len(xyz) and info["n_valid"] == int(v.sum()) and info["sum_k"] == int(k[v].astype(np.int64).sum())
    assert np.all(nrm[~v] == np.asarray(invalid)), f"{tag}: an invalid point's normal"
    if not v.any():
        return m
    n_dev = nrm[v]
    unit = np.abs(R.norm_ld(n_dev) - 1.0).astype(np.float64)
    q = R.rayleigh(m["cov"][v], n_dev)
    l3, l2 = m["eig"][v, 0], m["eig"][v, 1]
    bv = b[v]
    print(f"{tag}: n {len(xyz)} valid {int(v.sum())} k max {int(k.max())}  max||n|-1| {unit.max() / R.EPS:.2f} x 2^-53  "
          f"max (q - l3) / 4B {((q - l3) / (4 * bv)).max():.3e}")
    assert np.all(unit <= 8 * R.EPS)
    assert np.all(q <= l3 + 4 * bv), f"{tag}: {np.count_nonzero(q > l3 + 4 * bv)} points past the Rayleigh bound"
    gap = l2 - l3
    tol = np.full(len(gap), np.inf)
    np.divide(4 * bv, gap, out=tol, where=gap > 0)
    leg = tol <= 1e-6
    share = leg.mean()
    cr = R.cross_norm(n_dev[leg], m["normal"][v][leg])
    print(f"{tag}: Davis-Kahan leg judges {share:.4f} of the valid points, max |n x n_model| / tol "
          f"{(cr / tol[leg]).max() if leg.any() else 0.0:.3e}")
    if dk_share is not None:
        assert share >= dk_share
    assert np.all(cr <= tol[leg])
    return m


def _plane(n, seed, shift=(0.0, 0.0, 0.0), noise=0.004, side=None):
    """a noisy tilted plane of about 1000 points / m^2"""
    rng = np.random.default_rng(seed)
    side = (n / 1000.0) ** 0.5 if side is None else side
    u, w = rng.uniform(0, side, n), rng.uniform(0, side, n)
    a, c = np.array([0.8, 0.0, 0.6]), np.array([0.0, 1.0, 0.0])
    nn = np.cross(a, c)
    p = u[:, None] * a + w[:, None] * c + (noise * rng.standard_normal(n))[:, None] * nn
    return np.ascontiguousarray(p + np.asarray(shift))


def _sphere(n, seed, radius=0.5):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.ascontiguousarray(d * (radius + 0.002 * rng.standard_normal(n))[:, None])


@pytest.mark.parametrize("n", [1, 2, MIN_K, MIN_K + 1, 255, 256, 257, 4097])
def test_sizes(n):
    xyz = _plane(n, 100 + n, side=min(0.3, (n / 1000.0) ** 0.5) if n < 255 else None)
    _judge(f"plane n={n}", xyz, 0.1, _run(xyz, 0.1), dk_share=0.95 if n >= 255 else None)


def test_noisy_tilted_plane_4k():
    xyz = _plane(4096, 1)
    m = _judge("plane 4k", xyz, 0.1, _run(xyz, 0.1), dk_share=0.95)
    assert m["valid"].mean() > 0.95


def test_sphere_shell_4k():
    xyz = _sphere(4096, 2)
    m = _judge("sphere 4k", xyz, 0.1, _run(xyz, 0.1), dk_share=0.95)
    assert m["valid"].mean() > 0.95


def test_plane_far_from_the_origin():
    xyz = _plane(4096, 1, shift=(1000.0, -800.0, 300.0))
    _judge("plane shifted", xyz, 0.1, _run(xyz, 0.1), dk_share=0.95)


def test_exact_sheet():
    rng = np.random.default_rng(3)
    xyz = np.zeros((2048, 3))
    xyz[:, :2] = rng.uniform(0, 1.4, (2048, 2))
    dev = _run(xyz, 0.1)
    _judge("z = 0 sheet", xyz, 0.1, dev, dk_share=0.95)
    v = dev[4].astype(bool)
    assert np.all(dev[2][v, 2] == 0.0)  # l3 = 0: no term of the zz moment is non-zero
    # +-e_z within the bound: |n x e_z| <= 4 B / (l2 - l3) with the model's own l2 (l3 = 0)
    m = R.radius_normals(xyz, 0.1, MIN_K)
    tol = 4 * R.cov_bound(m["k"][v], 0.1) / m["eig"][v, 1]
    assert np.all(np.abs(dev[1][v, 2]) >= 1.0 - 8 * R.EPS) and np.all(np.hypot(dev[1][v, 0], dev[1][v, 1]) <= tol)


def test_collinear_points():
    """valid with l2 = l3 = 0: only the unit norm and the Rayleigh bound apply; on the x axis the covariance is diagonal, Jacobi's V is
    the identity and the tie rule (the lowest column among equal eigenvalues) gives e_y exactly"""
    xyz = np.zeros((300, 3))
    xyz[:, 0] = np.random.default_rng(4).uniform(0, 3.0, 300)
    dev = _run(xyz, 0.1)
    _judge("collinear", xyz, 0.1, dev)
    v = dev[4].astype(bool)
    assert v.any() and np.all(dev[2][v, 1:] == 0.0)
    assert np.all(dev[1][v] == np.array([0.0, 1.0, 0.0]))


def test_radius_boundary():
    """neighbours at d2 == r^2 exactly are excluded, one ulp inside they are included (r = 0.5: r^2 is exact)"""
    r = 0.5
    inside = np.nextafter(r, 0.0)
    core = np.array([[0.0, 0.0, 0.0], [0.1, 0.02, 0.01], [-0.1, 0.03, -0.02], [0.02, 0.1, 0.03], [0.01, -0.1, -0.01], [0.05, 0.05, -0.03]])
    on = np.array([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, 0, -r]])
    just = np.array([[inside, 0, 0], [0, -inside, 0], [0, 0, inside]])
    xyz = np.ascontiguousarray(np.concatenate([core, on, just]))
    assert all(R.neighbours(xyz, 0, r).tolist().count(j) == 0 for j in range(6, 10))
    dev = _run(xyz, r)
    _judge("boundary", xyz, r, dev)
    assert dev[3][0] == 5 + 3  # the five other core points and the three one ulp inside; none of the four on the sphere


def test_coincident_duplicates():
    xyz = _plane(1500, 5)
    xyz = np.ascontiguousarray(np.concatenate([xyz, xyz[:64], xyz[:16]]))  # 64 points twice, 16 of them three times
    dev = _run(xyz, 0.1)
    m = _judge("duplicates", xyz, 0.1, dev, dk_share=0.95)
    assert m["k"][0] == len(R.neighbours(xyz, 0, 0.1)) and 1500 in R.neighbours(xyz, 0, 0.1)


def test_viewpoint_sign():
    xyz = _sphere(4096, 2)
    vp = np.array([0.05, -0.02, 0.03])
    plain = _run(xyz, 0.1)
    dev = _run(xyz, 0.1, viewpoint=vp)
    m = _judge("sphere, viewpoint", xyz, 0.1, dev, dk_share=0.95)
    v = dev[4].astype(bool)
    n, w = dev[1], vp - xyz
    assert np.all(((n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2])[v] >= 0.0)  # the library's own expression
    assert np.all(np.abs(dev[1]) == np.abs(plain[1]))  # the same vector up to its sign, bit for bit
    dots = np.einsum("ij,ij->i", m["normal"], w)
    judged = v & (np.abs(dots) > 1e-6 * np.linalg.norm(w, axis=1))
    assert judged.sum() >= 0.95 * v.sum()
    oriented = m["normal"] * np.sign(dots)[:, None]
    assert np.all(np.einsum("ij,ij->i", oriented[judged], n[judged]) > 0.0)


def test_invalid_z_both_ways():
    xyz = np.ascontiguousarray(np.concatenate([_plane(1200, 6), [[50.0, 50.0, 50.0], [60.0, 0.0, 0.0], [60.01, 0.0, 0.0]]]))
    zero = _run(xyz, 0.1)
    one = _run(xyz, 0.1, invalid_z=True)
    _judge("invalid -> 0", xyz, 0.1, zero, dk_share=0.95)
    _judge("invalid -> e_z", xyz, 0.1, one, dk_share=0.95, invalid=(0.0, 0.0, 1.0))
    v = zero[4].astype(bool)
    assert not v[-3:].any() and zero[1][v].tobytes() == one[1][v].tobytes()


def test_run_to_run_and_fresh_context():
    xyz = _plane(4097, 7)
    with _engine() as e:
        e.upload(0, xyz, cell_size=0.1)
        a = e.radius_normals(0, 0.1, MIN_K, fetch=True)[1].tobytes()
        b = e.radius_normals(0, 0.1, MIN_K, fetch=True)[1].tobytes()
    with _engine() as e:
        e.upload(1, xyz)  # another slot, the automatic cell: the index is rebuilt at the radius level
        c = e.radius_normals(1, 0.1, MIN_K, fetch=True)[1].tobytes()
    assert a == b == c


def test_normals_follow_the_transform_and_feed_point_to_plane_icp():
    gt = _plane(4097, 8)
    est = np.ascontiguousarray(_plane(3000, 9) + [0.0, 0.0, 0.003])
    ang = 0.3
    T = np.eye(4)
    T[:3, :3] = [[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.5, -0.25, 0.125]
    with _engine() as e:
        e.upload(0, est, cell_size=0.1)
        e.upload(1, gt, cell_size=0.1)
        _, n0 = e.radius_normals(1, 0.1, MIN_K, invalid_z=True, fetch=True)
        with pytest.raises(Exception):
            e.get_covariances(1)
        e.nn1(0, 1, fetch=False)
        lsq = e.icp_lsq_sums(0, 1, 0.5)  # ME_ICP_POINT_TO_PLANE
        assert lsq.n_corr == 3000 and np.all(np.isfinite(list(lsq.JTJ))) and lsq.r2 > 0.0
        e.gicp_covariances(1)
        e.transform_cloud(1, T)
        n1 = e.get_normals(1)
    Rm = T[:3, :3]
    want = np.stack([(Rm[r, 0] * n0[:, 0] + Rm[r, 1] * n0[:, 1]) + Rm[r, 2] * n0[:, 2] for r in range(3)], 1)
    assert n1.tobytes() == want.tobytes()


def test_argument_errors():
    from cloud_map_evaluation_amd.engine import MapEvalError

    xyz = _plane(300, 10)
    with _engine() as e:
        e.upload(0, xyz, cell_size=0.1)
        for bad in ({"radius": 0.0}, {"radius": float("nan")}, {"min_k": 1}, {"viewpoint": [0.0, float("inf"), 0.0]}):
            kw = {"radius": 0.1, "min_k": MIN_K, **bad}
            with pytest.raises(MapEvalError):
                e.radius_normals(0, **kw)
