"""The coarse global registration (me_globreg.hip) against the numpy model (tests/_globreg_ref.py) at its edges: FPFH where the radius
gate, max_nn, duplicates, d2 == r^2 and tiny or large clouds decide; feature matching with exact ties inside a tile and across grid
columns; RANSAC across the batch boundary, with the re-scoring in several passes, at other edge ratios, with very few correspondences
and for the identity and a half turn.  Every case first asserts on the model that its input exercises the path it names.

Normals are random unit vectors handed over with set_normals (the same ones for copies of a point), so nothing depends on the normal
estimation.  Every comparison is an equality, a bound derived where it stands, or a tolerance test_gpu_globreg.py already uses."""
import math

import numpy as np
import pytest

import _globreg_ref as G

pytestmark = pytest.mark.gpu

CELL = 0.5
MAX_EDGE = 0.01  # the share of points a test may leave to the L1 bar (the model's bin-edge flag)


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _T(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def _device_fpfh(e, slot, xyz, nrm, radius, max_nn, cell=CELL):
    e.upload(slot, xyz, cell_size=cell)
    e.set_normals(slot, nrm)
    F = e.fpfh(slot, radius=radius, max_nn=max_nn)
    assert np.array_equal(e.download(slot), xyz)  # features come in the caller's order
    return F


def _check_fpfh(xyz, nrm, F, radius, max_nn, lists=None, max_edge=MAX_EDGE):
    """test_gpu_globreg._check_fpfh with the parameters open: equality off the model's bin-edge flag, the L1 bar 2 * 100 / m per block
    on it, and the flagged share capped."""
    ref, edge, m = G.fpfh(xyz, nrm, radius=radius, max_nn=max_nn, lists=lists)
    ok = ~edge
    assert edge.mean() <= max_edge, f"{edge.mean():.4f} of the points lie on a bin edge"
    assert F.shape == ref.shape
    assert np.array_equal(F[ok], ref[ok]), f"{np.count_nonzero((F[ok] != ref[ok]).any(1))} points differ off the bin edges"
    if edge.any():
        l1 = np.abs(F[edge] - ref[edge]).reshape(-1, 3, 11).sum(axis=2)
        bar = 2 * 100.0 / np.maximum(m[edge], 1)
        assert (l1 <= bar[:, None] + 1e-9).all()
    return ref, edge, m


@pytest.fixture(scope="module")
def planes():
    xyz = G.three_planes()
    assert 3000 <= len(xyz) <= 6000 and len(np.unique(xyz, axis=0)) == len(xyz)
    assert np.array_equal(xyz * 256.0, np.round(xyz * 256.0))  # dyadic
    return xyz, G.unit_normals(len(xyz), 7)


# ---- A. FPFH ---------------------------------------------------------------------------------------------------------------------------
GRID = [(1.0, 40), (0.5, 40), (1.0, 7), (0.4, 12), (1.0, 1), (1.0, 2), (1.0, 39)]


@pytest.mark.parametrize("radius,max_nn", GRID, ids=[f"r{r}-k{k}" for r, k in GRID])
def test_fpfh_parameter_grid(planes, radius, max_nn):
    xyz, nrm = planes
    with _engine() as e:
        F = _device_fpfh(e, 0, xyz, nrm, radius, max_nn)
    lists = G.knn_lists(xyz, max_nn)
    ref, edge, m = _check_fpfh(xyz, nrm, F, radius, max_nn, lists=lists)
    cut_by_radius = lists[1][:, -1] >= radius * radius  # the last list entry is outside: the radius ends the list, not max_nn
    if (radius, max_nn) in ((0.5, 40), (0.4, 12)):
        assert cut_by_radius.all() and 0.05 < (m == 0).mean() < 0.5
        assert np.array_equal((F == 0.0).all(axis=1), m == 0)
    elif (radius, max_nn) == (1.0, 7):
        assert 0.0 < cut_by_radius.mean() < 0.1 and (m == max_nn - 1).mean() > 0.9
    elif max_nn == 1:
        assert (m == 0).all() and (lists[0][:, 0] == np.arange(len(xyz))).all()
        assert (F == 0.0).all()
    elif max_nn == 2:
        assert (m == 1).mean() > 0.9 and (m <= 1).all()
    else:
        assert cut_by_radius.all() and (m > 0).all() and m.max() < max_nn - 1


def test_fpfh_neighbour_at_exactly_the_radius():
    xyz = G.lattice_cloud(12, 12, 2)
    nrm = G.unit_normals(len(xyz), 8)
    lists = G.knn_lists(xyz, 40)
    on_radius = (lists[1] == 9.0).any(axis=1)
    assert on_radius.mean() > 0.5  # lists that hold an entry at d2 == r^2, which the strict < leaves out
    with _engine() as e:
        F = _device_fpfh(e, 0, xyz, nrm, 3.0, 40)
    ref, edge, m = _check_fpfh(xyz, nrm, F, 3.0, 40, lists=lists)
    # the model with the entries at d2 == 9 let in is another feature for those points: the comparison can tell the two apart
    wrong, _, m2 = G.fpfh(xyz, nrm, radius=np.nextafter(3.0, 4.0), max_nn=40, lists=lists)
    assert (m2[on_radius] > m[on_radius]).all() and (wrong[on_radius] != ref[on_radius]).any(axis=1).all()


def test_fpfh_duplicated_points():
    xyz, nrm = G.tripled_cloud(200)
    lists = G.knn_lists(xyz, 10)
    i = np.arange(len(xyz))
    assert (lists[1][:, :3] == 0.0).all() and (lists[0][i % 3 != 0, 0] != i[i % 3 != 0]).all()  # the query is not the head of its list
    with _engine() as e:
        F = _device_fpfh(e, 0, xyz, nrm, 1.0, 10)
    ref, edge, m = _check_fpfh(xyz, nrm, F, 1.0, 10, lists=lists)
    assert (m >= 2).all()  # the two other copies at d2 == 0: L == 0 pair features, skipped in the weighted sum
    assert np.array_equal(F[0::3], F[1::3]) and np.array_equal(F[0::3], F[2::3])
    assert np.array_equal(ref, G.fpfh_scalar(xyz, nrm, 1.0, 10))


def test_fpfh_fewer_points_than_max_nn():
    rng = np.random.default_rng(4)
    seven = np.round(rng.uniform(0, 2, (7, 3)) * 256.0) / 256.0
    with _engine() as e:
        nrm = G.unit_normals(7, 5)
        F = _device_fpfh(e, 0, seven, nrm, 10.0, 40)
        ref, edge, m = _check_fpfh(seven, nrm, F, 10.0, 40)
        assert (m == 6).all()
        two = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25]])
        F = _device_fpfh(e, 0, two, nrm[:2], 10.0, 40)
        ref, edge, m = _check_fpfh(two, nrm[:2], F, 10.0, 40)
        assert (m == 1).all() and (F != 0.0).any(axis=1).all()
        F = _device_fpfh(e, 0, two, nrm[:2], 1.0, 40)  # |two[1] - two[0]| > 1: no neighbour
        assert F.shape == (2, 33) and (F == 0.0).all()
        F = _device_fpfh(e, 0, two[:1], nrm[:1], 1.0, 40)
        assert F.shape == (1, 33) and (F == 0.0).all()


def test_fpfh_of_a_large_cloud():
    """About 200 000 points as the scene generator gives them (no down-sample): many blocks, i * k and i * 33 far into the buffers.
    The model's lists come from the oracle's exact k-NN, on which the device's k-NN walk is pinned (test_gpu_registration.py)."""
    import oracle
    from cloud_map_evaluation_amd import synth

    xyz = np.ascontiguousarray(synth.campus_scene(200_000, density=50.0, seed=51).numpy())
    n = len(xyz)
    assert 150_000 <= n <= 250_000
    nrm = G.unit_normals(n, 52)
    radius = 0.5  # ~3.5 point spacings at 50 points / m^2
    idx, d2 = oracle.knn(xyz, xyz, 40, threads=16)
    cut_by_radius = d2[:, -1] >= radius * radius
    assert 0.1 < cut_by_radius.mean() < 0.9  # both gates decide, each for a good share of the points
    with _engine() as e:
        F = _device_fpfh(e, 0, xyz, nrm, radius, 40, cell=0.1)
    _check_fpfh(xyz, nrm, F, radius, 40, lists=(idx.astype(np.int64), d2), max_edge=0.001)  # the model flags no point of this cloud


# ---- B. feature ties -------------------------------------------------------------------------------------------------------------------
def _both_slots(e, xyz, nrm, radius, max_nn):
    F0 = _device_fpfh(e, 0, xyz, nrm, radius, max_nn)
    F1 = _device_fpfh(e, 1, xyz, nrm, radius, max_nn)
    assert np.array_equal(F0, F1)
    return F0


def _check_match(e, Fs, Fr, s=0, r=1):
    ref_m, sr, _ = G.match(Fs, Fr, mutual=True)
    corr_a, nc_a = e.fpfh_match(s, r, mutual=False)
    corr_m, nc_m = e.fpfh_match(s, r, mutual=True)
    assert np.array_equal(corr_a, sr) and nc_a == len(sr)
    assert np.array_equal(corr_m, ref_m) and nc_m == int((ref_m >= 0).sum())
    return corr_a, corr_m, nc_m


def test_match_ties_across_grid_columns(planes):
    xyz, nrm = planes
    n = len(xyz)
    both = np.concatenate([xyz, xyz + np.array([64.0, 0.0, 0.0])])
    assert np.array_equal(both[n:] - np.array([64.0, 0.0, 0.0]), xyz)  # the shift is exact
    # k_feat_nn's split of 2n reference rows (the host's formula): the two copies of a row lie in different grid columns
    qb = (2 * n + 255) // 256
    chunks = max(1, min((1024 + qb - 1) // qb, (2 * n + 255) // 256))
    chunk = (2 * n + chunks - 1) // chunks
    assert chunks > 1 and (np.arange(n) // chunk != (np.arange(n) + n) // chunk).all()
    with _engine() as e:
        F = _both_slots(e, both, np.concatenate([nrm, nrm]), 1.0, 40)
        assert np.array_equal(F[:n], F[n:])  # bit-identical halves: every feature has two reference rows at distance 0
        corr_a, corr_m, nc_m = _check_match(e, F, F)
    i = np.arange(2 * n)
    assert np.array_equal(corr_a, i % n)
    assert np.array_equal(corr_m[:n], i[:n]) and (corr_m[n:] == -1).all() and nc_m == n
    _check_fpfh(both, np.concatenate([nrm, nrm]), F, 1.0, 40)


def test_match_ties_inside_a_tile():
    xyz, nrm = G.tripled_cloud(200)
    with _engine() as e:
        F = _both_slots(e, xyz, nrm, 1.0, 10)
        assert np.array_equal(F[0::3], F[1::3]) and np.array_equal(F[0::3], F[2::3])  # equal features at adjacent indices
        corr_a, corr_m, nc_m = _check_match(e, F, F)
    i = np.arange(len(xyz))
    assert (corr_a <= i - i % 3).all() and (corr_a % 3 == 0).all()  # never a later copy


def test_match_of_zero_features(planes):
    xyz, nrm = planes
    with _engine() as e:
        F = _both_slots(e, xyz, nrm, 0.4, 12)
        zero = np.flatnonzero((F == 0.0).all(axis=1))
        assert len(zero) > 0.1 * len(xyz)
        corr_a, _, _ = _check_match(e, F, F)
    assert (corr_a[zero] == zero[0]).all()


@pytest.mark.parametrize("n_src,n_ref", [(4521, 453), (453, 4521)])
def test_match_of_unequal_sizes(n_src, n_ref):
    clouds = {4521: (G.three_planes(1507, 17.0 * math.sqrt(1.507), seed=5), 61), 453: (G.three_planes(151, 17.0 * math.sqrt(0.151), seed=6), 62)}
    for n in (n_src, n_ref):
        assert len(clouds[n][0]) == n and n % 64 != 0 and n % 256 != 0
    with _engine() as e:
        Fs = _device_fpfh(e, 0, clouds[n_src][0], G.unit_normals(n_src, clouds[n_src][1]), 1.0, 40)
        Fr = _device_fpfh(e, 1, clouds[n_ref][0], G.unit_normals(n_ref, clouds[n_ref][1]), 1.0, 40)
        _check_match(e, Fs, Fr)


# ---- C. RANSAC -------------------------------------------------------------------------------------------------------------------------
EPS = 0.15


@pytest.fixture(scope="module")
def pair():
    """The noisy pair of G.ransac_pair on the device; the correspondences are the device's own (fpfh_match), as in test_gpu_globreg.py."""
    src, ns, ref, nr, R0, t0 = G.ransac_pair()
    e = _engine()
    _device_fpfh(e, 0, src, ns, 1.0, 40)
    _device_fpfh(e, 1, ref, nr, 1.0, 40)
    corr, nc = e.fpfh_match(0, 1, mutual=True)
    sel = np.flatnonzero(corr >= 0)
    assert nc == len(sel) >= 100
    yield dict(e=e, src=src, ref=ref, cs=src[sel], cq=ref[corr[sel]], nc=nc)
    e.close()


def _register(e, **kw):
    return e.global_register(0, 1, **dict(dict(max_corr_dist=EPS, validate_top=16, scores=True), **kw))


def test_ransac_across_the_batch_boundary(pair):
    B = 1 << 18
    H = B + 1000 + 37
    assert H > B and (H - B) % 256 != 0
    e, cs, cq = pair["e"], pair["cs"], pair["cq"]
    T, info, sc = _register(e, max_iterations=H, seed=9)
    windows = np.concatenate([np.arange(0, 512), np.arange(B - 512, B + 512), np.arange(H - 512, H)])
    ref_sc, _ = G.ransac_scores(cs, cq, 9, 0, EPS, 0.9, hyps=windows)
    assert (ref_sc[512:1024] >= 0).any() and (ref_sc[1024:] >= 0).any()  # valid hypotheses on both sides of the boundary
    assert np.array_equal(sc[windows], ref_sc)
    valid, _ = G.ransac_scores(cs, cq, 9, H, EPS, 0.9, score=False)
    valid = valid >= 0
    # both batches hold valid hypotheses, and so few that whole blocks of k_ransac_score return against the compacted count
    for a, b in ((0, B), (B, H)):
        assert 0 < valid[a:b].sum() < (b - a) - 256
    assert np.array_equal(sc >= 0, valid)
    assert info["n_valid_hypotheses"] == int(valid.sum()) and info["n_corr"] == pair["nc"]
    assert sc[info["best_hypothesis"]] == info["best_corr_inliers"]
    T2, info2, sc2 = _register(e, max_iterations=H, seed=10)
    ref_sc2, _ = G.ransac_scores(cs, cq, 10, 0, EPS, 0.9, hyps=windows)
    assert np.array_equal(sc2[windows], ref_sc2) and not np.array_equal(ref_sc2, ref_sc)


@pytest.mark.parametrize("noise", [0.0, 0.005], ids=["exact-copy", "noisy-copy"])
def test_rescoring_in_several_passes(noise):
    """validate_top = 64 on ~150 000 source points: 55 + 9 hypotheses in two 1-NN passes.

    The exact rigid copy is the case as it was asked for; on it nearly every candidate reaches fitness 1, so which pass wrote which
    count cannot be told apart there.  The second case adds 5 mm of noise to the copy and gates at 15 mm: the candidates' fitnesses
    then differ by far more than the rounding slack and a count written to the wrong slot changes the winner.

    inlier_rmse: the device and math.fsum (exact) sum the same n non-negative terms; a sum of n such terms in any order is within
    (n - 1) 2^-53 relative of the exact one, and the division and the root add an ulp each: n 2^-52 relative bounds it (derived)."""
    import oracle
    from cloud_map_evaluation_amd import synth

    K, H, seed = 64, 1000, 5
    ref = np.ascontiguousarray(synth.campus_scene(150_000, density=50.0, seed=41).numpy())
    n = len(ref)
    per = min(K, (1 << 23) // n)
    assert per == 55 and K - per == 9  # two passes, the second one short
    nr = G.unit_normals(n, 42)
    R0, t0 = G.rotation(0.7, -0.04, 0.02), np.array([-12.0, 31.0, 1.5])
    base = ref + np.random.default_rng(43).normal(scale=noise, size=ref.shape) if noise else ref
    src = base @ R0.T + t0
    eps = 0.1 if noise == 0.0 else 0.015
    with _engine() as e:
        _device_fpfh(e, 0, src, nr @ R0.T, 0.5, 40, cell=0.1)
        _device_fpfh(e, 1, ref, nr, 0.5, 40, cell=0.1)
        corr, nc = e.fpfh_match(0, 1, mutual=True)
        T, info, sc = e.global_register(0, 1, max_corr_dist=eps, max_iterations=H, validate_top=K, seed=seed, scores=True)
    sel = np.flatnonzero(corr >= 0)
    cs, cq = src[sel], ref[corr[sel]]
    ref_sc, fits = G.ransac_scores(cs, cq, seed, H, eps, 0.9)
    assert np.array_equal(sc, ref_sc)
    valid = np.flatnonzero(ref_sc >= 0)
    assert len(valid) >= K and info["n_valid_hypotheses"] == len(valid) and info["n_corr"] == nc == len(sel)
    top = valid[np.lexsort((valid, -ref_sc[valid]))][:K]
    cand = []
    for h in top:
        _, d2 = oracle.nn1(ref, G.moved_points(fits[h], src), threads=16)
        inl = d2 < eps * eps
        cnt = int(inl.sum())
        cand.append(((-cnt / n, math.sqrt(math.fsum(d2[inl]) / cnt) if cnt else 0.0, int(h)), cnt))
    order = sorted(range(K), key=lambda t: cand[t][0])
    cnts = np.array([c for _, c in cand])
    print(f"noise {noise}: model counts min {cnts.min()} max {cnts.max()} winner rank {order[0]} lead {cnts[order[0]] - np.delete(cnts, order[0]).max()}")
    best_cnt = cand[order[0]][1]
    if noise:
        # the model's winner leads beyond the rounding slack, and it sits in one of the first K - per slots: exactly those a second
        # pass that wrote its counts at offset 0 would overwrite, with counts that are lower by more than the slack
        assert best_cnt - np.delete(cnts, order[0]).max() > 2
        assert order[0] < K - per and (cnts[per:] < best_cnt - 2).all()
    if best_cnt - np.delete(cnts, order[0]).max() > 2:
        assert info["best_hypothesis"] == int(top[order[0]])
    # the returned T_out, re-scored here
    assert info["best_hypothesis"] in set(int(h) for h in top)
    _, d2 = oracle.nn1(ref, G.moved_points(T, src), threads=16)
    inl = d2 < eps * eps
    cnt = int(inl.sum())
    assert info["fitness"] == cnt / n
    assert cnt >= best_cnt - 2  # no candidate beats the winner by more than the rounding slack between the model's T and the device's
    rmse = math.sqrt(math.fsum(d2[inl]) / cnt)
    assert abs(info["inlier_rmse"] - rmse) <= cnt * 2.0 ** -52 * rmse
    assert info["best_corr_inliers"] == ref_sc[info["best_hypothesis"]]
    np.testing.assert_allclose(T[:3, :], fits[info["best_hypothesis"]], atol=1e-12, rtol=0)


@pytest.fixture(scope="module")
def coarse_case():
    """The 3000-hypothesis case of test_gpu_globreg.py::test_ransac_scores_and_winner_match_the_model: 0.5 m down-samples of a scan pair,
    their normals as the device estimated them."""
    from cloud_map_evaluation_amd import synth

    est, gt = synth.scan_pair(300_000, density=2500.0, seed=21)
    T0 = _T(G.rotation(1.9, 0.03, 0.02), [25.0, 14.0, -2.0])
    with _engine() as e:
        out = []
        for s, xyz in ((0, est.numpy()), (1, gt.numpy())):
            e.upload(s, xyz, cell_size=0.1)
            e.voxel_downsample(s, 0.5)
            e.fpfh(s, radius=2.5, max_nn=40, normal_knn=30, fetch=False)
            out.append((e.download(s), e.get_normals(s)))
    (s_xyz, s_n), (r_xyz, r_n) = out
    return s_xyz @ T0[:3, :3].T + T0[:3, 3], s_n @ T0[:3, :3].T, r_xyz, r_n


def test_validate_top_above_the_valid_count(coarse_case):
    src, ns, ref, nr = coarse_case
    with _engine() as e:
        e.upload(0, src, cell_size=0.1)
        e.upload(1, ref, cell_size=0.1)
        e.set_normals(0, ns)
        e.set_normals(1, nr)
        kw = dict(radius=2.5, max_corr_dist=0.75, max_iterations=3000, seed=9, scores=True)
        T16, info16, sc16 = e.global_register(0, 1, validate_top=16, **kw)
        n_valid = info16["n_valid_hypotheses"]
        assert 16 < n_valid < 3000 and n_valid == int((sc16 >= 0).sum())
        Tk, infok, sck = e.global_register(0, 1, validate_top=n_valid, **kw)
        Tm, infom, scm = e.global_register(0, 1, validate_top=10**6, **kw)
    assert np.array_equal(Tm, Tk) and infom == infok and np.array_equal(scm, sck) and np.array_equal(scm, sc16)
    assert infom["fitness"] >= info16["fitness"]  # a superset of the 16 candidates


@pytest.mark.parametrize("edge_ratio", [0.5, 0.99, 1.0])
def test_ransac_edge_ratio(pair, edge_ratio):
    from cloud_map_evaluation_amd.engine import MapEvalError

    H = 3000
    ref_sc, _ = G.ransac_scores(pair["cs"], pair["cq"], 9, H, EPS, edge_ratio)
    if edge_ratio == 1.0:
        assert (ref_sc < 0).all()  # noisy pairs: no triangle has three edges of exactly equal length in both clouds
        with pytest.raises(MapEvalError, match=r"\[-3\].*no valid hypothesis"):
            _register(pair["e"], max_iterations=H, seed=9, edge_ratio=edge_ratio)
        return
    ks = G.samples(9, np.arange(H), len(pair["cs"]))
    passes = G.sample_checks(pair["cs"], pair["cq"], ks, edge_ratio)[1]
    assert (ref_sc >= 0).any() and not np.array_equal(passes, G.sample_checks(pair["cs"], pair["cq"], ks, 0.9)[1])  # the ratio decides
    T, info, sc = _register(pair["e"], max_iterations=H, seed=9, edge_ratio=edge_ratio)
    assert np.array_equal(sc, ref_sc) and info["n_valid_hypotheses"] == int((ref_sc >= 0).sum())


def _few_points(n):
    """n points at least 4 m apart in a 30 m cube, dyadic coordinates."""
    rng = np.random.default_rng(70 + n)
    pts = []
    while len(pts) < n:
        p = np.round(rng.uniform(0, 30, 3) * 256.0) / 256.0
        if all(np.linalg.norm(p - q) >= 4.0 for q in pts):
            pts.append(p)
    return np.array(pts)


def _copy_pair(e, ref, nr, R0, t0, radius):
    """ref and its rigid copy src = R0 ref + t0 on the device with features; the model's matching of the model's features is one to one."""
    src, ns = ref @ R0.T + t0, nr @ R0.T
    Fs, Fr = G.fpfh(src, ns, radius, 40)[0], G.fpfh(ref, nr, radius, 40)[0]
    assert np.array_equal(G.match(Fs, Fr, mutual=True)[0], np.arange(len(ref)))
    _device_fpfh(e, 0, src, ns, radius, 40)
    _device_fpfh(e, 1, ref, nr, radius, 40)
    corr, nc = e.fpfh_match(0, 1, mutual=True)
    assert np.array_equal(corr, np.arange(len(ref))) and nc == len(ref)
    return src


@pytest.mark.parametrize("n", [3, 4, 10])
def test_ransac_with_few_correspondences(n):
    H = 2000
    ref, nr = _few_points(n), G.unit_normals(n, 80 + n)
    R0, t0 = G.rotation(-2.3, 0.4, -0.2), np.array([7.0, -3.0, 11.0])
    with _engine() as e:
        src = _copy_pair(e, ref, nr, R0, t0, 100.0)
        T, info, sc = e.global_register(0, 1, max_corr_dist=0.1, max_iterations=H, validate_top=16, seed=3, scores=True)
    ref_sc, fits = G.ransac_scores(src, ref, 3, H, 0.1, 0.9)
    coincide, _ = G.sample_checks(src, ref, G.samples(3, np.arange(H), n), 0.9)
    assert 0.1 < coincide.mean() < 0.9 and np.array_equal(ref_sc < 0, coincide)  # a copy: only coinciding samples are invalid
    assert np.array_equal(sc, ref_sc)
    assert np.array_equal(sc < 0, coincide) and info["n_valid_hypotheses"] == H - int(coincide.sum()) and info["n_corr"] == n
    assert (sc[sc >= 0] == n).all() and info["best_corr_inliers"] == n and info["fitness"] == 1.0
    np.testing.assert_allclose(T[:3, :], fits[info["best_hypothesis"]], atol=1e-12, rtol=0)


def test_ransac_collinear_correspondences():
    from cloud_map_evaluation_amd.engine import MapEvalError

    H = 2000
    x = np.cumsum([0.0, 4.0, 5.0, 4.5, 6.0, 4.25, 5.5, 7.0, 4.75, 6.5])
    src = np.column_stack([x, np.zeros(10), np.zeros(10)])  # the source triangles are exactly degenerate
    ns = G.unit_normals(10, 90)
    R0, t0 = G.rotation(0.9, 0.2, 0.1), np.array([3.0, 2.0, 1.0])
    ref, nr = src @ R0.T + t0, ns @ R0.T
    ref_sc, _ = G.ransac_scores(src, ref, 3, H, 0.1, 0.9)
    coincide, passes = G.sample_checks(src, ref, G.samples(3, np.arange(H), 10), 0.9)
    assert (ref_sc < 0).all() and not passes.any() and not coincide.all()
    with _engine() as e:
        _device_fpfh(e, 0, src, ns, 100.0, 40)
        _device_fpfh(e, 1, ref, nr, 100.0, 40)
        corr, nc = e.fpfh_match(0, 1, mutual=True)
        assert np.array_equal(corr, np.arange(10))
        with pytest.raises(MapEvalError, match=r"\[-3\].*no valid hypothesis"):
            e.global_register(0, 1, max_corr_dist=0.1, max_iterations=H, seed=3)


MOTIONS = {"identity": (np.eye(3), np.zeros(3)), "half-turn": (np.diag([-1.0, -1.0, 1.0]), np.array([40.5, -12.25, 3.0]))}


@pytest.mark.parametrize("motion", list(MOTIONS))
def test_ransac_special_motions(planes, motion):
    """The true motion is the identity (Horn's matrix is diagonal: Jacobi's apq == 0 skip) or an exact half turn (a quaternion with
    w = 0).  Both map dyadic coordinates exactly, so the two clouds have identical features."""
    H = 3000
    R0, t0 = MOTIONS[motion]
    ref, nr = planes
    src, ns = ref @ R0.T + t0, nr @ R0.T
    assert np.array_equal((src - t0) @ R0, ref)  # exact
    with _engine() as e:
        Fs = _device_fpfh(e, 0, src, ns, 1.0, 40)
        Fr = _device_fpfh(e, 1, ref, nr, 1.0, 40)
        assert np.array_equal(Fs, Fr)
        corr, nc = e.fpfh_match(0, 1, mutual=True)
        T, info, sc = e.global_register(0, 1, max_corr_dist=0.1, max_iterations=H, validate_top=16, seed=6, scores=True)
    sel = np.flatnonzero(corr >= 0)
    assert np.array_equal(corr[sel], sel) and len(sel) > 0.9 * len(ref)
    ref_sc, fits = G.ransac_scores(src[sel], ref[corr[sel]], 6, H, 0.1, 0.9)
    assert (ref_sc >= 0).mean() > 0.9
    assert np.array_equal(sc, ref_sc) and info["n_valid_hypotheses"] == int((ref_sc >= 0).sum())
    assert info["best_corr_inliers"] == ref_sc[info["best_hypothesis"]]
    np.testing.assert_allclose(T[:3, :], fits[info["best_hypothesis"]], atol=1e-12, rtol=0)
