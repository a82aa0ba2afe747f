"""CPU checks of the coarse global registration's numpy model (tests/_globreg_ref.py): pair features on hand-made cases, the vectorised
FPFH against a scalar transcription, the Horn / Jacobi fit against an SVD Kabsch, the Philox sampling, and the C ABI bindings."""
import ctypes as C
import math

import numpy as np
import pytest

import _globreg_ref as G
from _perturb_ref import philox4x64_10


def _pf(p1, n1, p2, n2):
    return G.pair_features(np.array([p1]), np.array([n1]), np.array([p2]), np.array([n2]))[0]


def test_pair_feature_zero_length():
    assert list(_pf((1, 2, 3), (0, 0, 1), (1, 2, 3), (1, 0, 0))) == [0.0, 0.0, 0.0]


def test_pair_feature_parallel_normal_and_offset_gives_zero():
    # d parallel to n1 and |a1| >= |a2|: v = d x n1 = 0
    assert list(_pf((0, 0, 0), (0, 0, 1), (0, 0, 2), (1, 0, 0))) == [0.0, 0.0, 0.0]


def test_pair_feature_plain_branch():
    f = _pf((0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 0, 1))
    # a1 = a2 = 0: no swap, f2 = a1 = 0; v = d x n1 = (0, -1, 0); w = n1 x v = (1, 0, 0); f1 = v.n2 = 0; f0 = atan2(0, 1) = 0
    assert list(f) == [0.0, 0.0, 0.0]
    f = _pf((0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0))
    s = 1 / math.sqrt(2)
    # a1 = 1/sqrt2, a2 = 1/sqrt2: |a1| < |a2| is false -> f2 = a1
    assert f[2] == pytest.approx(s, abs=1e-15)


def test_pair_feature_swap_branch():
    # n1 orthogonal to d, n2 along d: |a1| = 0 < |a2| = 1 -> roles swap, f2 = -a2
    # (with n2 along d, after the swap v = d' x n1' = 0: the whole feature is zero)
    f = _pf((0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 0, 0))
    assert list(f) == [0.0, 0.0, 0.0]
    f = _pf((0, 0, 0), (0, 1, 0), (1, 0, 0), (s := 1 / math.sqrt(2), 0.0, s))
    assert f[2] == pytest.approx(-s, abs=1e-15)
    # the same pair seen from the other side gives the unswapped branch with the same |f2|
    g = _pf((1, 0, 0), (s, 0.0, s), (0, 0, 0), (0, 1, 0))
    assert abs(g[2]) == pytest.approx(s, abs=1e-15)


@pytest.mark.parametrize("axis,off", [(0, 0), (1, 11), (2, 22)])
def test_every_bin_edge(axis, off):
    for b in range(12):
        if axis == 0:
            v = -math.pi + 2 * math.pi * b / 11
        else:
            v = -1.0 + 2.0 * b / 11
        f = np.zeros((3, 3))
        f[:, axis] = [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]
        pos = G.bin_positions(f)[:, axis]
        got = G.bins(f)[:, axis] - off
        want = np.clip(np.floor(pos), 0, 10).astype(int)
        assert list(got) == list(want)
        assert 0 <= got.min() and got.max() <= 10
        assert G.near_edge(f).all()
    # far from every edge
    assert not G.near_edge(np.array([[0.01, 0.05, 0.05]]))[0]
    # the extreme values clamp into [0, 10]
    f = np.array([[math.pi, 1.0, 1.0], [-math.pi, -1.0, -1.0]])
    assert list(G.bins(f)[0]) == [10, 21, 32] and list(G.bins(f)[1]) == [0, 11, 22]


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 2, (n, 3))
    xyz[: n // 3, 2] = 0.0  # a plane, with duplicate-free random points above it
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[: n // 3] = (0, 0, 1)
    xyz[5] = xyz[4]  # one duplicate point (d2 == 0 neighbour, L == 0 pair)
    return xyz, nrm


def test_fpfh_model_against_scalar_loops():
    xyz, nrm = _cloud(300, 3)
    fv, edge, m = G.fpfh(xyz, nrm, radius=0.6, max_nn=20)
    fs = G.fpfh_scalar(xyz, nrm, radius=0.6, max_nn=20)
    ok = ~edge
    assert ok.sum() > 250
    assert np.array_equal(fv[ok], fs[ok])
    assert np.abs(fv - fs).max() < 1e-6 or edge.any()
    assert (m <= 19).all() and (m > 0).all()
    # every block of a point with neighbours sums to 200 (100 from the weighted neighbours, 100 from its own SPFH)
    sums = fv.reshape(-1, 3, 11).sum(axis=2)
    np.testing.assert_allclose(sums, 200.0, rtol=1e-12)


def test_feature_nn_ties_go_to_the_smallest_index():
    R = np.zeros((5, 33))
    R[1] = 1.0
    R[3] = 1.0
    Q = np.ones((2, 33))
    assert list(G.feature_nn(Q, R)) == [1, 1]
    corr, sr, rs = G.match(Q, R, mutual=True)
    assert list(sr) == [1, 1] and rs[1] == 0 and list(corr) == [1, -1]


def test_horn_fit_matches_svd_kabsch():
    rng = np.random.default_rng(11)
    for _ in range(200):
        p = rng.uniform(-20, 20, (3, 3))
        a = rng.normal(size=4)
        a /= np.linalg.norm(a)
        w, x, y, z = a
        R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
        q = p @ R.T + rng.uniform(-50, 50, 3) + rng.normal(scale=0.05, size=(3, 3))
        T = G.horn_fit3(p, q)
        K = G.kabsch_svd(p, q)
        np.testing.assert_allclose(T[:, :3], K[:, :3], atol=1e-12)
        np.testing.assert_allclose(T[:, 3], K[:, 3], atol=1e-12 * 100)


def test_philox_sampling_indices():
    # counter (h, 4, 0, 0): the words are Random123's philox4x64-10; index = high word of w * n
    h = np.arange(4, dtype=np.uint64)
    w = philox4x64_10(h, 4, 0, 0, 7, 0)
    ks = G.samples(7, h, 1000)
    for i in range(4):
        for j in range(3):
            assert ks[i, j] == (int(w[j][i]) * 1000) >> 64
    assert ((ks >= 0) & (ks < 1000)).all()
    # a pure function of (seed, h): the same rows for a sub-range, another seed differs
    assert np.array_equal(G.samples(7, h[2:], 1000), ks[2:])
    assert not np.array_equal(G.samples(8, h, 1000), ks)
    # n = 2^32: w >> 32
    ks32 = G.samples(7, h, 1 << 32)
    assert all(ks32[i, 0] == int(w[0][i]) >> 32 for i in range(4))


def test_ransac_model_on_a_known_transform():
    rng = np.random.default_rng(5)
    cs = rng.uniform(-30, 30, (200, 3))
    ang = 2.0
    R = np.array([[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1]])
    cq = cs @ R.T + np.array([40.0, -12.0, 3.0])
    cq[150:] = rng.uniform(-30, 30, (50, 3))  # 25 % wrong matches
    scores, fits = G.ransac_scores(cs, cq, seed=3, n_hyp=300, eps=0.1)
    assert (scores >= -1).all() and (scores != -1).any()
    best = int(np.argmax(scores))
    assert scores[best] == 150
    np.testing.assert_allclose(fits[best][:, :3], R, atol=1e-9)


def _noisy_correspondences():
    rng = np.random.default_rng(5)
    cs = rng.uniform(-30, 30, (200, 3))
    R = G.rotation(2.0, 0.1, -0.2)
    cq = cs @ R.T + np.array([40.0, -12.0, 3.0]) + rng.normal(scale=0.02, size=cs.shape)
    cq[150:] = rng.uniform(-30, 30, (50, 3))  # 25 % wrong matches
    return cs, cq


@pytest.mark.parametrize("edge_ratio", [0.9, 0.99])
def test_ransac_scores_with_the_checks_at_once_match_the_scalar_form(edge_ratio):
    cs, cq = _noisy_correspondences()
    old_sc, old_fits = G.ransac_scores_scalar(cs, cq, 3, 3000, 0.1, edge_ratio)
    new_sc, new_fits = G.ransac_scores(cs, cq, 3, 3000, 0.1, edge_ratio)
    assert 30 < (old_sc >= 0).sum() < 2900 and len(set(old_sc)) > 3
    assert np.array_equal(new_sc, old_sc) and sorted(new_fits) == sorted(old_fits)
    assert all(np.array_equal(new_fits[h], old_fits[h]) for h in old_fits)
    # any list of hypothesis numbers, in any order: the rows of those hypotheses
    hyps = np.random.default_rng(1).permutation(3000)[:700]
    sub_sc, sub_fits = G.ransac_scores(cs, cq, 3, 0, 0.1, edge_ratio, hyps=hyps)
    assert np.array_equal(sub_sc, old_sc[hyps]) and sorted(sub_fits) == sorted(int(h) for h in hyps[old_sc[hyps] >= 0])
    val, _ = G.ransac_scores(cs, cq, 3, 3000, 0.1, edge_ratio, score=False)
    assert np.array_equal(val >= 0, old_sc >= 0) and set(val) == {-1, 0}
    # hypothesis numbers beyond 2^18 are as good as any
    far = np.array([1 << 18, (1 << 18) + 5, 1 << 40])
    far_sc, _ = G.ransac_scores(cs, cq, 3, 0, 0.1, edge_ratio, hyps=far)
    for t, h in enumerate(far):
        ok, T = G.hypothesis(cs, cq, G.samples(3, np.array([h]), len(cs))[0], 0.1, edge_ratio)
        assert (far_sc[t] >= 0) == ok


def test_sample_checks_against_the_scalar_hypothesis():
    # few correspondences (coinciding samples dominate), collinear ones (every triangle degenerate), edge_ratio 1 on an exact copy
    rng = np.random.default_rng(2)
    cs = np.round(rng.uniform(0, 30, (4, 3)) * 256.0) / 256.0
    cq = cs + np.array([1.0, 2.0, 3.0])
    ks = G.samples(3, np.arange(2000), 4)
    coincide, passes = G.sample_checks(cs, cq, ks, 1.0)
    assert 0.5 < coincide.mean() < 0.8 and np.array_equal(passes, ~coincide)  # 1 - 4 * 3 * 2 / 4^3 = 0.625
    sc, _ = G.ransac_scores(cs, cq, 3, 2000, 0.1, 1.0)
    assert np.array_equal(sc >= 0, passes) and (sc[sc >= 0] == 4).all()
    line = np.column_stack([np.arange(10.0) ** 2, np.zeros(10), np.zeros(10)])
    coincide, passes = G.sample_checks(line, line, G.samples(3, np.arange(500), 10), 0.9)
    assert not passes.any() and not coincide.all()
    assert not any(G.hypothesis(line, line, k, 0.1, 0.9)[0] for k in G.samples(3, np.arange(500), 10))


def test_horn_fit_of_the_identity_and_a_half_turn():
    # the identity: Horn's 4 x 4 matrix is diagonal up to rounding (Jacobi's apq == 0 skip); the half turn about z: a quaternion with w = 0
    rng = np.random.default_rng(12)
    for R, t in ((np.eye(3), np.zeros(3)), (np.diag([-1.0, -1.0, 1.0]), np.array([40.5, -12.25, 3.0]))):
        for _ in range(100):
            p = np.round(rng.uniform(0, 17, (3, 3)) * 256.0) / 256.0
            q = p @ R.T + t
            T = G.horn_fit3(p, q)
            K = G.kabsch_svd(p, q)
            np.testing.assert_allclose(T[:, :3], K[:, :3], atol=1e-12)
            np.testing.assert_allclose(T[:, 3], K[:, 3], atol=1e-12 * 100)
            np.testing.assert_allclose(T[:, :3], R, atol=1e-12)
            assert G.moved_d2(T, p, q).max() < 1e-20


def test_moved_points_is_the_order_of_moved_d2():
    rng = np.random.default_rng(3)
    T, s, q = rng.normal(size=(3, 4)), rng.normal(size=(50, 3)), rng.normal(size=(50, 3))
    d = G.moved_points(T, s) - q
    assert np.array_equal((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], G.moved_d2(T, s, q))


def test_edge_inputs_do_what_their_cases_say():
    """The clouds of test_gpu_globreg_edges.py, on the model alone."""
    P, N = G.three_planes(), G.unit_normals(3000, 7)
    assert len(np.unique(P, axis=0)) == len(P) == 3000
    for (r, k), (cut_lo, cut_hi, m0_lo) in {(1.0, 40): (1, 1, 0), (0.5, 40): (1, 1, 0.05), (1.0, 7): (0.01, 0.1, 0), (0.4, 12): (1, 1, 0.1)}.items():
        idx, d2 = G.knn_lists(P, k)
        F, edge, m = G.fpfh(P, N, r, k, lists=(idx, d2))
        assert edge.mean() <= 0.01 and cut_lo <= (d2[:, -1] >= r * r).mean() <= cut_hi and (m == 0).mean() >= m0_lo
        if (r, k) == (0.4, 12):  # every zero feature matches the first one
            zero = np.flatnonzero(m == 0)
            assert np.array_equal(zero, np.flatnonzero((F == 0).all(axis=1)))
            assert (G.feature_nn(F, F)[zero] == zero[0]).all()
    L = G.lattice_cloud()
    idx, d2 = G.knn_lists(L, 40)
    assert (d2 == 9.0).any(axis=1).mean() > 0.5 and G.fpfh(L, G.unit_normals(len(L), 8), 3.0, 40, lists=(idx, d2))[1].mean() <= 0.01
    D, ND = G.tripled_cloud(200)
    F, edge, m = G.fpfh(D, ND, 1.0, 10)
    assert not edge.any() and np.array_equal(F, G.fpfh_scalar(D, ND, 1.0, 10))
    assert np.array_equal(F[0::3], F[1::3]) and np.array_equal(F[0::3], F[2::3])


def test_shifted_copy_gives_identical_features_and_ties_to_the_lower_half():
    P, N = G.three_planes(), G.unit_normals(3000, 7)
    n = len(P)
    F, edge, _ = G.fpfh(np.concatenate([P, P + np.array([64.0, 0, 0])]), np.concatenate([N, N]), 1.0, 40)
    assert np.array_equal(F[:n], F[n:]) and edge.mean() <= 0.01
    corr, sr, _ = G.match(F, F, mutual=True)
    assert np.array_equal(sr, np.arange(2 * n) % n)
    assert np.array_equal(corr[:n], np.arange(n)) and (corr[n:] == -1).all()


def test_bindings_match_the_header_structs():
    from cloud_map_evaluation_amd import _lib

    assert C.sizeof(_lib.FpfhParams) == 16
    assert C.sizeof(_lib.GlobRegParams) == 16 + 8 + 8 + 8 + 4 + 4 + 8
    assert C.sizeof(_lib.GlobRegInfo) == 6 * 8
    L = _lib.load()
    for s in ("me_voxel_downsample_into", "me_fpfh", "me_fpfh_match", "me_global_register"):
        assert hasattr(L, s) and s in _lib.SYMBOLS
