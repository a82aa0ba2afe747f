"""The robust registration step without a GPU: the bindings against the header, the model's weights at dyadic inputs, the model's
W = (Ct + Cs)^(-1/2) rows against scipy's matrix square root, and the model loop on a map with a 20 % ghost copy, where the Tukey loss
must beat plain least squares (tests/_robust_reg_ref.py is the model the GPU tests judge the device by)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _globreg_ref as G
import _reg_ref as R
import _robust_reg_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Largest deviations measured on the CPU with the inputs of the two tests below (DESIGN.md section 4.17 records them):
W_VS_SQRTM = 2.33e-14  # max |W_model - sqrtm(inv(M))| / max |sqrtm(inv(M))| over eps in {1e-6, 1e-3, 1}
W_ALLOWED = 2 * W_VS_SQRTM


def test_bindings_match_the_header():
    from cloud_map_evaluation_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "mapeval_hip.h")).read()
    assert "me_icp_lsq_sums_robust" in _lib.SYMBOLS and "me_icp_information" in _lib.SYMBOLS
    assert ("int me_icp_lsq_sums_robust(me_ctx *ctx, int query_slot, int mode, double max_distance, int kernel, double k,\n"
            "                           me_icp_robust *out);") in hdr
    assert "int me_icp_information(me_ctx *ctx, int query_slot, double max_distance, double info[36], int64_t *n_corr);" in hdr
    body = hdr[hdr.index("typedef struct me_icp_robust {"):hdr.index("} me_icp_robust;")]
    assert "".join(body.split()) == ("typedefstructme_icp_robust{int64_tn_corr,n_source,n_zero_weight,n_degenerate;"
                                     "doubleJTJ[36],JTr[6],r2,sum_d2,sum_w,sum_wr2;")
    assert [f for f, _ in _lib.IcpRobust._fields_] == ["n_corr", "n_source", "n_zero_weight", "n_degenerate", "JTJ", "JTr", "r2", "sum_d2",
                                                       "sum_w", "sum_wr2"]
    assert C.sizeof(_lib.IcpRobust) == 8 * (4 + 36 + 6 + 4)
    ids = dict(re.findall(r"#define ME_ROBUST_(\w+) (\d)", hdr))
    assert {k.lower(): int(v) for k, v in ids.items()} == _lib.ROBUST_KERNELS
    assert (RR.L2, RR.L1, RR.HUBER, RR.CAUCHY, RR.GM, RR.TUKEY) == tuple(_lib.ROBUST_KERNELS[k] for k in ("l2", "l1", "huber", "cauchy", "gm", "tukey"))
    L = _lib.load()
    assert hasattr(L, "me_icp_lsq_sums_robust") and hasattr(L, "me_icp_information")


def test_weights_at_dyadic_inputs():
    """k = 0.25, |r| in {0, 0.125, 0.25, 0.5}: every operation is exact in fp64 except where a hand value says otherwise"""
    k = 0.25
    r = np.array([0.0, 0.125, 0.25, 0.5])
    for sign in (1.0, -1.0):
        assert np.array_equal(RR.weight(RR.L1, sign * r, k), [0.0, 8.0, 4.0, 2.0])            # 1 / |r|, 0 at r == 0
        assert np.array_equal(RR.weight(RR.HUBER, sign * r, k), [1.0, 1.0, 1.0, 0.5])          # k / max(|r|, k): exactly 1 at |r| <= k
        assert np.array_equal(RR.weight(RR.CAUCHY, sign * r, k), [1.0, 0.8, 0.5, 0.2])         # 1 / (1 + (r/k)^2): 1/1.25, 1/2, 1/5
        assert np.array_equal(RR.weight(RR.TUKEY, sign * r, k), [1.0, 0.5625, 0.0, 0.0])       # (1 - min(1, |r|/k)^2)^2: 0.75^2, 0 at |r| >= k
        gm = RR.weight(RR.GM, sign * r, k)                                                     # k / (k + r^2)^2
        assert np.array_equal(gm, [4.0, 0.25 / (0.265625 * 0.265625), 0.25 / (0.3125 * 0.3125), 1.0])
    assert RR.weight(RR.GM, 0.5, k) == 1.0 and RR.weight(RR.CAUCHY, k, k) == 0.5
    assert np.array_equal(RR.weight(RR.TUKEY, [0.25, 0.3, 1e300], k), [0.0, 0.0, 0.0])
    assert np.array_equal(RR.weight(RR.HUBER, [0.0, 1e-300, 0.25], k), [1.0, 1.0, 1.0])
    assert np.array_equal(RR.weight(RR.HUBER, [0.3, -7.0, 1e200], 1e300), [1.0, 1.0, 1.0])  # (the W path without robustness)
    assert np.array_equal(RR.weight(RR.L2, [0.3, -7.0], k), [1.0, 1.0])


def test_vectorised_jacobi_is_the_scalar_one():
    rng = np.random.default_rng(1)
    A = rng.normal(size=(60, 3, 3))
    A = A @ A.transpose(0, 2, 1)
    A[3] = np.diag([1.0, 2.0, 3.0])   # no sweep
    A[4] = np.eye(3)
    A[5, 0, 1] = A[5, 1, 0] = 0.0     # a skipped rotation
    A[6] = -A[6]                      # negative definite
    d, V = RR.jacobi3(A)
    for i in range(len(A)):
        ds, Vs = G.jacobi_sym(3, A[i].reshape(-1).tolist())
        assert np.array_equal(d[i], ds) and np.array_equal(V[i].reshape(-1), Vs), i
    W, lam, ok = RR.w_matrix(A)
    assert not ok[6] and ok[:6].all() and np.array_equal(W[ok], W[ok].transpose(0, 2, 1))
    bad = np.stack([np.eye(3) * np.nan, np.diag([1.0, 0.0, 1.0]), np.diag([1.0, np.inf, 1.0])])
    assert not RR.w_matrix(bad)[2].any()


def _gicp_pairs(eps, n=400, seed=11):
    rng = np.random.default_rng(seed)
    ns, nt = rng.normal(size=(2, n, 3))
    ns /= np.linalg.norm(ns, axis=1, keepdims=True)
    nt /= np.linalg.norm(nt, axis=1, keepdims=True)
    src = rng.uniform(-20, 20, (n, 3))
    tgt = src + rng.normal(scale=0.05, size=(n, 3))
    return src, tgt, R.gicp_cov(ns, eps), R.gicp_cov(nt, eps)


@pytest.mark.parametrize("eps", [1e-6, 1e-3, 1.0])
def test_model_rows_against_the_matrix_square_root(eps):
    """The three rows W_i [-skew(vs) | I], W_i d with unit weights against scipy.linalg.sqrtm(inv(M)) on k_gicp_cov's output.  The bound is
    twice the largest deviation measured here on the CPU; it belongs to these inputs (400 random normal pairs), not to the method."""
    import scipy.linalg

    src, tgt, cs, ct = _gicp_pairs(eps)
    M = ct + cs
    W, lam, ok = RR.w_matrix(M)
    assert ok.all()
    d = [src[:, a] - tgt[:, a] for a in range(3)]
    WJ, r = RR.gicp_rows(src, d, W)
    worst = 0.0
    for i in range(len(src)):
        Wr = np.real(scipy.linalg.sqrtm(np.linalg.inv(M[i])))
        x, y, z = src[i]
        Jr = Wr @ np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1.0]])
        rr = Wr @ (src[i] - tgt[i])
        sc = np.abs(Wr).max()
        worst = max(worst, np.abs(W[i] - Wr).max() / sc)
        Jm = np.array([[WJ[a][c][i] for c in range(6)] for a in range(3)])
        assert np.abs(Jm - Jr).max() <= W_ALLOWED * sc * 3 * max(1.0, np.abs(src[i]).max())
        assert np.abs(np.array([r[a][i] for a in range(3)]) - rr).max() <= W_ALLOWED * sc * 3 * np.abs(src[i] - tgt[i]).max()
    print(f"eps {eps:g}: max |W - sqrtm(inv(M))| / max |sqrtm(inv(M))| = {worst:.3e}")
    assert worst <= W_ALLOWED


def test_tukey_beats_least_squares_on_a_ghosted_map():
    """Point-to-plane on 100 000 points, 20 % of the map a rigid ghost copy: the Tukey pose error must be far below the L2 one
    (measured here: L2 3.1e-2, Tukey 1.5e-5)."""
    import oracle

    gt, m, pose = RR.outlier_scene()
    n_gt = oracle.estimate_normals_knn(gt, 20)
    l2 = RR.robust_loop(1, RR.L2, 1.0, m, gt, RR.OUTLIER_GATE, tgt_attr=n_gt)
    tk = RR.robust_loop(1, RR.TUKEY, RR.OUTLIER_TUKEY_K, m, gt, RR.OUTLIER_GATE, tgt_attr=n_gt)
    e2, et = RR.pose_error(l2["transformation"], pose), RR.pose_error(tk["transformation"], pose)
    print(f"pose error: L2 {e2:.3e}, Tukey {et:.3e}")
    assert et < e2 / 100
    plain = R.icp_lsq_loop(1, m, gt, RR.OUTLIER_GATE, tgt_attr=n_gt)  # the L2 arm IS the plain model loop
    assert np.abs(plain["transformation"] - l2["transformation"]).max() < 1e-12 and plain["iterations"] == l2["iterations"]


def test_multi_scale_refuses_mismatched_lists():
    from cloud_map_evaluation_amd import icp

    with pytest.raises(ValueError):
        icp.icp_multi_scale(None, [0.4, 0.2, 0.0], [1.0, 0.5], [10, 10, 10], 1)
    with pytest.raises(ValueError):
        icp._kernel_scale("tukey", None)
    assert icp._kernel_scale("l1", None) == 1.0
