"""k_w2_batch / w2_gaussian (regularize_sigma, jacobi_rot, chol3) on the MI355X against the 50-digit model of tests/_vmd_ref.py, family
by family: e = |W_dev^2 - D| / S within the family's tolerance of _vmd_ref.W2_TOL (8 x the oracle's own measured error, at least 64 u)."""
import numpy as np
import pytest

import _vmd_ref as V

pytestmark = pytest.mark.gpu


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _run(e, f):
    return e.w2_batch(f["mu1"], f["s1"], f["n1"], f["mu2"], f["s2"], f["n2"])


def _check(w, tags):
    """w[j] against the model of element tags[j] = (family, index); -> the largest e / tolerance per family."""
    assert np.isfinite(w).all() and (w >= 0).all()
    worst = {}
    for j, (fam, i) in enumerate(tags):
        d, s, _ = V.w2_model(fam)
        worst[fam] = max(worst.get(fam, 0.0), V.w2_error_units(w[j], d[i], s[i]) * V.U / V.w2_tol(fam))
    return worst


@pytest.mark.parametrize("family", list(V.w2_families()))
def test_family_against_the_model(family):
    f = V.w2_families()[family]
    with _engine() as e:
        w = _run(e, f)
    worst = _check(w, [(family, i) for i in range(len(w))])[family]
    print(f"{family}: {len(w)} inputs, max e = {worst * V.W2_TOL[family][1]:.2f} u of {V.W2_TOL[family][1]:g} u")
    assert worst <= 1.0
    if family == "identical":
        # tr chol(L S L^T) = sum L_ii^2, not tr S: the reference's W of a Gaussian with itself is sqrt(2 sum_{i>j} L_ij^2), zero only
        # where the matrix is diagonal (here: the zero matrices, isotropic after the clamp); there D = 0 by cancellation, and whatever
        # the sign of the rounding W is a tiny non-negative number
        zero = (f["s1"] == 0).all(axis=1)
        assert zero.sum() == 10 and (w[zero] <= 1e-9).all() and (w[~zero] > 1e-3).all()


@pytest.mark.parametrize("count", [1, 255, 256, 257, 2001])
def test_batch_sizes_and_independence_of_the_batch(count):
    f, tags = V.w2_batch(count)
    with _engine() as e:
        w = _run(e, f)
        again = _run(e, f)
        assert w.shape == (count,) and w.tobytes() == again.tobytes()  # two calls: identical bytes
        worst = _check(w, tags)
        assert max(worst.values()) <= 1.0, worst
        if count == 2001:  # the same element alone, and at the block edges of a smaller batch, gives the bytes it gives inside the 2001
            for j in (0, 255, 256, 511, 1024, 2000):
                one = _run(e, {k: v[j:j + 1] for k, v in f.items()})
                assert one.tobytes() == w[j:j + 1].tobytes()
            part = _run(e, {k: v[3:260] for k, v in f.items()})
            assert part.tobytes() == w[3:260].tobytes()


def test_nan_does_not_escape_and_an_indefinite_product_gives_zero_or_a_finite_w():
    """max(0, NaN) = 0 in the reference (std::max(0.0, NaN)) and on the device (fmax): a NaN in mu or in a matrix that is read gives W = 0
    exactly, as the model; the matrix of a voxel of n <= 1 is never read.  After the clamp M = L1 S2 L1^T is positive definite in exact
    arithmetic, so an indefinite M is a product of rounding alone (condition 1e18 here) and the model cannot say which value a double
    computation gets: what is pinned is that W is finite, non-negative and W^2 <= |dmu|^2 + tr S1 + tr S2 (tr chol >= 0 or NaN -> 0)."""
    g = V.w2_families()["generic"]
    f = {k: np.repeat(v[5:6], 8, axis=0).copy() for k, v in g.items()}
    f["mu1"][0, 1] = np.nan
    f["mu2"][1, 2] = np.nan
    f["s1"][2, 4] = np.nan
    f["s2"][3, 0] = np.nan
    f["s1"][4, :] = np.nan
    f["n1"][4] = 1  # not read
    f["s2"][5, 3] = np.nan
    f["n2"][5] = 0  # not read
    rng = np.random.default_rng(3)
    for j in (6, 7):  # eigenvalues 1e12, 1 and 0 under a rotation: the rebuilt matrix is off by 1e-4, far above the clamped 1e-6
        q = V._rot(rng)
        f["s1"][j] = ((q * np.array([1e12, 1.0, 0.0])) @ q.T).reshape(9) * (f["n1"][j] - 1)
    with _engine() as e:
        w = _run(e, f)
    assert np.isfinite(w).all() and (w >= 0).all()
    assert (w[:4] == 0.0).all()
    for j in (4, 5):
        d, s, wm = V.w2_squared(f["mu1"][j], f["s1"][j], int(f["n1"][j]), f["mu2"][j], f["s2"][j], int(f["n2"][j]))
        assert wm > 0 and V.w2_error_units(w[j], d, s) <= V.W2_TOL["small_n"][1]
    for j in (6, 7):
        d, s, wm = V.w2_squared(f["mu1"][j], f["s1"][j], int(f["n1"][j]), f["mu2"][j], f["s2"][j], int(f["n2"][j]))
        print(f"indefinite product {j}: W_dev = {w[j]:.6g}, exact W = {wm:.6g}")
        assert w[j] * w[j] <= float(s) * (1 + 1e-9)


def test_empty_batch_and_bad_arguments():
    from cloud_map_evaluation_amd.engine import MapEvalError

    with _engine() as e:
        z3, z9, zn = np.zeros((0, 3)), np.zeros((0, 9)), np.zeros(0, np.int32)
        assert e.w2_batch(z3, z9, zn, z3, z9, zn).shape == (0,)
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            e._ck(e._L.me_w2_batch(e._ctx, 0, 0, 0, 0, 0, 0, 1, 0))
