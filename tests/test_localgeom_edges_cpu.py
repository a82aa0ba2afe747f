"""The exact model of tests/_localgeom_edge_cases.py held to _localgeom_ref.brute, and the properties its clouds are built to have:
the nine sums of every neighbourhood are exact (recomputed in exact rational arithmetic), no eigenvalue reaches the clamp as -0.0,
the ties, the interior points, the dyadic totals and the viewpoint's dot == 0 are what the GPU tests take them to be.

brute() is O(n^2) in Python: it judges every cloud of at most a few thousand points whole.  The two clouds of 65537+ points are
judged through cuts that leave the judged neighbourhoods whole: the sheet's smaller sizes are its own first points, and the cluster
cloud's clusters are isolated, so its first 70 clusters alone give their points the same neighbourhoods (asserted)."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _localgeom_edge_cases as E  # noqa: E402
import _localgeom_ref as R  # noqa: E402

BRUTE_MAX = 3000


def _small_clouds():
    """(tag, xyz, r, min_k) of every cloud the GPU tests run that brute() can judge whole"""
    tie, _ = E.tie_lattice()
    out = [("tie r", tie, E.TIE_R, E.TIE_MIN_K), ("tie r+", tie, E.TIE_R_IN, E.TIE_MIN_K)]
    out += [(f"sheet {n} min_k {m}", E.sheet(n), E.SHEET_R, m) for n in E.SIZES if n <= BRUTE_MAX for m in E.SHEET_MIN_KS]
    out += [(f"reuse r={r!r}", E.reuse_lattice(), r, E.REUSE_MIN_K) for r, _ in E.reuse_radii()]
    out += [(f"border isolated={iso}", E.border_lattice(iso), E.BORDER_R, E.BORDER_MIN_K) for iso in (False, True)]
    out += [("view", E.view_sheet(), E.VIEW_R, E.VIEW_MIN_K), ("clusters 70", E.clusters(70), E.CL_R, E.CL_MIN_K)]
    return out


def _all_clouds():
    """(tag, xyz, r): every cloud, the large and the translated ones included, for the exactness of the sums"""
    out = [(t, x, r) for t, x, r, _ in _small_clouds() if "min_k 23" not in t]
    out += [("sheet 65537", E.sheet(65537), E.SHEET_R), ("clusters", E.clusters(), E.CL_R)]
    out += [(f"border far isolated={iso}", E.border_lattice(iso) + E.FAR, E.BORDER_R) for iso in (False, True)]
    return out


@pytest.mark.parametrize("tag,xyz,r,min_k", _small_clouds(), ids=[c[0] for c in _small_clouds()])
def test_model_against_brute(tag, xyz, r, min_k):
    eig, k, valid, raw, _ = E.model(xyz, r, min_k, with_raw=True)
    eig_b, k_b, valid_b = R.brute(xyz, r, min_k)
    assert np.array_equal(k, k_b)
    b = R.eig_bound(k_b, r)
    # validity can only differ where the exact l1 is within the bound of 0: nowhere on these clouds
    assert not np.any((k_b >= min_k) & (eig_b[:, 0] <= b))
    assert np.array_equal(valid.astype(bool), valid_b)
    assert np.all(np.abs(eig - eig_b) <= b[:, None])
    assert np.all(eig[valid == 0] == 0.0)
    assert not np.any((raw == 0.0) & np.signbit(raw))  # fmax(-0.0, 0.0) is the one place the restatement could not pin


def _exact_sums(xyz, r):
    """k and the nine sums in integers: coordinates x 2^5 are integers below 2^53 (asserted), so d and d d^T are integer
    arithmetic; -> (k, Fractions per point as rows of 9)"""
    from scipy.spatial import cKDTree

    scaled = xyz * 32.0
    assert np.all(scaled == np.rint(scaled)) and np.all(np.abs(scaled) < 2.0 ** 52)
    P = scaled.astype(np.int64)
    pairs = cKDTree(xyz).query_pairs(r * (1.0 + 1e-6), output_type="ndarray")
    i = np.concatenate([pairs[:, 0], pairs[:, 1]])
    j = np.concatenate([pairs[:, 1], pairs[:, 0]])
    D = P[j] - P[i]
    d2 = (D * D).sum(1)
    r2 = Fraction(r * r) * 1024  # the kernel's r2 = fl(r * r), exactly, in units of 2^-10
    keep = np.array([Fraction(int(v)) < r2 for v in np.unique(d2)], bool)[np.searchsorted(np.unique(d2), d2)]
    i, D = i[keep], D[keep]
    n = len(xyz)
    k = np.bincount(i, minlength=n)
    cols = [D[:, 0], D[:, 1], D[:, 2], D[:, 0] * D[:, 0], D[:, 0] * D[:, 1], D[:, 0] * D[:, 2], D[:, 1] * D[:, 1],
            D[:, 1] * D[:, 2], D[:, 2] * D[:, 2]]
    S = np.zeros((n, 9), np.int64)
    for c, w in enumerate(cols):
        np.add.at(S[:, c], i, w)
    return k, S


@pytest.mark.parametrize("tag,xyz,r", _all_clouds(), ids=[c[0] for c in _all_clouds()])
def test_the_nine_sums_are_exact(tag, xyz, r):
    """the fp64 sums of moments() equal the rational ones, and so does any other order of summation: every term is a multiple of
    2^-10 and sum |term| < 2^43 * 2^-10"""
    k, s = E.moments(xyz, r)
    k_x, S = _exact_sums(xyz, r)
    assert np.array_equal(k, k_x)
    den = [32] * 3 + [1024] * 6
    rows = np.unique(np.concatenate([S, s], 1), axis=0)  # (a lattice has few distinct neighbourhoods)
    for row in rows:
        for c in range(9):
            assert Fraction(int(row[c]), den[c]) == Fraction(float(row[9 + c])), (tag, c)
    assert k.max() * 1024 * (r * 32 + 1) ** 2 < 2.0 ** 43
    if len(xyz) <= 600:  # the same, neighbour by neighbour in Fractions, with the kernel's own fp64 d = p_j - q
        fx = [[Fraction(float(v)) for v in p] for p in xyz]
        r2 = Fraction(r * r)
        for q in range(len(xyz)):
            acc = [Fraction(0)] * 9
            cnt = 0
            for p in range(len(xyz)):
                d = [fx[p][a] - fx[q][a] for a in range(3)]
                if p == q or d[0] * d[0] + d[1] * d[1] + d[2] * d[2] >= r2:
                    continue
                assert [Fraction(float(xyz[p, a] - xyz[q, a])) for a in range(3)] == d
                cnt += 1
                terms = d + [d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]]
                acc = [x + y for x, y in zip(acc, terms)]
            assert cnt == k[q] and acc == [Fraction(float(v)) for v in s[q]], (tag, q)


def test_ties_at_the_radius():
    xyz, ijk = E.tie_lattice()
    for r, inclusive in ((E.TIE_R, False), (E.TIE_R_IN, True)):
        eig, k, valid = E.model(xyz, r, E.TIE_MIN_K)
        assert np.array_equal(k, E.tie_counts(ijk, inclusive))
        inner = E.tie_interior(ijk)
        assert inner.sum() == 27 and valid[inner].all()
        full = sum(1 for a in range(-5, 6) for b in range(-5, 6) for c in range(-5, 6)
                   if 0 < a * a + b * b + c * c < 25 + inclusive)
        assert np.all(k[inner] == full)
        e = eig[inner]
        assert np.all(e[:, 0] == e[:, 1]) and np.all(e[:, 1] == e[:, 2]) and np.all(e[:, 0] > 0)
        f = E.features(e)
        assert np.all(f[:, 1] == 0.0) and np.all(f[:, 2] == 0.0) and np.all(f[:, 3] == 1.0)
        nrm = E.model_normals(xyz, r, E.TIE_MIN_K)
        assert np.all(nrm[inner] == [1.0, 0.0, 0.0])  # V stays the identity: the lowest-index column
    k_out = E.model(xyz, E.TIE_R, E.TIE_MIN_K)[1]
    k_in = E.model(xyz, E.TIE_R_IN, E.TIE_MIN_K)[1]
    assert np.all(k_in > k_out) and (k_in - k_out)[E.tie_interior(ijk)].max() == 30  # 6 of 5-0-0 and 24 of 3-4-0


def test_min_k_edge_has_points_on_both_sides():
    xyz, _ = E.tie_lattice()
    k = E.model(xyz, E.TIE_R, 2)[1]
    K = int(np.median(k))
    at = k == K
    assert at.sum() > 0 and (k < K).sum() > 0 and (k > K).sum() > 0
    assert E.model(xyz, E.TIE_R, K)[2][at].all()
    eig, _, valid = E.model(xyz, E.TIE_R, K + 1)
    assert not valid[at].any() and not eig[at].any()


def test_sheet_sizes_mix_valid_and_invalid():
    eig, k, valid = E.model(E.sheet(513), E.SHEET_R, 2)
    assert k.max() == 30 and np.all(eig[valid == 1, 2] > 0.0)
    layer = np.arange(513) % 3
    _, k, valid = E.model(E.sheet(513), E.SHEET_R, 23)
    assert not valid[layer != 1].any() and valid[layer == 1].any() and k[layer != 1].max() == 22
    assert [E.model(E.sheet(n), E.SHEET_R, 2)[1].tolist() for n in (1, 2, 3)] == [[0], [1, 1], [2, 2, 2]]
    # a cut of the sheet leaves the points far from the cut their neighbourhoods: the first 513 points of 65537, rows 0 .. 7 of 10
    big = E.model(E.sheet(65537), E.SHEET_R, 23)
    small = E.model(E.sheet(513), E.SHEET_R, 23)
    rows = np.arange(513) // 48
    for a, b in zip(big, small):
        assert np.array_equal(a[:513][rows <= 7], b[rows <= 7])
    assert (65537 + 255) // 256 == 257 and (257 + 255) // 256 == 2  # 257 blocks: the reduction's chunk is 2, the last one ragged


def test_cluster_totals_are_dyadic():
    xyz = E.clusters()
    n = len(xyz)
    assert n == 10 * E.CL_COUNT >= 65537 and (n + 255) // 256 == 257
    eig, k, valid = E.model(xyz, E.CL_R, E.CL_MIN_K)
    sub = E.model(E.clusters(70), E.CL_R, E.CL_MIN_K)  # isolated clusters: the first 70 alone have the same neighbourhoods
    for a, b in zip((eig, k, valid), sub):
        assert np.array_equal(a[:700], b)
    centre = np.zeros(n, bool)
    centre[0::10] = centre[1::10] = True
    assert np.array_equal(valid.astype(bool), centre) and np.all(k[centre] == 9) and np.all(k[~centre] < E.CL_MIN_K)
    _, s = E.moments(xyz, E.CL_R)
    assert not s[centre, :3].any() and not s[centre][:, [4, 5, 7]].any()  # sx = sy = sz = 0, a diagonal covariance
    assert np.all(eig[centre, 0] == 2.0 ** -4)  # l1 = 2 * (16 * 2^-5)^2 / 8
    assert len(np.unique(eig[centre], axis=0)) == len(E.CL_SHAPES)
    f = E.features(eig[centre])
    t = E.totals(eig, k, valid)
    assert t["n_valid"] == 2 * E.CL_COUNT and t["sum_k"] == 18 * E.CL_COUNT
    for c, name in enumerate(E.SUM_FIELDS):
        vals = [Fraction(float(v)) for v in np.unique(f[:, c])]
        if name in E.DYADIC_ROWS:
            # every value is the exact quotient and a multiple of 2^-12 below 1: any order of summation is exact
            assert all(v.denominator <= 4096 and 0 <= v < 1 for v in vals), name
            assert sum(Fraction(float(v)) for v in f[:, c]) == Fraction(t[name]), name
    l = [[Fraction(float(v)) for v in row] for row in np.unique(eig[centre], axis=0)]
    for l1, l2, l3 in l:
        assert l1 == Fraction(1, 16) and l1 >= l2 >= l3 > 0
        tot = l1 + l2 + l3
        assert tot.numerator & (tot.numerator - 1) != 0  # no power of two: the surface variation row is not dyadic
    # the three compare-swaps all have work: the largest entry of the diagonal stands on each axis in turn
    raw = E.model(xyz, E.CL_R, E.CL_MIN_K, with_raw=True)[3][centre]
    assert set(np.argmax(raw, 1).tolist()) == {0, 1, 2} and len({tuple(np.argsort(r_)) for r_ in np.unique(raw, axis=0)}) >= 4


def test_reuse_radii_straddle_the_window():
    c = E.REUSE_C
    cell_h = c * (1.0 + 2.0 ** -20)
    for r, builds in E.reuse_radii():
        want_h = r * (1.0 + 2.0 ** -20)
        assert (cell_h < want_h or cell_h > 1.5 * want_h) == bool(builds), r
        assert cell_h < want_h or cell_h <= 2.0 * want_h  # (a window of factor 2 would keep the last one too: one build fewer)
    ks = [E.model(E.reuse_lattice(), r, E.REUSE_MIN_K)[1].max() for r, _ in E.reuse_radii()]
    assert len(set(ks)) >= 3  # the radii are told apart by k


def test_border_cloud_and_its_translation():
    for iso in (False, True):
        xyz = E.border_lattice(iso)
        far = xyz + E.FAR
        assert np.array_equal(far - E.FAR, xyz)  # the translation is exact
        a = E.model(xyz, E.BORDER_R, E.BORDER_MIN_K)
        b = E.model(far, E.BORDER_R, E.BORDER_MIN_K)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        if iso:
            assert not a[1][-6:].any() and not a[2][-6:].any() and not a[0][-6:].any()
            assert np.array_equal(xyz.min(0), xyz[-6:].min(0)) and np.array_equal(xyz.max(0), xyz[-6:].max(0))
        else:
            assert a[2].all()


def test_viewpoint_dot_is_exactly_zero_on_the_interior():
    xyz = E.view_sheet()
    inner = E.view_interior(xyz)
    plain = E.model_normals(xyz, E.VIEW_R, E.VIEW_MIN_K)
    assert inner.sum() == 128 and np.all(plain[inner] == [0.0, 0.0, 1.0])
    q = np.flatnonzero(inner & (xyz[:, 2] == 0.0))[0]
    for dz, want in ((0.0, 1.0), (1.0 / 16, 1.0), (-1.0 / 16, -1.0)):
        vp = np.array([0.40625, 0.28125, xyz[q, 2] + dz])
        v = vp - xyz
        dot = (plain[:, 0] * v[:, 0] + plain[:, 1] * v[:, 1]) + plain[:, 2] * v[:, 2]
        level = inner & (xyz[:, 2] == xyz[q, 2])
        assert np.all(dot[level] == dz)
        out = E.model_normals(xyz, E.VIEW_R, E.VIEW_MIN_K, viewpoint=vp)
        assert np.all(out[level] == [0.0, 0.0, want])
        assert np.all(np.abs(out) == np.abs(plain))
    assert (E.model_normals(xyz, E.VIEW_R, 22)[:, 2] == 0.0).all()  # k <= 21: nobody is valid at min_k = 22
    assert np.all(E.model_normals(xyz, E.VIEW_R, 22, invalid_z=True) == [0.0, 0.0, 1.0])
