"""The cases of tests/_perturb_edge_cases.py hit the edges they claim, under the numpy model alone (no GPU): the keep patterns come
out as built, the deformation flips flip, every outlier count is the listed one, w one ulp inside the radius is positive and tiny,
the mpmath signs of the region rule agree with the model with nobody left out, and no coordinate is -0.0."""
import math
import os
import sys

import mpmath
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _perturb_edge_cases as E  # noqa: E402
import _perturb_ref as R  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def cases():
    return E.all_cases()


def test_no_negative_zero_and_every_cloud_is_finite_and_distinct(cases):
    for c in cases:
        src = c["src"]
        assert np.isfinite(src).all(), c["name"]
        assert not (np.signbit(src) & (src == 0)).any(), c["name"]
        assert len(np.unique(src, axis=0)) == len(src), c["name"]  # distinct points: a wrong base or slot cannot hide


@pytest.mark.parametrize("n", E.SIZES)
def test_patterns_come_out_as_built(n):
    cs = E.pattern_cases(n)
    built = {c["pattern"].tobytes() for c in cs}
    i = np.arange(n)
    for want in [i >= 0, i < 0, i == 0, i == n - 1, i != 0, i != n - 1, i % 2 == 0, (i // 64) % 2 == 1, (i // 256) % 2 == 0] + \
            [i == lone for lone in (255, 256, 257) if lone < n]:  # (patterns that coincide at a small n are built once)
        assert want.tobytes() in built
    for c in cs:
        want = c["pattern"]
        assert len(want) == n
        assert np.array_equal(c["ref"]["src_index"], np.nonzero(want)[0]), c["name"]
        if c["expect"] is None:
            assert c["ref"]["n_kept"] == 0
        else:
            assert np.array_equal(_bits(c["ref"]["points"]), _bits(c["src"][want])), c["name"]
    # the two ratio assignments of one pattern are complements
    for a, b in zip(cs[::2], cs[1::2]):
        assert np.array_equal(a["pattern"], ~b["pattern"])


def test_pattern_sizes_cover_first_and_last_dropped():
    pats = E.keep_patterns(2049)
    assert not pats["all_but_first"][0] and pats["all_but_first"][1:].all()
    assert not pats["all_but_last"][-1] and pats["all_but_last"][:-1].all()
    assert pats["first"].sum() == 1 and pats["last"].sum() == 1 and pats["last"][-1]
    assert pats["lone_256"].sum() == 1 and pats["lone_256"][256]
    assert np.array_equal(pats["runs_256"][:513], np.r_[np.ones(256, bool), np.zeros(256, bool), True])


def test_region_borders_rest_on_the_mpmath_signs(cases):
    borders = [c for c in cases if c["name"].startswith("border/")]
    assert len(borders) == 4
    for c in borders:
        assert c["left_out"] <= 0, "a border point was left out"
        src, region = c["src"], c["kw"]["region_size"]
        swapped = c["kw"]["sparse_ratio"] == 0.0
        want = ~c["mp_positive"] if swapped else c["mp_positive"]
        assert np.array_equal(c["ref"]["src_index"], np.nonzero(want)[0])
        # the cases that are claimed are there: a product of exactly 0, x == +-k region, survey offsets on either axis and on both
        x, y = src[:, 0], src[:, 1]
        for v in (0.0, region, -region, 2 * region, -2 * region, 3 * region, -3 * region, 4e5 - 3, 4e5, 4e5 + 3):
            sel = (x == v) & (np.abs(y) == region / 2)
            assert sel.sum() == 2 and set(np.sign(y[sel])) == {1.0, -1.0}, v  # a kept and a dropped partner
        for v in (0.0, region, -3 * region, 3e6 - 3, 3e6 + 3):
            assert ((y == v) & (np.abs(x) == region / 2)).sum() == 2, v
        assert ((x >= 4e5 - 3) & (y >= 3e6 - 3)).sum() == 7
        at0 = (x == 0) | (y == 0)
        assert at0.sum() == 4 and not c["mp_positive"][at0].any()  # sin(0) = 0: the product is not > 0, the dense ratio applies
    one = next(c for c in borders if c["kw"]["region_size"] == 1.0)
    # sin(fl(pi)) > 0 > sin(-fl(pi)), at 50 digits as in fp64
    assert E.sine_sign(1.0, 1.0) == 1 and E.sine_sign(-1.0, 1.0) == -1 and E.sine_sign(0.0, 1.0) == 0
    assert math.sin(math.pi) > 0
    # survey-sized: |sin| is about 1e-11 there and its sign is that of the rounding of x / region pi
    a = float(E._arg(4e5 + 1, 1.0))
    assert 0 < abs(mpmath.sin(mpmath.mpf(a))) < 1e-9
    assert len({E.sine_sign(4e5 + k, 1.0) for k in range(-3, 4)} | {E.sine_sign(3e6 + k, 1.0) for k in range(-3, 4)}) == 2
    del one


def test_a_reciprocal_multiply_would_change_survivors():
    """sin(x (pi / region)) in place of sin(x / region pi) changes sides for some point of the region = 0.3 cloud (with region = 1 the
    two expressions are the same operations), so the device test of that cloud tells them apart."""
    cs = {c["kw"]["region_size"]: c for c in E.border_cases() if c["kw"]["sparse_ratio"] == 1.0}
    assert E.reciprocal_multiply_flips(cs[0.3]) >= 10
    assert E.reciprocal_multiply_flips(cs[1.0]) == 0


def test_deform_cases_hit_their_edges(cases):
    d = {c["name"]: c for c in cases if c["name"].startswith("deform/")}
    plain = d["deform/plain"]
    names, pts, c0 = plain["names"], plain["src"], np.array(E.DC)
    dv = pts - c0
    dist = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
    by = dict(zip(names, dist))
    for k in names:
        if k.startswith("at_R"):
            assert by[k] == E.DR, k  # exactly on the sphere, in the kernel's own expression
    assert by["below_R_x"] == E.D_BELOW == E.DR * (1.0 - 2.0 ** -52) < E.DR and by["centre"] == 0.0 and by["half_R_x"] == E.DR / 2
    w = E.w_exact(E.D_BELOW, E.DR)
    assert 0 < w < mpmath.mpf("1e-29")
    out = plain["ref"]["points"]
    for i in plain["copies"]:
        assert np.array_equal(_bits(out[i]), _bits(pts[i])), names[i]
    moved = [i for i in range(len(names)) if i not in plain["copies"] and names[i] != "below_R_x"]
    assert all(np.any(out[i] != pts[i]) for i in moved) and len(moved) == 3
    i = names.index("below_R_x")  # moved by at most |strength| w: nothing an fp64 coordinate of this size can show
    assert np.max(np.abs(out[i] - pts[i])) <= 0.3 * float(w) + 2 * np.spacing(4.0)
    # -strength mirrors the move; R = inf moves every point but the centre by exactly strength along its direction (w = 1)
    neg = d["deform/negative"]["ref"]["points"]
    np.testing.assert_allclose(neg - pts, -(out - pts), rtol=0, atol=1e-15)
    inf = d["deform/inf_R"]["ref"]["points"]
    far = [i for i, k in enumerate(names) if k != "centre"]
    np.testing.assert_allclose(np.linalg.norm(inf[far] - pts[far], axis=1), 0.3, rtol=0, atol=1e-15)
    assert np.array_equal(_bits(inf[names.index("centre")]), _bits(c0))
    assert np.array_equal(_bits(d["deform/nan_R"]["ref"]["points"]), _bits(pts))


def test_deform_flips_flip(cases):
    d = {c["name"]: c for c in cases if c["name"].startswith("deform/flip/")}
    for tag, before, after in (("kept_to_dropped", True, False), ("dropped_to_kept", False, True)):
        c = d[f"deform/flip/{tag}"]
        kw = c["kw"]
        density = dict(sparse_ratio=kw["sparse_ratio"], dense_ratio=kw["dense_ratio"], region_size=kw["region_size"], seed=kw["seed"])
        undeformed = set(R.perturb(c["src"], **density)["src_index"])
        deformed = set(c["ref"]["src_index"])
        assert (1 in undeformed) == before and (1 in deformed) == after, tag
        assert undeformed - {1} == deformed - {1} == {2}  # the bystanders: one dropped, one kept, neither moved
        if after:
            assert np.any(c["ref"]["points"][0] != c["src"][1])  # the survivor is the deformed point


def test_outlier_counts_are_the_listed_ones(cases):
    d = [c for c in cases if c["name"].startswith("outliers/")]
    assert len(d) == len(E.OUTLIER_COUNTS) + 3
    assert 100 * 0.29 == 28.999999999999996 and 100 * 0.57 < 57 and 10 * 0.7 == 7.0
    for c in d:
        ref, kw = c["ref"], c["kw"]
        m = len(ref["bases"])
        if c["m"] is not None:
            assert m == c["m"], c["name"]
        assert len(ref["points"]) == ref["n_kept"] + m
        if kw["outlier_range"] == 0.0 and m:
            kept = ref["points"][:ref["n_kept"]]
            assert np.array_equal(_bits(ref["points"][ref["n_kept"]:]), _bits(kept[ref["bases"]])), c["name"]
            assert np.array_equal(ref["bases"], R.outlier_bases(ref["n_kept"], m, kw["seed"]))
    assert [len(c["ref"]["bases"]) for c in d[:len(E.OUTLIER_COUNTS)]] == [28, 56, 7, 1, 1, 0, 257, 204]
    on = next(c for c in d if c["name"] == "outliers/density_on")
    assert 0 < on["ref"]["n_kept"] < len(on["src"]) and len(on["ref"]["bases"]) == int(on["ref"]["n_kept"] * 0.3) > 0
    assert len(np.unique(on["ref"]["bases"])) > 100
    nb = next(c for c in d if c["name"] == "outliers/noised_base")
    assert np.all(nb["ref"]["points"][:257] != nb["src"])  # every coordinate is noised


def test_seed_cases_tell_the_words_of_the_key_apart(cases):
    d = {c["kw"]["seed"]: c["ref"]["src_index"] for c in cases if c["name"].startswith("seed/")}
    assert set(d) == set(E.SEEDS) and (1 << 64) - 1 in d and 1 << 63 in d
    sets = [tuple(v) for v in d.values()]
    assert len(set(sets)) == len(sets)  # six seeds, six survivor sets: no two differ only in bits the key drops
    for v in d.values():
        assert 1800 < len(v) < 2300  # about half of 4097
    # the survivors a 32-bit key would give: what a truncated seed computes is somebody else's set
    assert np.array_equal(R.perturb(next(c for c in cases if c["name"] == "seed/7")["src"], sparse_ratio=0.5, dense_ratio=0.5,
                                    region_size=E.BIG_REGION, seed=((1 << 32) + 7) & 0xFFFFFFFF)["src_index"], d[7])


def test_philox_key_with_bits_above_2_32():
    """the numpy model against numpy's own Philox for keys with high bits in either word (the device is compared with the model)"""
    M64 = (1 << 64) - 1
    for k0, k1 in (((1 << 32) + 7, 0), (1 << 63, 0), (M64, 0), (0xDEADBEEF00000001, 1 << 40)):
        g = np.random.Philox(counter=np.array([4, 1, 0, 0], dtype=np.uint64), key=k0 | (k1 << 64))  # first block: counter + 1
        want = g.random_raw(4 * 64).reshape(64, 4)
        mine = R.philox4x64_10(np.arange(5, 69, dtype=np.uint64), 1, 0, 0, k0, k1)
        assert np.array_equal(np.stack(mine, axis=1), want)
