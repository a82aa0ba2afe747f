"""The cases of tests/_prep_edge_cases.py hit the edges they claim (every case's own check, on the numpy model alone), and the model
of tests/_prep_ref.py equals the CPU oracle wherever the oracle has an entry: oracle.voxel_downsample, oracle.transform,
oracle.jet_color, oracle.render_distance and oracle.render_entropy, all compared as bit patterns (the entropy colours too: both sides
run the host's log).  The oracle has no entry for the averaged normals, the inlier gate, the index limit or the refusals: there the
model is held against a second, independent few-line statement written out below.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _prep_edge_cases as E  # noqa: E402
import _prep_ref as R  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def oracle():
    import oracle as o

    return o


SMALL = E.all_small_cases()


# ---- every case hits its edge ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SMALL, ids=[c["name"] for c in SMALL])
def test_case_hits_its_edge(c):
    c["check"]()


@pytest.mark.parametrize("n", E.BBOX_SIZES)
def test_bbox_cases_hit_their_edge(n):
    seen = set()
    for where in E.bbox_variants(n):
        E.ds_bbox_case(n, where)["check"]()
        seen.update(where)
    assert seen == ({0, 255, 256, 262143} | ({262144} if n == 262145 else set()))
    # 1024 blocks of 256 threads: index 262 143 is the last of the first trip, index 262 144 the first of block 0's second trip
    assert min(1024, (n + 255) // 256) * 256 == 262144 and (n > 262144) == (262144 in seen)


def test_entropy_tail_case_hits_its_edge():
    E.re_body_case(E.RE_TAIL_N, tail=True)["check"]()


def test_every_cloud_is_shuffled_and_free_of_negative_zero():
    for c in SMALL:
        xyz = c["xyz"]
        assert np.isfinite(xyz).all() and not (np.signbit(xyz) & (xyz == 0)).any(), c["name"]
        if len(xyz) >= 255:
            for d in range(3):  # no axis is in sorted order: the sorted permutation is not the identity
                assert (np.diff(xyz[:, d]) < 0).any() and (np.diff(xyz[:, d]) > 0).any(), c["name"]


# ---- down-sample ------------------------------------------------------------------------------------------------------------------------------
DS = E.ds_small_cases()


@pytest.mark.parametrize("c", DS, ids=[c["name"] for c in DS])
def test_downsample_model_equals_oracle(oracle, c):
    ref = R.downsample(c["xyz"], c["vs"])
    assert _same(ref["points"], oracle.voxel_downsample(c["xyz"], c["vs"]))


def test_downsample_model_equals_oracle_at_the_bbox_sizes(oracle):
    for n in E.BBOX_SIZES:
        c = E.ds_bbox_case(n, E.bbox_variants(n)[-1])
        assert _same(R.downsample(c["xyz"], c["vs"])["points"], oracle.voxel_downsample(c["xyz"], c["vs"]))


def _downsample_by_hand(xyz, vs, normals):
    """The second statement (the oracle averages no normals and knows no index limit): Python floats and a dict, point by point."""
    lo = [min(p[d] for p in xyz) for d in range(3)]
    acc = {}
    for i, p in enumerate(xyz):
        t = []
        for d in range(3):
            f = math.floor((float(p[d]) - (lo[d] - vs * 0.5)) / vs)
            if f < 0 or f > 2097151:
                return None
            t.append(f)
        a = acc.setdefault(tuple(t), [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0])
        for d in range(3):
            a[0][d] = a[0][d] + float(p[d])
            if normals is not None:
                a[1][d] = a[1][d] + float(normals[i][d])
        a[2] += 1
    order = sorted(acc)  # ascending (fx, fy, fz): what the packed key's order must be
    pts = np.array([[s / acc[k][2] for s in acc[k][0]] for k in order])
    nrm = np.array([[s / acc[k][2] for s in acc[k][1]] for k in order])
    return order, pts, nrm


@pytest.mark.parametrize("c", [c for c in DS if len(c["xyz"]) <= 8000], ids=lambda c: c["name"])
def test_downsample_model_equals_the_statement_by_hand(c):
    order, pts, nrm = _downsample_by_hand(c["xyz"], c["vs"], c["normals"])
    ref = R.downsample(c["xyz"], c["vs"], c["normals"])
    assert _same(ref["points"], pts)
    keys = [(fx << 42) | (fy << 21) | fz for fx, fy, fz in order]
    assert keys == sorted(keys) and keys == [int(k) for k in ref["keys"]]  # the key's order is the tuple's order, across the 21-bit fields
    if c["normals"] is not None:
        assert _same(ref["normals"], nrm)
        assert not np.allclose(np.linalg.norm(ref["normals"], axis=1), 1.0)  # averaged, not re-normalised


def test_refusals_of_the_model():
    # (no oracle entry: the oracle truncates the index to int and never refuses)
    for c in E.ds_refused_cases():
        assert R.downsample(c["xyz"], c["vs"]) is R.REFUSED and _downsample_by_hand(c["xyz"], c["vs"], None) is None
    ok = E.ds_key_field_case()
    assert R.downsample(ok["xyz"], 1.0) is not R.REFUSED and _downsample_by_hand(ok["xyz"], 1.0, None) is not None
    for vs in E.BAD_VOXEL_SIZES:
        assert R.downsample(ok["xyz"], vs) is R.REFUSED
    assert math.isnan((1.0 - (0.0 - math.inf * 0.5)) / math.inf)  # vs = inf: the index is inf / inf = NaN, which no comparison accepts


# ---- transform ----------------------------------------------------------------------------------------------------------------------------------
TF = E.tf_cases()


@pytest.mark.parametrize("c", TF, ids=[c["name"] for c in TF])
def test_transform_model_equals_oracle(oracle, c):
    assert _same(R.transform(c["xyz"], c["T"]), oracle.transform(c["xyz"], c["T"]))


def test_transform_identities_and_the_zero_divisor(oracle):
    xyz = E.tf_cloud(257)
    for name, T in E.identities().items():
        assert np.array_equal(T, np.eye(4)), name  # -0.0 == 0.0: the library takes both spellings for the identity
        assert _same(R.transform(xyz, T), xyz), name  # (no coordinate is -0.0, the one value the products could change)
    assert np.signbit(E.identities()["identity_negative_zeros"][0, 1])
    for c in (E.tf_w_zero_case(), E.tf_w_zero_case(all_nan=True)):
        got, want = R.transform(c["xyz"], c["T"]), oracle.transform(c["xyz"], c["T"])
        fin = np.isfinite(want).all(axis=1)
        assert _same(got[fin], want[fin]) and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    # down-sample after the projective transform: the model chains, the oracle chains
    p = [t for t in TF if t["name"] == "transform/proj_x/4097"][0]
    moved = R.transform(p["xyz"], p["T"])
    assert _same(R.downsample(moved, 0.5)["points"], oracle.voxel_downsample(oracle.transform(p["xyz"], p["T"]), 0.5))


# ---- Jet and render_distance ----------------------------------------------------------------------------------------------------------------------
def test_jet_color_model_equals_oracle_on_and_around_every_breakpoint(oracle):
    vals = [-1.0, -0.0, 2.0, math.inf, -math.inf, math.nan]
    for r in np.arange(-2, 11) / 8.0:
        vals += E._nbrs(r)
    got = R.jet_color(np.array(vals))
    for v, g in zip(vals, got):
        assert _same(g, oracle.jet_color(v)), v
    assert (R.jet_color(np.array([math.nan])) == 0.0).all()
    # exactly on a breakpoint the `<=` takes the lower piece: 0.125 -> green's argument is -0.75 -> 0.0, blue's is -0.25 -> 1.0 by interpolation
    assert R.jet_color(np.array([0.125])).tolist() == [[0.0, 0.0, 1.0]]


def test_jet_base_is_continuous_so_either_comparison_gives_the_same_bits():
    """Why no test can tell `<=` from `<` in jet_base: the interpolation meets the plateaus exactly (0.0 at -0.75 and 0.75, 1.0 at
    -0.25 and 0.25, in fp64 without rounding), so the value ON a breakpoint is the same whichever piece takes it."""
    def strict(v):
        return np.select([v < -0.75, v < -0.25, v < 0.25, v < 0.75],
                         [0.0, R._interpolate(v, 0.0, -0.75, 1.0, -0.25), 1.0, R._interpolate(v, 1.0, 0.25, 0.0, 0.75)], default=0.0)
    v = np.array([x for b in R.JET_BREAKS for x in E._nbrs(b)])
    assert _same(strict(v), R.jet_base(v))
    assert R.jet_base(np.array(R.JET_BREAKS)).tolist() == [0.0, 1.0, 1.0, 0.0]
    assert not np.signbit(R.jet_base(np.array(R.JET_BREAKS))).any() and not np.signbit(strict(np.array(R.JET_BREAKS))).any()


RD = E.rd_cases()


@pytest.mark.parametrize("c", RD, ids=[c["name"] for c in RD])
def test_render_distance_model_equals_oracle(oracle, c):
    assert _same(R.render_distance(c["d2"], c["dis"]), oracle.render_distance(c["d2"], c["dis"]))


@pytest.mark.parametrize("c", RD, ids=[c["name"] for c in RD])
def test_inlier_gate_model_equals_the_statement_by_hand(c):
    # (no oracle entry for the gate as a per-point mask)
    for gate, mode in E.GATES:
        want = [True if gate < 0 else (x < gate * gate if mode == 1 else x <= gate) for x in c["d2"].tolist()]
        assert R.inliers(c["d2"], gate, mode).tolist() == want


# ---- render_entropy ------------------------------------------------------------------------------------------------------------------------------
RE = E.re_small_cases()


def _entropy_equals_oracle(oracle, c):
    ref = R.render_entropy(c["xyz"], c["ent"], c["valid"])
    oxyz, orgb, omn, omx = oracle.render_entropy(c["xyz"], c["ent"], c["valid"])
    assert _same(ref["xyz"], oxyz) and ref["n_valid"] == len(oxyz)
    assert _same([ref["min_abs"], ref["max_abs"]], [omn, omx])
    assert _same(ref["rgb"], orgb)


@pytest.mark.parametrize("c", RE, ids=[c["name"] for c in RE])
def test_render_entropy_model_equals_oracle(oracle, c):
    _entropy_equals_oracle(oracle, c)


def test_render_entropy_model_equals_oracle_in_the_tail(oracle):
    _entropy_equals_oracle(oracle, E.re_body_case(E.RE_TAIL_N, tail=True))


def test_exact_mask_marks_only_plateaus_and_nan():
    ne = np.array([math.nan, 0.0, 0.125, 0.125 + 2e-6, 0.25, 0.5, 1.0])
    m = R.jet_exact_mask(ne)
    assert m[0].all()
    assert m[1].tolist() == [True, True, False]        # args -1.5, -1.0, -0.5: blue is on a slope
    assert m[2].tolist() == [True, False, False]       # green and blue ON breakpoints
    assert m[3].tolist() == [True, False, True]        # blue just inside its plateau, green on its slope
    rgb = R.jet_color(ne)
    assert np.isin(rgb[m], (0.0, 1.0)).all()
