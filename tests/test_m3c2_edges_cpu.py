"""The generators of tests/_m3c2_edge_cases.py against the model of tests/_m3c2_ref.py alone (no GPU): every case has the property it
was built for, so that tests/test_gpu_m3c2_edges.py cannot pass vacuously."""
import math

import numpy as np

import _m3c2_edge_cases as E
import _m3c2_ref as R


def test_fp64_model_agrees_with_the_exact_model_where_the_sums_are_exact():
    """m3c2_fp64 on a dyadic lattice against m3c2 (exact fractions, one rounding): the same sets, and values within the bounds of
    DESIGN.md section 4.15; where S_own == 0 and n divides S_other the distance is the same number"""
    pts = np.array([(i / 8, j / 8, k / 8) for i in range(-3, 4) for j in range(-3, 4) for k in range(-2, 3)], np.float64)
    other = pts + [0.0, 0.0, 1 / 16]
    nrm = np.tile([0.0, 0.0, 1.0], (len(pts), 1))
    a, b = R.m3c2(pts, other, nrm, 3 / 8, 2 / 8, 3, 0.001), R.m3c2_fp64(pts, other, nrm, 3 / 8, 2 / 8, 3, 0.001)
    for k in ("n_own", "n_other", "valid"):
        assert np.array_equal(a[k], b[k]), k
    v = a["valid"]
    assert v.sum() > 100 and b["order_free"][v].all()
    n = (a["n_own"] + a["n_other"])[v]
    assert (np.abs(a["dist"][v] - b["dist"][v]) <= n * E.U * 0.25).all()
    for key, cnt in (("var_own", a["n_own"][v]), ("var_other", a["n_other"][v])):
        assert (np.abs(a[key][v] - b[key][v]) <= (3 * cnt + 10) * E.U * 0.25 * 0.25).all(), key
    assert not R.order_free(np.array([0.1, 0.2, 0.3])) and R.order_free(np.array([0.1, 0.1, 0.1])) and R.order_free(np.array([0.25, -3 / 64]))


def test_frame_restates_the_index():
    f = E.frame(np.array([[0.3, -0.2, 0.1], [1.3, 0.4, 0.2]]), 0.25)
    assert f.cell_h == 0.25 * (1 + 2.0 ** -20) and np.array_equal(f.origin, np.array([1.0, -1.0, 0.0]) * f.cell_h)
    assert f.ncell == 5.0 and f.bits == 3 and f.cell_lim == 8 and f.builds and f.fine_h == math.ldexp(f.cell_h, -18)
    assert np.array_equal(f.cells([[0.3, -0.2, 0.1], [1.3, 0.4, 0.2], [-0.3, 5.0, 0.0]]), [[0, 0, 0], [4, 2, 0], [-3, 20, 0]])
    assert not E.frame(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), 1e-7).builds
    assert E.frame(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), 5e-4).builds


def test_a_more_core_points_than_one_round_and_four_equal_maxima():
    c = E.case_a()
    m, n, slots = c["model"], c["n"], c["slots"]
    assert n == len(c["own"]) == 256 * E.BLOCKS + 257 > 256 * E.BLOCKS
    assert 1400 < int(c["mask"].sum()) < 1600 and 3000 < len(c["other"]) < 5000
    assert {0, n - 1} <= set(slots.tolist()) and m["valid"][slots].all()
    d = m["dist"][slots]
    assert np.array_equal(np.abs(d).view(np.uint64), np.full(4, 1.0).view(np.uint64))  # bit-equal
    assert (d < 0).sum() == 2 and d[np.argmin(slots)] < 0
    rest = m["valid"].copy()
    rest[slots] = False
    assert rest.sum() > 1000 and np.abs(m["dist"][rest]).max() < 1.0  # nobody else reaches them
    assert m["order_free"].all() and (m["var_other"][rest] > 0).any() and m["significant"][rest].any() and not m["significant"][rest].all()
    assert (c["mask"] != 0).sum() > m["valid"].sum()  # (some core points are invalid too)


def test_b_the_other_cloud_fills_its_frame_and_core_points_sit_in_every_border_cell():
    c = E.case_b()
    f, m = E.frame(c["other"], E.RB), c["model"]
    lim = f.cell_lim
    assert f.builds and f.ncell == lim == 4 and np.array_equal(f.origin, np.zeros(3))
    oc = f.cells(c["other"])
    for a in range(3):
        assert set(np.unique(oc[:, a]).tolist()) == {0.0, 1.0, 2.0, 3.0}  # cells 0 and cell_lim - 1 are populated
    cells = f.cells(c["own"])
    near = ((cells == -1) | (cells == lim)).any(axis=1) & ((cells >= -1) & (cells <= lim)).all(axis=1)
    out = ((cells <= -2) | (cells >= lim + 1)).any(axis=1)
    assert near.sum() > 500 and out.sum() > 500 and (~near & ~out).sum() > 50
    for a in range(3):  # every border cell on every axis, served (n_other > 0) and not
        for edge in (-1, lim):
            sel = near & (cells[:, a] == edge)
            assert (m["n_other"][sel] > 0).sum() > 10, (a, edge)
        for edge in (-2, lim + 1):
            assert (cells[:, a] == edge).sum() > 50
    corner = ((cells == -1) | (cells == lim)).all(axis=1)
    assert (m["n_other"][corner] > 0).sum() >= 8  # every corner cell of the frame serves a core point diagonally outside it
    assert (m["n_other"][out] == 0).all() and not m["valid"][out].any()
    assert m["valid"][near].any() and m["valid"][~near & ~out].any()
    ulp = cells[c["n_product"]:c["n_product"] + c["n_ulp"]].reshape(3, 2, 3, 3)  # axis, boundary, the three points, xyz
    for a in range(3):
        assert set(ulp[a, 0, :, a].tolist()) == {-2.0, -1.0} and set(ulp[a, 1, :, a].tolist()) == {float(lim), float(lim + 1)}
    far = c["far"]
    fo = E.frame(c["own"], E.RB)
    assert fo.builds and fo.bits == E.MORTON_BITS and cells[far, 0] > 2.0 ** 20 - 8
    assert m["n_own"][far] == 1 and m["n_other"][far] == 0 and not m["valid"][far]


def test_c_no_two_core_points_share_a_neighbourhood_of_cells():
    c = E.case_c()
    f, fo = E.frame(c["other"], E.RB), E.frame(c["own"], E.RB)
    for own, sel in ((c["own"], c["mask"] != 0), (c["lone"], np.ones(len(c["lone"]), bool))):
        cells = f.cells(own[sel])
        assert len(cells) == 144 >= 130
        apart = np.abs(cells[:, None, :] - cells[None, :, :]).max(axis=2)
        assert (apart[~np.eye(len(cells), dtype=bool)] > 2).all()
    assert not np.array_equal(f.origin, fo.origin)  # the frames' origins differ ...
    shift = (fo.lo - f.lo) / f.cell_h
    assert (shift != np.rint(shift)).all()  # ... and bbox_lo by no multiple of the cell edge
    m = c["model"]
    core = c["mask"] != 0
    assert m["valid"][core].all() and (m["n_own"][core] == 3).all() and (m["n_other"][core] == 5).all() and m["order_free"].all()
    assert len(np.unique(m["dist"][core])) >= 7 and (m["dist"][core] < 0).any() and (m["dist"][core] > 0).any()
    assert (m["n_own"][~core] == 0).all()
    lm = c["lone_model"]
    assert (lm["n_own"] == 1).all() and (lm["n_other"] == 5).all() and not lm["valid"].any()


def test_d_runs_per_cell_and_duplicates():
    c = E.case_d()
    f, m = E.frame(c["other"], E.RB), c["model"]
    assert f.builds and np.array_equal(f.origin, np.zeros(3))
    _, runs = np.unique(f.cells(c["other"]), axis=0, return_counts=True)
    assert sorted(runs.tolist()) == [1] + list(E.D_RUNS)
    bounds = np.cumsum((1,) + E.D_RUNS)
    clusters = [c["other"][bounds[k]:bounds[k + 1]] for k in range(len(E.D_RUNS))]
    for k, pts in enumerate(clusters):
        for other_pts in clusters[k + 1:]:
            d = np.sqrt(((pts[:, None, :] - other_pts[None, :, :]) ** 2).sum(axis=2))
            assert d.min() > 3 * E.RB
    _, own_runs = np.unique(E.frame(c["own"], E.RB).cells(c["own"]), axis=0, return_counts=True)
    assert sorted(own_runs.tolist()) == [5, 5, 5, 5, 5, E.D_DUPLICATES]
    start = 0
    for k, run in enumerate(E.D_RUNS):
        copies = E.D_DUPLICATES if run == 129 else 5
        sel = slice(start, start + copies)
        assert (np.sqrt(((clusters[k][:, None, :] - c["own"][None, sel, :]) ** 2).sum(axis=2)) < E.RB).all()  # nearer than R
        assert (m["n_other"][sel] == run).all() and (m["n_own"][sel] == copies).all() and m["valid"][sel].all()
        assert (m["var_own"][sel] == 0).all()
        start += copies
    assert m["order_free"].all() and (m["var_other"] > 0).sum() >= E.D_DUPLICATES and m["n_own"].max() >= 200


def test_e_counts_only_m_m_is_valid():
    c = E.case_e_counts()
    for mp in E.E_MINS:
        m = c["models"][mp]
        group = c["combos"][:, 0] == mp
        a, b = c["combos"][:, 1], c["combos"][:, 2]
        assert np.array_equal(m["n_own"], a) and np.array_equal(m["n_other"], b)
        assert {(int(x), int(y)) for x, y in zip(a[group], b[group])} == {(mp - 1, mp - 1), (mp - 1, mp), (mp, mp - 1), (mp, mp)}
        assert np.array_equal(m["valid"][group], (a[group] == mp) & (b[group] == mp))
        v = m["valid"]
        assert (m["dist"][v] == E.E_DIST).all() and (m["var_own"][v] == 0).all() and (m["var_other"][v] == 0).all() and m["order_free"].all()
        assert (m["dist"][~v] == 0).all() and (m["lod"][~v] == 0).all()


def test_e_lod_at_below_and_above_the_distance():
    below, equal, above = E.lod_triple()
    assert below is not None and above is not None and below < above
    assert E.lod_of(below) < E.E_DIST < E.lod_of(above)
    assert np.nextafter(E.lod_of(below), math.inf) >= E.E_DIST or equal is not None
    assert equal is not None and E.lod_of(equal) == E.E_DIST  # (equality is met for dist = 1/16: the device test runs all three)
    assert not (E.E_DIST > E.lod_of(equal)) and E.E_DIST > E.lod_of(below) and not (E.E_DIST > E.lod_of(above))


def test_e_raw_variances_of_both_signs_exist():
    neg, pos = E.variance_pairs()
    assert len(neg) == 3 and len(pos) == 3
    for n, c in neg:
        assert E.identical_t_raw(n, c) < 0.0
    for n, c in pos:
        assert E.identical_t_raw(n, c) > 0.0
    case = E.case_e_variance()
    m = case["model"]
    assert m["valid"].all() and m["order_free"].all()
    for i, (n, c, negative) in enumerate(case["kind"]):
        assert m["n_other"][i] == n and m["raw_other"][i] == E.identical_t_raw(n, c)
        assert (m["raw_other"][i] < 0) == negative and m["var_other"][i] == (0.0 if negative else m["raw_other"][i])
        assert not np.signbit(m["var_other"][i])


def test_f_the_refused_radii_are_refused_by_the_frame_and_the_valid_one_is_not():
    c = E.case_f()
    a, b = c["clouds"]
    tiny, small, good = (math.hypot(*p) for p in (E.F_TINY, E.F_SMALL, (E.F_RP, E.F_L)))
    assert not E.frame(a, tiny).builds  # slot 0 refuses first
    assert E.frame(a, small).builds and not E.frame(b, small).builds  # slot 0 is re-indexed, then slot 1 refuses
    assert E.frame(a, good).builds and E.frame(b, good).builds and E.frame(a, E.F_CELL).builds and E.frame(b, E.F_CELL).builds
