"""me_m3c2 on the MI355X at the places tests/test_gpu_m3c2.py does not reach, on the inputs of tests/_m3c2_edge_cases.py (whose
properties tests/test_m3c2_edges_cpu.py proves): k_m3_final striding over more than 256 * 1024 core points with four equal maxima, the
clamp into the other cloud's frame at both ends of every axis, waves whose lanes sit in unrelated cells, runs longer than the wave
tile and coincident duplicates, the gates of k_m3_final at equality, and a refused radius.  Every cloud is uploaded with cell_size = R,
so the frame _m3c2_edge_cases.frame() computes is the one the library builds.  The sets are compared with np.array_equal on every core
point; where the sums do not depend on their order (dyadic lattices, axis normals; identical t) dist and the variances are compared
with ==, lod with the two ulp of DESIGN.md section 4.15, the sums of the totals with n_valid u max|term| against math.fsum."""
import math
import struct

import numpy as np
import pytest

import _m3c2_edge_cases as E
import _search_ref as SR

pytestmark = pytest.mark.gpu

U = E.U
FLOAT_TOTALS = ("sum_dist", "sum_abs_dist", "sum_dist2", "sum_lod", "max_abs_dist")
INT_TOTALS = ("n_core", "n_no_normal", "n_valid", "n_significant", "sum_n_own", "sum_n_other", "argmax")
PER_POINT = ("dist", "lod", "var_own", "var_other", "n_own", "n_other", "valid", "significant")


def _engine(own, other, nrm, cell, query=0):
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    e.upload(query, own, cell_size=cell)
    e.upload(1 - query, other, cell_size=cell)
    e.set_normals(query, nrm)
    return e


def _bytes(tot):
    return struct.pack("<5d7q", *[tot[k] for k in FLOAT_TOTALS], *[tot[k] for k in INT_TOTALS])


def _same_sets(pp, m):
    for k in ("n_own", "n_other", "valid"):
        assert np.array_equal(pp[k], m[k]), k


def _same_values(pp, m):
    """a case whose sums do not depend on their order: the model's bits"""
    v = m["valid"]
    assert m["order_free"][v].all()
    for k in ("dist", "var_own", "var_other"):
        assert np.array_equal(pp[k], m[k]), k  # (zeros where invalid or masked out, on both sides)
        assert not np.signbit(pp[k][~v]).any() and (k == "dist" or not np.signbit(pp[k]).any()), k
    _lod_and_significance(pp, m["lod"])
    assert (pp["lod"][~v] == 0).all() and not pp["significant"][~v].any()


def _lod_and_significance(pp, lod):
    """lod within two ulp of the evaluation on the device's own values (here the model's: they are equal), significance exact on them"""
    assert (np.abs(pp["lod"] - lod) <= 2 * np.spacing(lod)).all()
    assert np.array_equal(pp["significant"], pp["valid"] & (np.abs(pp["dist"]) > pp["lod"]))


def _totals_follow(tot, pp, n_core, sums=False):
    """the totals against the device's own per-point result: the integer fields and the maximum exactly; with `sums` the four sums
    within n_valid u max|term| of math.fsum (case A, as tests/test_gpu_m3c2.py: on a handful of nearly equal terms that bound is
    below half an ulp of the total, so the small cases check the integer fields and the pair alone)"""
    v = pp["valid"]
    nv = int(v.sum())
    assert (tot["n_core"], tot["n_no_normal"], tot["n_valid"], tot["n_significant"]) == (n_core, 0, nv, int(pp["significant"].sum()))
    assert tot["sum_n_own"] == int(pp["n_own"][v].sum(dtype=np.int64)) and tot["sum_n_other"] == int(pp["n_other"][v].sum(dtype=np.int64))
    d = pp["dist"][v]
    for key, terms in (("sum_dist", d), ("sum_abs_dist", np.abs(d)), ("sum_dist2", d * d), ("sum_lod", pp["lod"][v])) if sums else ():
        err, bound = abs(tot[key] - math.fsum(terms)), nv * U * float(np.abs(terms).max())
        print(key, "error:", err, "bound n_valid u max|term|:", bound)
        assert err <= bound, key
    worst = np.flatnonzero(v & (np.abs(pp["dist"]) == np.abs(d).max()))
    assert struct.pack("<d", tot["max_abs_dist"]) == struct.pack("<d", float(np.abs(d).max())) and tot["argmax"] == int(worst.min())


# ---- A ---------------------------------------------------------------------------------------------------------------------------
def test_a_strided_totals_and_the_smallest_index_among_equal_maxima():
    c = E.case_a()
    m, mask, slots, n = c["model"], c["mask"], c["slots"], c["n"]
    with _engine(c["own"], c["other"], c["nrm"], math.hypot(E.A_RP, E.A_L)) as e:
        t1, pp = e.m3c2(0, E.A_RP, E.A_L, E.A_MIN, E.A_REG, mask, fetch=True)
        t2 = e.m3c2(0, E.A_RP, E.A_L, E.A_MIN, E.A_REG, mask)
        t_all, pp_all = e.m3c2(0, E.A_RP, E.A_L, E.A_MIN, E.A_REG, None, fetch=True)
        t_none, pp_none = e.m3c2(0, E.A_RP, E.A_L, E.A_MIN, E.A_REG, np.zeros(n, np.uint8), fetch=True)
    # the masked call: about 1500 core points spread over the whole index range, against the model
    _same_sets(pp, m)
    _same_values(pp, m)
    assert t1["argmax"] == int(slots.min()) == 0 and struct.pack("<d", t1["max_abs_dist"]) == struct.pack("<d", 1.0)
    assert pp["dist"][0] == -1.0  # (the smallest index holds a negative distance: the key is |dist|)
    v = m["valid"]
    assert (t1["n_core"], t1["n_no_normal"], t1["n_valid"]) == (int(mask.sum()), 0, int(v.sum()))
    assert t1["n_significant"] == int(m["significant"].sum())
    assert t1["sum_n_own"] == int(m["n_own"][v].sum(dtype=np.int64)) and t1["sum_n_other"] == int(m["n_other"][v].sum(dtype=np.int64))
    _totals_follow(t1, pp, int(mask.sum()), sums=True)
    assert _bytes(t1) == _bytes(t2)  # a second call: byte-identical totals
    # every point a core point: each block of k_m3_final strides, each of 257 threads folds two entries
    assert n > 256 * E.BLOCKS
    core = mask != 0
    for k in PER_POINT:
        assert np.array_equal(pp_all[k][core], pp[k][core]), k  # (a point's result does not depend on the mask)
    _lod_and_significance(pp_all, 1.96 * (np.sqrt(pp_all["var_own"] / np.maximum(pp_all["n_own"], 1) + pp_all["var_other"] / np.maximum(pp_all["n_other"], 1))
                                          + E.A_REG) * pp_all["valid"])
    assert pp_all["valid"].sum() > 100000 and (pp_all["n_own"] > 0).all()
    _totals_follow(t_all, pp_all, n, sums=True)
    assert t_all["argmax"] == 0 and t_all["max_abs_dist"] == 1.0
    # no core point at all
    assert (t_none["n_core"], t_none["n_valid"], t_none["argmax"]) == (0, 0, -1)
    for k in FLOAT_TOTALS:
        assert struct.pack("<d", t_none[k]) == struct.pack("<d", 0.0), k
    for k in INT_TOTALS[:-1]:
        assert t_none[k] == 0, k
    for k in PER_POINT:
        assert not pp_none[k].any(), k


# ---- B ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("query", [0, 1])
def test_b_core_points_in_around_and_beyond_the_other_frames_border_cells(query):
    c = E.case_b()
    m = c["model"]
    with _engine(c["own"], c["other"], c["nrm"], E.RB, query) as e:
        tot, pp = e.m3c2(query, E.RP, E.L, E.B_MIN, 0.0, None, fetch=True)
    _same_sets(pp, m)
    assert np.array_equal(pp["significant"], pp["valid"] & (np.abs(pp["dist"]) > pp["lod"]))
    far = c["far"]
    assert pp["n_other"][far] == 0 and pp["n_own"][far] == 1 and not pp["valid"][far]
    assert tot["n_core"] == len(c["own"]) and tot["n_valid"] == int(m["valid"].sum()) > 0
    assert tot["sum_n_other"] == int(m["n_other"][m["valid"]].sum())


# ---- C ---------------------------------------------------------------------------------------------------------------------------
def test_c_every_lane_in_a_cell_of_its_own():
    c = E.case_c()
    with _engine(c["own"], c["other"], c["nrm"], E.RB) as e:
        tot, pp = e.m3c2(0, E.RP, E.L, E.C_MIN, 0.0, c["mask"], fetch=True)
    _same_sets(pp, c["model"])
    _same_values(pp, c["model"])
    _totals_follow(tot, pp, 144)
    assert tot["n_valid"] == 144
    with _engine(c["lone"], c["other"], c["lone_nrm"], E.RB) as e:  # without the companions: 64 pending lanes, 64 unrelated cells
        tot, pp = e.m3c2(0, E.RP, E.L, 2, 0.0, None, fetch=True)
    _same_sets(pp, c["lone_model"])
    assert (pp["n_other"] == 5).all() and (pp["n_own"] == 1).all() and tot["n_valid"] == 0 and tot["n_core"] == 144
    for k in ("dist", "lod", "var_own", "var_other"):
        assert not pp[k].any(), k


# ---- D ---------------------------------------------------------------------------------------------------------------------------
def test_d_runs_longer_than_the_wave_tile_and_coincident_duplicates():
    c = E.case_d()
    m = c["model"]
    with _engine(c["own"], c["other"], c["nrm"], E.RB) as e:
        tot, pp = e.m3c2(0, E.RP, E.L, E.D_MIN, 0.0, None, fetch=True)
    _same_sets(pp, m)
    _same_values(pp, m)
    assert set(np.unique(pp["n_other"]).tolist()) == set(E.D_RUNS) and pp["n_own"].max() == E.D_DUPLICATES and pp["valid"].all()
    _totals_follow(tot, pp, len(c["own"]))


# ---- E ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_points", E.E_MINS)
def test_e_min_points_on_either_cloud(min_points):
    c = E.case_e_counts()
    m = c["models"][min_points]
    with _engine(c["own"], c["other"], c["nrm"], E.RB) as e:
        tot, pp = e.m3c2(0, E.RP, E.L, min_points, 0.0, None, fetch=True)
    _same_sets(pp, m)
    _same_values(pp, m)
    group = c["combos"][:, 0] == min_points
    assert np.array_equal(pp["valid"][group], (c["combos"][group, 1] == min_points) & (c["combos"][group, 2] == min_points))
    inv = ~pp["valid"]
    assert inv.any() and np.array_equal(pp["n_own"][inv], c["combos"][inv, 1]) and np.array_equal(pp["n_other"][inv], c["combos"][inv, 2])
    for k in ("dist", "lod", "var_own", "var_other"):
        assert not pp[k][inv].any(), k
    _totals_follow(tot, pp, len(c["own"]))


def test_e_clamped_variance_is_plus_zero_and_an_unclamped_one_keeps_its_bits():
    c = E.case_e_variance()
    m = c["model"]
    with _engine(c["own"], c["other"], c["nrm"], E.RB) as e:
        tot, pp = e.m3c2(0, E.RP, E.L, 5, 0.0, None, fetch=True)
    _same_sets(pp, m)
    _same_values(pp, m)
    negative = np.array([k[2] for k in c["kind"]])
    assert negative.any() and (~negative).any() and (m["raw_other"][negative] < 0).all()
    assert (pp["var_other"][negative] == 0.0).all() and not np.signbit(pp["var_other"][negative]).any()
    assert np.array_equal(pp["var_other"][~negative].view(np.uint64), m["raw_other"][~negative].view(np.uint64)) and (pp["var_other"][~negative] > 0).all()
    assert np.isfinite(pp["lod"]).all()


def test_e_significance_is_strict_at_lod_equal_to_the_distance():
    c = E.case_e_counts()
    below, equal, above = E.lod_triple()
    assert equal is not None  # (the CPU test shows that equality is met: all three are run)
    with _engine(c["own"], c["other"], c["nrm"], E.RB) as e:
        for reg, expect in ((equal, False), (below, True), (above, False)):
            tot, pp = e.m3c2(0, E.RP, E.L, 2, reg, None, fetch=True)
            v = pp["valid"]
            assert v.sum() >= 15 and (pp["dist"][v] == E.E_DIST).all() and not pp["var_own"][v].any() and not pp["var_other"][v].any()
            assert (pp["lod"][v] == E.lod_of(reg)).all()
            assert (pp["significant"][v] == expect).all() and tot["n_significant"] == (int(v.sum()) if expect else 0)
        assert E.lod_of(equal) == E.E_DIST and E.lod_of(below) < E.E_DIST < E.lod_of(above)


# ---- F ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refused", ["tiny", "far", "both"])
def test_f_a_refused_radius_leaves_the_engine_as_it_was(refused):
    """tiny: rp and L so small that slot 0, the first to be re-indexed, would need more than 2^21 cells per axis: nothing is touched.
    far: a radius that slot 0 takes and slot 1 with its one far point does not: slot 0 has been re-indexed (its sorted results are
    gone, as after any re-index), slot 1 keeps its index.  Either way every later pass works on both slots, a lazy rebuild included
    (the transform at the end rebuilds at the cell size of the upload).  both: the one after the other on one engine."""
    from cloud_map_evaluation_amd.engine import Engine, MapEvalError

    c = E.case_f()
    clouds, normals = c["clouds"], c["normals"]
    with Engine(0) as e:
        for s in (0, 1):
            e.upload(s, clouds[s], cell_size=E.F_CELL)
            e.set_normals(s, normals[s])
        t1, p1 = e.m3c2(0, E.F_RP, E.F_L, fetch=True)
        assert t1["n_valid"] > 800
        nn = {s: e.nn1(s, 1 - s) for s in (0, 1)}
        for query, (rp, depth) in {"tiny": [(0, E.F_TINY)], "far": [(1, E.F_SMALL)], "both": [(0, E.F_TINY), (1, E.F_SMALL)]}[refused]:
            with pytest.raises(MapEvalError, match=r"^\[-1\]"):
                e.m3c2(query, rp, depth)
        if refused == "tiny":  # no slot was re-indexed: everything resident is still there
            p = e.m3c2_fetch(0)
            assert all(np.array_equal(p[k], p1[k]) for k in PER_POINT)
            for s in (0, 1):
                idx, d2 = e.nn_fetch(s)
                assert np.array_equal(idx, nn[s][0]) and np.array_equal(d2, nn[s][1])
        else:  # slot 0 took the small radius and was re-indexed: its result went with its sorted order
            with pytest.raises(MapEvalError, match=r"^\[-3\]"):
                e.m3c2_fetch(0)
        order = SR.ordered(clouds[0], clouds[1])
        idx, d2 = e.knn_search(0, 1, 4)
        ref_idx, ref_d2 = SR.knn_from(order, 4)
        assert np.array_equal(idx, ref_idx) and np.array_equal(d2, ref_d2)
        off, idx, d2 = e.radius_search(0, 1, 0.05)
        ref = SR.radius_from(order, 0.05)
        assert np.array_equal(off, ref[0]) and np.array_equal(idx, ref[1]) and np.array_equal(d2, ref[2])
        for s in (0, 1):
            idx, d2 = e.nn1(s, 1 - s)
            brute = SR.dist2(clouds[s], clouds[1 - s]).min(axis=1)
            assert np.array_equal(d2, brute) and np.array_equal(SR.dist2(clouds[s], clouds[1 - s])[np.arange(len(idx)), idx], brute)
        healthy = 1 if refused == "tiny" else 0  # (the slot the refusal did not come from; the other one is rebuilt lazily below)
        assert e.mme(healthy, E.F_CELL, 5, per_point=False) is not None
        t2, p2 = e.m3c2(0, E.F_RP, E.F_L, fetch=True)
        assert _bytes(t1) == _bytes(t2) and all(np.array_equal(p1[k], p2[k]) for k in PER_POINT)
        # a lazy rebuild of either slot is at the cell size of its upload, which both clouds take
        T = np.eye(4)
        T[:3, 3] = (0.25, -0.5, 0.125)
        moved = []
        for s in (0, 1):
            e.transform_cloud(s, T)
            moved.append(e.download(s))
        for s in (0, 1):
            idx, d2 = e.nn1(s, 1 - s)
            assert np.array_equal(d2, SR.dist2(moved[s], moved[1 - s]).min(axis=1))
        assert e.mme(1 - healthy, E.F_CELL, 5, per_point=False) is not None
