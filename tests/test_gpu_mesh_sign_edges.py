"""me_mesh_topology and me_mesh_signed_distance on the MI355X at the exact edges of csrc/me_meshsign.hip, on the inputs of
tests/_mesh_edge_cases.py (whose properties tests/test_mesh_edges_cpu.py shows on the models alone).  The comparisons are
test_gpu_mesh._check and test_gpu_mesh_sign._check_topology / _check_sign, unchanged; on top of _check_sign every case asserts that
its rounding band is EMPTY, so the 0.1 % cap hides no point here."""
import math

import numpy as np
import pytest

import _mesh_edge_cases as E
import _mesh_ref as R
import _mesh_sign_ref as S
from test_gpu_mesh import _check
from test_gpu_mesh_sign import _check_sign, _check_topology, _engine

pytestmark = pytest.mark.gpu

TOTAL_KEYS = ("n_query", "n_matched", "n_signed", "n_inside", "n_outside", "n_on", "n_unsigned", "n_unreliable", "argmin", "argmax",
              "min_signed", "max_signed")


def _run(q, v, t, max_distance=math.inf, banded=True):
    """One cloud against one mesh: the distance, the topology and the sign, each against its model.  banded=False is for queries whose g
    is exactly zero on the model AND on the device (flat geometry: the pseudo-normal's in-plane components are exact zeros whatever
    atan2 returns): _check_sign would put them all into its band, so every point is compared instead, none excluded."""
    q = np.ascontiguousarray(q, np.float64)
    with _engine() as e:
        e.upload(0, q)
        e.mesh_upload(v, t)
        dt, pp = e.mesh_distance(0, fetch=True)
        cnt, tf = e.mesh_topology(fetch=True)
        tot, sp = e.mesh_signed_distance(0, max_distance, fetch=True)
    _check(dt, pp, q, v, t)
    topo = _check_topology(cnt, tf, v, t)
    if banded:
        m = _check_sign(tot, sp, pp, q, v, t, topo, max_distance)
        assert not E.band(m, pp["d2"]).any(), "a point in the rounding band"
    else:
        m = S.signed(q, v, t, pp, topo)
        assert np.array_equal(sp["signed_d"], m["signed_d"], equal_nan=True) and np.array_equal(sp["flags"], m["flags"])
        want = S.totals(pp["d2"], pp["region"], sp["signed_d"], sp["flags"], max_distance)
        assert all(tot[k] == want[k] for k in TOTAL_KEYS) and list(tot["n_by_region"]) == want["n_by_region"]
    return tot, sp, pp, cnt, tf, m


@pytest.mark.parametrize("n", E.A_SIZES)
def test_a_strided_totals_and_gate_of_k_sign_final(n):
    """Items 1 and 2.  More than 256 * 1024 queries against the cube: every block of k_sign_final strides (me_meshsign.hip:263),
    take_max (me_meshsign.hip:282) meets the largest signed distance in four lanes of different rounds and blocks, and the second,
    negated pass (me_meshsign.hip:454, `negate ? -s : s`) the smallest; argmax and argmin must be the smallest original index of their
    group.  The gate `!(d2_s[i] <= max2)` (me_meshsign.hip:264) sees d2 == D * D (counted: it is then the largest signed distance), the
    next double above (not counted) and the next double below."""
    c = E.case_a(n)
    v, t, q, D = c["v"], c["t"], c["q"], c["gate"]
    dist, _, sg = E.case_a_models(n)
    with _engine() as e:
        e.upload(0, q)
        e.mesh_upload(v, t)
        _, pp = e.mesh_distance(0, fetch=True)
        cnt, tf = e.mesh_topology(fetch=True)
        tot, sp = e.mesh_signed_distance(0, fetch=True)
        gated, gp = e.mesh_signed_distance(0, D, fetch=True)
    assert all(np.array_equal(pp[k], dist[k]) for k in ("d2", "tri", "region", "closest"))
    topo = _check_topology(cnt, tf, v, t)
    for res, per, md in ((tot, sp, math.inf), (gated, gp, D)):
        m = _check_sign(res, per, pp, q, v, t, topo, md)
        assert not E.band(m, pp["d2"]).any()
        assert np.array_equal(per["signed_d"], sg["signed_d"]) and np.array_equal(per["flags"], sg["flags"])
    g, u = c["groups"], c["ulp"]["gate"]
    assert (tot["argmax"], tot["max_signed"], tot["argmin"], tot["min_signed"]) == (int(g["max_d"][0]), 2.0, int(g["min_signed"][0]), -0.3125)
    first = min(int(g["gate"][0]), u["eq"])
    assert (gated["argmax"], gated["max_signed"], gated["argmin"], gated["min_signed"]) == (first, D, int(g["min_signed"][0]), -0.3125)
    d2 = dist["d2"]
    want = S.totals(d2, dist["region"], sg["signed_d"], sg["flags"], D)
    assert gated["n_matched"] == gated["n_signed"] == want["n_matched"] == int((d2 < D * D).sum()) + 5, "the points at equality count"
    assert list(gated["n_by_region"]) == want["n_by_region"] and sum(want["n_by_region"]) == want["n_matched"] < n
    assert (gp["signed_d"][[u["eq"], u["above"], u["below"]]] > 0).all() and d2[u["above"]] > D * D > d2[u["below"]]


def test_c_g_is_exactly_zero_beside_a_flat_sheet():
    """Item 4.  In-plane queries beyond the rim and the corners of a flat sheet: the closest feature is an edge or a vertex whose
    pseudo-normal is not zero, and g == 0.0 exactly: the last `else` of k_mesh_sign (me_meshsign.hip:235) gives UNSIGNED, the flags
    are UNSIGNED | UNRELIABLE (the rim is BOUNDARY, its vertices TAINTED) and signed_d is NaN.  The same queries lifted by +-1/8 are
    signed +-sqrt(d2) and UNRELIABLE."""
    c = E.case_c()
    v, t = c["v"], c["t"]
    tot, sp, pp, _, _, m = _run(c["plane"], v, t, banded=False)
    k = len(c["plane"])
    assert (pp["region"] != R.FACE).all() and (m["g"] == 0.0).all() and (np.abs(m["N"]).sum(1) > 0).all()
    assert (sp["flags"] == S.UNSIGNED | S.UNRELIABLE).all() and np.isnan(sp["signed_d"]).all()
    assert (tot["n_unsigned"], tot["n_unreliable"], tot["n_signed"], tot["argmax"], tot["argmin"]) == (k, k, 0, -1, -1)
    for side, sign in (("up", 1.0), ("down", -1.0)):
        tot, sp, pp, _, _, m = _run(c[side], v, t)
        assert np.array_equal(sp["signed_d"], sign * np.sqrt(pp["d2"])) and (sp["flags"] == S.UNRELIABLE).all()
        assert (tot["n_unsigned"], tot["n_unreliable"], tot["n_outside"], tot["n_inside"]) == (0, k, k * (sign > 0), k * (sign < 0))
    tot, sp, pp, _, _, _ = _run(np.vstack([c["plane"], c["up"], c["down"]]), v, t, banded=False)
    assert (tot["n_unsigned"], tot["n_unreliable"], tot["n_outside"], tot["n_inside"], tot["n_on"]) == (k, 3 * k, k, k, 0)


def test_d_zero_features_on_a_closed_manifold():
    """Item 5.  Every triangle of the sheet over its own three vertices, and once more reversed: closed, oriented_manifold, and every
    edge sum and vertex sum exactly zero, so TOPO_ZERO comes from `s == 0` with n_face == 2 in k_topo_edges (me_meshsign.hip:120) and
    k_topo_verts (me_meshsign.hip:160), passes k_topo_expand (me_meshsign.hip:180-181) and makes k_mesh_sign answer UNSIGNED by
    `tf & ME_MESH_TOPO_ZERO` (me_meshsign.hip:232) off the faces.  On a face the winner is the copy with the lower caller index, the
    front one (normal +z): above the sheet is outside (+), below is inside (-).  Points on the sheet are ON with +0.0."""
    c = E.case_d()
    v, t = c["v"], c["t"]
    q = np.vstack([c["face_up"], c["face_down"], c["off"], c["on"]])
    a, b = len(c["face_up"]), len(c["face_up"]) + len(c["face_down"])
    off = slice(b, b + len(c["off"]))
    tot, sp, pp, cnt, tf, m = _run(q, v, t)
    assert cnt["closed"] and cnt["oriented_manifold"] and cnt["n_zero_edges"] == cnt["n_edges"] == 3 * c["n_front"]
    assert cnt["n_zero_vertices"] == len(v) and cnt["n_unreferenced_vertices"] == 0
    assert (tf["vertex_flags"] == S.ZERO).all() and (tf["edge_flags"] == S.ZERO).all()
    assert (tf["vertex_normal"] == 0).all() and (tf["edge_normal"] == 0).all()
    assert (pp["tri"][:b] < c["n_front"]).all() and (pp["region"][:b] == R.FACE).all()
    assert (sp["signed_d"][:a] == 0.125).all() and (sp["signed_d"][a:b] == -0.125).all() and (sp["flags"][:b] == 0).all()
    assert (pp["region"][off] != R.FACE).all() and (sp["flags"][off] == S.UNSIGNED).all() and np.isnan(sp["signed_d"][off]).all()
    on = slice(off.stop, len(q))
    assert (sp["flags"][on] == S.ON).all() and (sp["signed_d"][on] == 0).all() and not np.signbit(sp["signed_d"][on]).any()
    assert (tot["n_unsigned"], tot["n_on"], tot["n_unreliable"]) == (len(c["off"]), len(c["on"]), 0)


@pytest.mark.parametrize("lane", sorted(E.E_LANES))
@pytest.mark.parametrize("kind", ["fan", "fin"])
def test_e_runs_longer_than_a_block(kind, lane):
    """Item 6.  A run of 300 equal keys whose head stands on lane 255 of a block, or on lane 0, and which ends in the next block: the
    head's lane walks it serially through the sorted records, `for (j = i; j < n && key[j] == k; ++j)`, in k_topo_verts
    (me_meshsign.hip:145; the fan's hub, and the fin's two end vertices) and in k_topo_edges (me_meshsign.hip:102; the fin's shared
    edge, NONMANIFOLD), while no other lane of either block may start in it (`head[i]`, me_meshsign.hip:96 and :140)."""
    c = E.case_e(kind, lane)
    v, t = c["v"], c["t"]
    tot, sp, pp, cnt, tf, m = _run(c["q"], v, t)
    assert cnt["n_unreferenced_vertices"] == 5 and cnt["n_nonmanifold_edges"] == (kind == "fin")
    assert tot["n_query"] == E.E_RUN and tot["n_inside"] > 0 and tot["n_outside"] > 0 and tot["n_on"] > 0
    if kind == "fan":
        assert tf["vertex_flags"][c["first"]] == 0 and (tf["vertex_normal"][c["first"], :2] == 0).all()
        assert abs(tf["vertex_normal"][c["first"], 2] - 2.0 * math.pi) < 1e-12
    else:
        assert (tf["edge_flags"][-E.E_RUN:, 0] == S.NONMANIFOLD).all() and (tf["vertex_flags"][c["first"]:c["first"] + 2] == S.TAINTED).all()


@pytest.mark.parametrize("nv", E.F_NV)
def test_f_key_packing_at_powers_of_two(nv):
    """Item 7.  n_vertices at and around 2^3, 2^4 and 2^8 with triangles that name the vertices nv - 2, nv - 1 and 0: `bits` is the
    smallest value with nv < 2^bits (me_meshsign.hip:310-311), the edge key `lo << bits | hi` (me_meshsign.hip:66) takes its largest
    real value, no_edge (me_meshsign.hip:312) lies above it, and the sorts run over 2 * bits (me_meshsign.hip:339) and bits
    (me_meshsign.hip:361) bits: one bit too few in either place merges or misorders these keys."""
    c = E.case_f(nv)
    v, t = c["v"], c["t"]
    with _engine() as e:
        e.mesh_upload(v, t)
        cnt, tf = e.mesh_topology(fetch=True)
    m = _check_topology(cnt, tf, v, t)
    (t1, e1), (t2, e2) = c["top_edge"]
    assert m["eid"][t1, e1] == m["eid"][t2, e2] == cnt["n_edges"] - 1
    assert tf["edge_flags"][t1, e1] == tf["edge_flags"][t2, e2] == m["edge_flags"][t1, e1] == (S.NONMANIFOLD if nv == 8 else 0)
    assert tf["edge_normal"][t1, e1].tobytes() == tf["edge_normal"][t2, e2].tobytes() == m["edge_normal"][t1, e1].tobytes()
    assert (tf["edge_flags"][c["twice"]] == S.ZERO).all() and (tf["edge_normal"][c["twice"]] == 0).all()
    assert not tf["vertex_flags"][nv - 1] & S.ZERO and not tf["vertex_flags"][nv - 2] & S.ZERO


@pytest.mark.parametrize("first", [True, False], ids=["degenerate_first", "degenerate_last"])
@pytest.mark.parametrize("kind", ["pair", "cube"])
def test_g_degenerate_triangle_beside_a_real_one(kind, first):
    """Item 8.  A collinear triangle shares an edge with a real one: m == 2 but n_face == 1.  BOUNDARY is decided by m
    (`if (m == 1)`, me_meshsign.hip:117), not by the faces that give a normal (`if (!deg[t])`, me_meshsign.hip:110; the same at
    the vertices, me_meshsign.hip:149): the shared edge is neither BOUNDARY nor ZERO and its normal is the single face normal.  Queries
    at equal distance from both: with the degenerate triangle first in the caller's order it wins and k_mesh_sign answers UNSIGNED
    by `degenerate` (me_meshsign.hip:232) although g != 0; with the real one first the edge's pseudo-normal gives the sign."""
    c = E.case_g(kind, first)
    v, t = c["v"], c["t"]
    tot, sp, pp, cnt, tf, m = _run(c["q"], v, t)
    (ta, ea), (tb, eb), real = c["shared"]
    assert tf["edge_flags"][ta, ea] == tf["edge_flags"][tb, eb] == 0
    assert tf["edge_normal"][ta, ea].tobytes() == tf["edge_normal"][tb, eb].tobytes() == S.faces(v, t)[1][real].tobytes()
    tie = slice(0, c["n_tie"])
    if first:
        assert (pp["tri"][tie] == c["deg"]).all() and (sp["flags"][tie] & S.UNSIGNED).all() and np.isnan(sp["signed_d"][tie]).all()
        assert (m["g"][tie] != 0).all()
    else:
        assert (pp["tri"][tie] != c["deg"]).all() and not (sp["flags"][tie] & S.UNSIGNED).any() and not np.isnan(sp["signed_d"][tie]).any()
    if kind == "cube":
        assert cnt["closed"] and cnt["oriented_manifold"] and cnt["n_zero_edges"] == 0
