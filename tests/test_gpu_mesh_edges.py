"""me_mesh_distance and me_mesh_sample on the MI355X at the exact edges of csrc/me_mesh.hip, on the inputs of tests/_mesh_edge_cases.py
(whose properties tests/test_mesh_edges_cpu.py shows on the models alone).  The comparison is test_gpu_mesh._check, unchanged: d2,
triangle, region and closest point EQUAL to the brute-force model on every point, counts equal, sums within 1e-9.

Out of scope: the `taken` bytes of the tree levels 9 to 16 of k_mesh_dist (taken_get / taken_set with s >= 64) need more than 8^8
triangles."""
import math

import numpy as np
import pytest

import _mesh_edge_cases as E
import _mesh_ref as R
from test_gpu_mesh import _check, _engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", E.A_SIZES)
def test_a_strided_totals_and_gates_of_k_mesh_final(n):
    """Items 1 and 2.  More than 256 * 1024 queries against the cube: every block of k_mesh_final strides (`i += stride`,
    me_mesh.hip:286), take_max (me_mesh.hip:302) meets the largest d in four lanes of different rounds and blocks and must keep the
    smallest original index, here 0 without a gate and the first point at d == D with one.  The gate `!(d2 <= g.max2)`
    (me_mesh.hip:288) and the two threshold counts `d2 <= g.t2[k]` (me_mesh.hip:295) each see a point at exactly the value, one at the
    next double above and one at the next double below."""
    c = E.case_a(n)
    v, t, q, D, ths = c["v"], c["t"], c["q"], c["gate"], c["thresholds"]
    dist = E.case_a_models(n)[0]
    with _engine() as e:
        e.upload(0, q)
        e.mesh_upload(v, t)
        tot, pp = e.mesh_distance(0, thresholds=ths, fetch=True)
        gated, pg = e.mesh_distance(0, D, ths, fetch=True)
    _check(tot, pp, q, v, t, math.inf, ths, model=dist)
    _check(gated, pg, q, v, t, D, ths, model=dist)
    g, u = c["groups"], c["ulp"]
    assert (tot["n_matched"], tot["worst_index"], tot["max"]) == (n, int(g["max_d"][0]), 2.0) and (pp["d2"][g["max_d"]] == 4.0).all()
    first = min(int(g["gate"][0]), u["gate"]["eq"])
    assert (gated["worst_index"], gated["max"]) == (first, D) and (pg["d2"][g["gate"]] == D * D).all()
    d2 = dist["d2"]
    assert gated["n_matched"] == int((d2 <= D * D).sum()) == int((d2 < D * D).sum()) + 5, "the points at equality count"
    assert gated["n_matched"] == n - int((d2 >= np.nextafter(D * D, math.inf)).sum()), "the point one double above does not"
    for k, name in enumerate(("t_lo", "t_hi")):
        T2 = ths[k] * ths[k]
        assert (pg["d2"][u[name]["eq"]], pg["d2"][u[name]["above"]], pg["d2"][u[name]["below"]]) == (T2, np.nextafter(T2, 4.0), np.nextafter(T2, 0.0))
        assert tot["n_within"][k] == gated["n_within"][k] == int((d2 <= T2).sum()) > int((d2 < T2).sum())
        assert tot["n_within"][k] == n - int((d2 >= np.nextafter(T2, 4.0)).sum())


@pytest.mark.parametrize("shifted", [False, True], ids=["origin", "shifted_1024"])
def test_b_bit_equal_distances_in_different_subtrees(shifted):
    """Item 3.  Two parallel sheets, queries on the plane half way: every such query has bit-equal minima in the two halves of the
    tree.  The winner of k_mesh_dist must be the lexicographic minimum of (d2, caller index) (`d == best && o < best_o`,
    me_mesh.hip:225) whichever box is walked first, so the box holding the equal distance must not be pruned: `bb > bound`
    (me_mesh.hip:246) with the bound of mesh_bound (me_mesh.hip:116).  Three caller orders: as generated, reversed (the lower caller
    index lies in the box visited later), a fixed random permutation; and all of it once more moved by (1024, -1024, 1024)."""
    c = E.case_b(shifted)
    v, q = c["v"], c["q"]
    with _engine() as e:
        e.upload(0, q)
        for name in E.B_ORDERS:
            t = np.ascontiguousarray(c["t"][c["orders"][name]])
            e.mesh_upload(v, t)
            tot, pp = e.mesh_distance(0, fetch=True)
            info = e.mesh_info()
            assert (info["triangles"], info["depth"]) == (1024, 4)
            m = _check(tot, pp, q, v, t, model=E.case_b_model(shifted, name))
            assert np.array_equal(pp["tri"], m["tri"]), name
            assert (pp["d2"][:c["n_mid"]] >= 0.25).all() and tot["n_matched"] == len(q)


def test_h_sampler_around_zero_area_triangles():
    """Item 9.  Zero-area triangles (collinear, and a repeated index) first, in the middle and last in the caller's order: the search
    of k_mesh_sample (`cum[mid] > u`, me_mesh.hip:331-336) must pass over cum[0] == 0, over two equal neighbours in the middle and
    must not fall through to the last index, whose cumulative area equals the total."""
    c = E.case_h()
    v, t, n = c["v"], c["t"], c["n"]
    area, deg = R.areas(v, t)
    with _engine() as e:
        e.mesh_upload(v, t)
        info = e.mesh_info()
        assert info["degenerate"] == 3 and info["area"] == np.cumsum(area)[-1]
        for seed in c["seeds"]:
            assert e.mesh_sample(1, n, seed=seed) == n
            want, pick = R.sample(v, t, n, seed)
            assert not deg[pick].any()
            assert np.array_equal(e.download(1), want), seed
