"""The generators of tests/_mesh_edge_cases.py against the models alone (tests/_mesh_ref.py, tests/_mesh_sign_ref.py): every property
the device tests rely on is a property of the inputs, shown here without a GPU.  Per case: the ties and their Morton spread (B), g == 0
exactly (C), zero sums (D), run lengths and lane positions (E), key extremes (F), which triangle wins (G), no degenerate pick (H), and an
empty rounding band (A to G), so the 0.1 % cap of _check_sign never hides a point of these cases."""
import math

import numpy as np
import pytest

import _mesh_edge_cases as E
import _mesh_ref as R
import _mesh_sign_ref as S
import _perturb_ref as P


def _same_topology(a, b):
    assert a["counts"] == b["counts"], (a["counts"], b["counts"])
    for k in ("eid", "edge_flags", "vertex_flags"):
        assert np.array_equal(a[k], b[k]), k
    assert a["edge_normal"].tobytes() == b["edge_normal"].tobytes() and a["vertex_normal"].tobytes() == b["vertex_normal"].tobytes()


@pytest.mark.parametrize("n", E.A_SIZES)
def test_a_strided_totals_and_gates(n):
    c = E.case_a(n)
    dist, topo, sg = E.case_a_models(n)
    d2, q = dist["d2"], c["q"]
    assert n > E.ROUND and len(q) == n and not E.band(sg, d2).any()
    assert topo["counts"]["closed"] and topo["counts"]["oriented_manifold"] and not (sg["flags"] & S.UNSIGNED).any()
    on = d2 == 0.0
    assert on.sum() > 1000 and not np.signbit(d2[on]).any() and (sg["flags"][on] == S.ON).all()
    assert set(dist["region"].tolist()) == set(range(7))
    # the tie groups: four points each, bit-equal, the extreme of their total, nobody else has the value
    D, g = c["gate"], c["groups"]
    assert all(len(s) == 4 for s in g.values()) and g["max_d"][0] == 0 and g["max_d"][-1] == n - 1
    assert (d2[g["max_d"]] == 4.0).all() and (d2 <= 4.0).all() and set(np.flatnonzero(d2 == 4.0)) == set(g["max_d"])
    assert (d2[g["gate"]] == D * D).all() and set(np.flatnonzero(d2 == D * D)) == set(g["gate"]) | {c["ulp"]["gate"]["eq"]}
    sd = sg["signed_d"]
    assert (sd[g["min_signed"]] == -0.3125).all() and set(np.flatnonzero(sd == sd.min())) == set(g["min_signed"])
    tot = S.totals(d2, dist["region"], sd, sg["flags"])
    assert (tot["argmax"], tot["max_signed"], tot["argmin"], tot["min_signed"]) == (0, 2.0, int(g["min_signed"][0]), -0.3125)
    gated = S.totals(d2, dist["region"], sd, sg["flags"], D)
    first = min(int(g["gate"][0]), c["ulp"]["gate"]["eq"])
    assert (gated["argmax"], gated["max_signed"], gated["argmin"]) == (first, D, tot["argmin"]) and gated["n_matched"] < n
    assert R.totals(dist, D)["worst_index"] == first and R.totals(dist)["worst_index"] == 0
    if n > 2 * E.ROUND:  # the same block's first and second round hold members of every group
        assert all(s[0] < E.ROUND and s[0] + E.ROUND in s for s in g.values())
    # the gates: exactly the value, one double above, one double below
    for name, u in c["ulp"].items():
        T2 = u["T"] * u["T"]
        assert math.sqrt(T2) == u["T"], "T * T is exact"
        assert (d2[u["eq"]], d2[u["above"]], d2[u["below"]]) == (T2, np.nextafter(T2, math.inf), np.nextafter(T2, 0.0)), name
    t = R.totals(dist, D, c["thresholds"])
    at = np.array([[u["eq"], u["above"], u["below"]] for u in c["ulp"].values()])
    assert not (d2[at[:, 1]] <= (np.array([D, *c["thresholds"]]) ** 2)).any()
    assert t["n_matched"] == int((d2 <= D * D).sum()) and t["n_within"][0] == int((d2 <= 0.140625).sum()) and t["n_within"][1] == int((d2 <= 1.5625).sum())
    assert t["n_within"][0] < t["n_within"][1] < t["n_matched"]


@pytest.mark.parametrize("shifted", [False, True])
def test_b_ties_across_subtrees(shifted):
    c = E.case_b(shifted)
    v, t, q = c["v"], c["t"], c["q"]
    assert len(t) == 1024 and len(q) <= 5000
    corners = v[t]
    spread = np.zeros(len(q), bool)
    base = E.case_b_model(shifted, "as_generated")
    for name in E.B_ORDERS:
        order = c["orders"][name]
        rank = R.morton_rank(v, t[order])
        m = E.case_b_model(shifted, name)
        lower_later = 0
        for s in range(0, len(q), 128):
            dd = R.closest(q[s:s + 128, None, :], corners[order][None, :, 0], corners[order][None, :, 1], corners[order][None, :, 2])[0]
            tied = dd == dd.min(1, keepdims=True)
            assert np.array_equal(np.argmax(tied, 1), m["tri"][s:s + 128]), "the winner is the smallest caller index of the bit-equal minima"
            r = np.where(tied, rank[None, :], -1)
            spread[s:s + 128] = (r.max(1) - np.where(tied, rank[None, :], 1 << 30).min(1)) > 8
            lower_later += int((rank[m["tri"][s:s + 128]] > np.where(tied, rank[None, :], 1 << 30).min(1) + 8).sum())
        assert spread.mean() >= 0.3 and spread[:c["n_mid"]].all(), name
        if name != "as_generated":
            assert lower_later > 0.3 * len(q), "the winner stands more than a leaf behind another bit-equal minimum in Morton order"
        assert np.array_equal(m["d2"], base["d2"]), "the distance does not depend on the caller's order; the winner does"
    assert not np.array_equal(c["orders"]["reversed"][E.case_b_model(shifted, "reversed")["tri"]], base["tri"])
    assert R.morton_rank(v, t).tolist() != list(range(1024))
    sg = S.signed(q, v, t, base, S.topology(v, t))
    assert not E.band(sg, base["d2"]).any()


def test_c_g_is_exactly_zero_beside_a_flat_sheet():
    c = E.case_c()
    v, t = c["v"], c["t"]
    dist, topo, sg = E.models(v, t, c["plane"])
    assert (dist["region"] != R.FACE).all() and (dist["region"] >= 4).any() and ((dist["region"] >= 1) & (dist["region"] <= 3)).any()
    assert (sg["g"] == 0.0).all() and (np.abs(sg["N"][:, 2]) > 0).all() and (sg["N"][:, :2] == 0).all() and not sg["structural"].any()
    assert (sg["flags"] == S.UNSIGNED | S.UNRELIABLE).all() and np.isnan(sg["signed_d"]).all() and (dist["d2"] > 0).all()
    for side, sign in (("up", 1.0), ("down", -1.0)):
        dist, _, sg = E.models(v, t, c[side])
        assert not E.band(sg, dist["d2"]).any() and (sg["flags"] == S.UNRELIABLE).all()
        assert np.array_equal(sg["signed_d"], sign * np.sqrt(dist["d2"]))
    q = np.vstack([c["plane"], c["up"], c["down"]])
    dist, _, sg = E.models(v, t, q)
    tot = S.totals(dist["d2"], dist["region"], sg["signed_d"], sg["flags"])
    k = len(c["plane"])
    assert (tot["n_unsigned"], tot["n_unreliable"], tot["n_outside"], tot["n_inside"], tot["n_on"]) == (k, 3 * k, k, k, 0)


def test_d_every_sum_is_zero_on_the_double_sided_sheet():
    c = E.case_d()
    v, t = c["v"], c["t"]
    topo = S.topology(v, t)
    _same_topology(topo, S.record_topology(v, t))
    cnt = topo["counts"]
    assert cnt["closed"] and cnt["oriented_manifold"] and cnt["n_zero_edges"] == cnt["n_edges"] == 3 * c["n_front"]
    assert cnt["n_unreferenced_vertices"] == 0 and cnt["n_zero_vertices"] == len(v) and cnt["n_tainted_vertices"] == 0
    assert (topo["vertex_flags"] == S.ZERO).all() and (topo["edge_flags"] == S.ZERO).all()
    assert (topo["vertex_normal"] == 0).all() and (topo["edge_normal"] == 0).all() and (topo["valence"] == 2).all()
    for side, sign in (("face_up", 1.0), ("face_down", -1.0)):
        dist, _, sg = E.models(v, t, c[side])
        assert (dist["region"] == R.FACE).all() and (dist["tri"] < c["n_front"]).all(), "the front copy (normal +z) wins the tie with its reverse"
        assert np.array_equal(sg["signed_d"], np.full(len(c[side]), sign * 0.125)) and (sg["flags"] == 0).all() and not E.band(sg, dist["d2"]).any()
    dist, _, sg = E.models(v, t, c["off"])
    assert (dist["region"] != R.FACE).all() and (sg["flags"] == S.UNSIGNED).all() and sg["structural"].all() and (dist["d2"] > 0).all()
    dist, _, sg = E.models(v, t, c["on"])
    assert (dist["d2"] == 0).all() and (sg["flags"] == S.ON).all() and (sg["signed_d"] == 0).all() and not np.signbit(sg["signed_d"]).any()


@pytest.mark.parametrize("lane", sorted(E.E_LANES))
@pytest.mark.parametrize("kind", ["fan", "fin"])
def test_e_runs_longer_than_a_block(kind, lane):
    c = E.case_e(kind, lane)
    v, t, q = c["v"], c["t"], c["q"]
    rec = S.record_topology(v, t)
    _same_topology(S.topology(v, t), rec)
    runs = rec["vertex_runs"] if kind == "fan" else rec["edge_runs"]
    long_runs = [r for r in runs if r[1] >= 256]
    head, length, key = long_runs[0]
    assert len(long_runs) == 1 and (head, length) == (c["head"], E.E_RUN) and head % 256 == lane
    assert head // 256 != (head + length - 1) // 256, "the run crosses a block boundary"
    if kind == "fan":
        assert key == c["first"] and rec["counts"]["n_unreferenced_vertices"] == 5
        assert not rec["vertex_flags"][c["first"]] & (S.ZERO | S.TAINTED)
    else:
        bits = S.key_bits(len(v))
        assert key == (c["first"] << bits) | (c["first"] + 1) and rec["counts"]["n_nonmanifold_edges"] == 1
        vr = {k: (h, n) for h, n, k in rec["vertex_runs"]}
        assert vr[c["first"]] == (c["head"], E.E_RUN) and vr[c["first"] + 1] == (c["head"] + E.E_RUN, E.E_RUN)
    dist, topo, sg = E.models(v, t, q)
    assert len(q) == E.E_RUN and not E.band(sg, dist["d2"]).any() and (dist["tri"] >= len(t) - E.E_RUN).all()
    assert (dist["region"] >= 4).any() and ((dist["region"] >= 1) & (dist["region"] <= 3)).any() and (dist["region"] == 0).any()
    assert (sg["signed_d"] > 0).any() and (sg["signed_d"] < 0).any() and (sg["flags"] & S.ON).any()


@pytest.mark.parametrize("nv", E.F_NV)
def test_f_key_packing_at_powers_of_two(nv):
    c = E.case_f(nv)
    v, t = c["v"], c["t"]
    assert len(v) == nv
    bits = S.key_bits(nv)
    assert nv < (1 << bits) and nv >= (1 << (bits - 1))
    key, val, no_edge, _ = S.edge_records(t, nv)
    real = key[key != no_edge]
    assert real.max() == ((nv - 2) << bits) | (nv - 1) and no_edge == (nv << bits) | nv > real.max() and (key == no_edge).sum() == 3
    assert (np.diff(key) >= 0).all() and (key[-3:] == no_edge).all() and no_edge < (1 << (2 * bits))
    vkey, _ = S.corner_records(t, nv)
    assert vkey.max() == nv - 1 and (np.diff(vkey) >= 0).all()
    topo = S.topology(v, t)
    _same_topology(topo, S.record_topology(v, t))
    (t1, e1), (t2, e2) = c["top_edge"]
    assert topo["eid"][t1, e1] == topo["eid"][t2, e2] == topo["counts"]["n_edges"] - 1
    # (at nv = 8 the vertices 6 and 7 are the cube's own, and its edge (6, 7) now carries four triangles)
    assert topo["edge_flags"][t1, e1] == (S.NONMANIFOLD if nv == 8 else 0) and (topo["edge_normal"][t1, e1] != 0).any()
    assert (topo["eid"][c["twice"]] == -1).all() and (topo["edge_flags"][c["twice"]] == S.ZERO).all() and (topo["edge_normal"][c["twice"]] == 0).all()


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("kind", ["pair", "cube"])
def test_g_degenerate_neighbour(kind, first):
    c = E.case_g(kind, first)
    v, t, q = c["v"], c["t"], c["q"]
    topo = S.topology(v, t)
    _same_topology(topo, S.record_topology(v, t))
    assert topo["deg"].sum() == 1 and topo["deg"][c["deg"]]
    (ta, ea), (tb, eb), real = c["shared"]
    assert topo["eid"][ta, ea] == topo["eid"][tb, eb] >= 0
    assert topo["edge_flags"][ta, ea] == 0, "m == 2: not BOUNDARY although one face only gives a normal; not ZERO"
    nhat = S.faces(v, t)[1]
    assert topo["edge_normal"][ta, ea].tobytes() == nhat[real].tobytes()
    if kind == "cube":
        assert topo["counts"]["closed"] and topo["counts"]["oriented_manifold"] and topo["counts"]["n_zero_edges"] == 0
    dist, _, sg = E.models(v, t, q)
    assert not E.band(sg, dist["d2"]).any()
    tie = slice(0, c["n_tie"])
    a, b, g = (v[t][None, :, k] for k in range(3))
    dd = R.closest(q[tie, None, :], a, b, g, topo["deg"][None, :])[0]
    assert ((dd == dd.min(1, keepdims=True)).sum(1) >= 2).all() and (dd[:, c["deg"]] == dd.min(1)).all(), "the degenerate triangle ties"
    if first:
        assert (dist["tri"][tie] == c["deg"]).all() and (sg["flags"][tie] & S.UNSIGNED).all() and (sg["g"][tie] != 0).all()
    else:
        assert (dist["tri"][tie] != c["deg"]).all() and not (sg["flags"][tie] & S.UNSIGNED).any() and (sg["signed_d"][tie] != 0).all()


def test_h_sampler_never_picks_a_zero_area_triangle():
    c = E.case_h()
    v, t = c["v"], c["t"]
    area, deg = R.areas(v, t)
    cum = np.cumsum(area)
    z0, zm, z1 = c["zero"]
    assert sorted(np.flatnonzero(deg)) == [z0, zm, z1] == [0, len(t) // 2, len(t) - 1] and (area[deg] == 0).all() and (area[~deg] > 0).all()
    assert cum[0] == 0.0 and cum[zm] == cum[zm - 1] and cum[z1] == cum[z1 - 1]
    for seed in c["seeds"]:
        pts, pick = R.sample(v, t, c["n"], seed)
        assert not deg[pick].any() and len(np.unique(pick)) == len(t) - 3, "every real triangle is drawn, no zero-area one"
        u = P.u01(P.philox4x64_10(np.arange(c["n"], dtype=np.uint64), 0, 0, 0, int(seed), 0)[0]) * cum[-1]
        assert (u < cum[-1]).all() and ((cum[pick] > u) & (np.where(pick > 0, cum[pick - 1], 0.0) <= u)).all()
