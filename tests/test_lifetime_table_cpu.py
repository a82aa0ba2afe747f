"""The lifetime tables of tests/_lifetime.py are complete, cited and not vacuous (no GPU)."""
import re

import _lifetime as L


def test_every_cell_has_a_cited_entry():
    assert len(L.PRODUCERS) >= 16 and len(L.DISTURBERS) >= 23
    for p in L.PRODUCERS:
        for d in L.DISTURBERS:
            for side in L.SIDES:
                assert (p, d, side) in L.EXPECT, (p, d, side)
                verdict, cite = L.EXPECT[(p, d, side)]
                assert verdict in (L.KEEP, L.DROP, L.ROTATED, L.NEW)
                # a citation names the header ("H:" + entry point) or a DESIGN.md section ("D:" + number)
                assert isinstance(cite, str) and re.search(r"\b[HD]:\S", cite), (p, d, side, cite)
    assert len(L.EXPECT) == len(L.PRODUCERS) * len(L.DISTURBERS) * 2


def test_rotated_is_the_one_documented_carry_over():
    rotated = {k for k, v in L.EXPECT.items() if v[0] == L.ROTATED}
    assert rotated == {("normals", "transform_cloud", "own"), ("covariances", "transform_cloud", "own")}


def test_new_only_where_the_disturber_writes_the_result():
    for (p, d, side), (verdict, _) in L.EXPECT.items():
        if verdict == L.NEW:
            D = L.DISTURBERS[d]
            assert p in D.get("writes", ()) + D.get("writes_other", ()) or (L.PRODUCERS[p].get("rebuilt_on_demand") and D["group"] == "points")


def test_keep_floor():
    """a table that accepted DROP everywhere would hide a library that forgets everything"""
    assert len(L.RESORT) == 8
    assert set(L.CLOUD_ORDER) == {"normals", "covariances", "fpfh", "outlier_mask", "cluster", "planes", "orient"}
    for cell in L.KEEP_FLOOR:
        assert L.EXPECT[cell][0] == L.KEEP, cell
    # the cloud-order results under every re-sort of their slot that does not write them or replace the normals
    for p in ("outlier_mask", "cluster", "planes"):
        assert sum((p, d, "own") in L.KEEP_FLOOR for d in L.RESORT) >= 7
    for p in ("normals", "covariances", "fpfh", "orient"):
        assert sum((p, d, "own") in L.KEEP_FLOOR for d in L.RESORT) == 7  # (all but radius_normals)
    # every slot-keyed result under the other slot's mme, cluster_dbscan, local_geometry, radius_outlier, reconstruct
    slot_keyed = [p for p, P in L.PRODUCERS.items() if P["keyed"] == "slot"]
    assert len(slot_keyed) >= 11
    for p in slot_keyed:
        for d in ("mme", "cluster_dbscan", "local_geometry", "radius_outlier", "reconstruct"):
            assert (p, d, "other") in L.KEEP_FLOOR
    # ... and under the searches that write no 1-NN result nothing is listed as a disturber at all: they re-index no slot
    assert len(L.KEEP_FLOOR) >= 120
    keep = sum(v[0] == L.KEEP for v in L.EXPECT.values())
    assert keep >= len(L.EXPECT) // 2


def test_only_engine_methods_are_used():
    from cloud_map_evaluation_amd.engine import Engine

    for table in (L.PRODUCERS, L.DISTURBERS):
        for name, entry in table.items():
            assert entry["engine"], name
            for m in entry["engine"]:
                assert callable(getattr(Engine, m, None)), (name, m)
    for m in ("twin", "timers_enable", "timer", "download", "size", "set_slab", "upload_slab", "transform_cloud"):
        assert callable(getattr(Engine, m, None)), m


def test_the_two_sorts_group_the_points_differently():
    for s in (0, 1):
        a, b = L.cell_ids(L.points(s), L.CELL), L.cell_ids(L.points(s), L.R_FAR)
        assert not L.order_isomorphic(a, b) and L.order_isomorphic(a, a) and L.order_isomorphic(b, b)


def test_design_document_carries_this_table():
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    assert "```\n" + L.render() + "\n```" in text, "DESIGN.md 4.21 does not show the table tests/_lifetime.py derives"
