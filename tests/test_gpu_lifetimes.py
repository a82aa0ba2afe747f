"""Every resident result across every re-sort, point replacement and input replacement (tests/_lifetime.py holds the tables).

Per (producer, disturber, own | other) cell, on a fresh engine: make the result, fetch it twice (bytewise equal), run the disturber
with the timers on (a re-sort disturber must launch k_morton, a new-points disturber must change download()), fetch again.  The
outcome must be the one EXPECT names - ME_ERR_STATE for DROP, the same bytes for KEEP, the rotation model of
tests/_reg_ref.py for ROTATED, and for NEW the bytes of a fresh engine that ran the disturber without the producer's make (after a
point replacement also: other bytes than before) - and, whatever the table says, a successful fetch that returns other bytes than
before is a failure everywhere but in the NEW and ROTATED cells.  Comparisons are bytes against an engine's bytes, or an error code:
the numbers themselves belong to the per-feature suites.

That a re-sort happened is asserted per cell from the k_morton launch count.  That the new permutation differs from the old one is
NOT proved here: the module only checks on the CPU that the radius-cell ids of the points (cloud_build_index's cell formula) are not
order-isomorphic between the two cell sizes - a plausibility check on the inputs, about cells, with no model of the Hilbert order of
the finer codes the library sorts on.  The sorted-order results do not lean on it: their own-slot re-sort cells are DROP, where any
successful fetch fails.
"""
import re

import numpy as np
import pytest

import _lifetime as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _sorts_differ_and_scratch():
    for s in (0, 1):
        a, b = L.cell_ids(L.points(s), L.CELL), L.cell_ids(L.points(s), L.R_FAR)
        assert not L.order_isomorphic(a, b), "the cell ids of the two sizes are order-isomorphic: choose other inputs"
        assert L.order_isomorphic(a, a)
    yield
    L.close_scratch()


def _same(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def _fetch(P, e, s):
    from cloud_map_evaluation_amd.engine import MapEvalError

    try:
        return {k: np.ascontiguousarray(v) for k, v in P["fetch"](e, s).items()}, None
    except MapEvalError as ex:
        return None, str(ex)


def _cell(pname, dname, side, twin=False):
    """-> None, or what went wrong"""
    from cloud_map_evaluation_amd.engine import Engine

    import _reg_ref

    P, D = L.PRODUCERS[pname], L.DISTURBERS[dname]
    want = L.EXPECT[(pname, dname, side)][0]
    s = 0
    t = s if side == "own" else 1 - s
    with Engine(0) as e:
        L.base(e)
        P["make"](e, s)
        before, err = _fetch(P, e, s)
        if before is None:
            return f"the fetch after make failed: {err}"
        again, err = _fetch(P, e, s)
        if again is None or not _same(before, again):
            return "two fetches in a row differ"
        lane = e.twin() if twin else e
        lane.timers_enable(True)
        m0 = lane.timer("morton")[1]
        xyz0 = e.download(t)
        D["act"](lane, t)
        if D["group"] == "resort":
            need = 2 if D.get("both") else 1
            if lane.timer("morton")[1] - m0 < need:
                return f"the disturber did not re-sort (k_morton launches rose by {lane.timer('morton')[1] - m0}, want >= {need})"
        if D["group"] == "points":
            xyz1 = e.download(t)
            if xyz1.shape == xyz0.shape and np.array_equal(xyz1, xyz0):
                return "the disturber left the points as they were"
        after, err = _fetch(P, e, s)
        if after is None:
            if not re.search(r"\[-3\]", err):
                return f"fetch failed with something else than ME_ERR_STATE: {err}"
            got = L.DROP
        elif _same(before, after):
            got = L.KEEP
        else:
            got = "CHANGED"
        if want == L.DROP or want == L.KEEP:
            return None if got == want else f"want {want}, got {got}"  # (CHANGED fails both: the safety net)
        if got == L.DROP:
            return f"want {want}, got DROP ({err})"
        if want == L.ROTATED:
            n2, c2 = _reg_ref.rotate_attr(L.transform(), before.get("normals"), before.get("cov"))
            model = {"normals": n2} if "normals" in before else {"cov": c2.reshape(before["cov"].shape)}
            return None if _same(model, after) else "want ROTATED, the fetch differs from the rotation model"
        # NEW: a current result of the disturber's own making, with nothing of the earlier one in it
        if D["group"] == "points" and got == L.KEEP:
            return "want NEW after a point replacement, the fetch returns the earlier bytes (a result about points that are gone)"
        if P.get("make_alters_inputs"):
            return None if got == "CHANGED" else "want NEW, the fetch returns the earlier bytes"
    with Engine(0) as f:  # the same event on an engine that never held the earlier result
        L.base(f)
        D["act"](f.twin() if twin else f, t)
        fresh, err = _fetch(P, f, s)
    if fresh is None:
        return f"want NEW, the fetch on a fresh engine failed: {err}"
    return None if _same(fresh, after) else "want NEW, the fetch differs from a fresh engine's after the same event"


def _sweep(pname, disturbers, twin=False):
    bad = []
    for dname in disturbers:
        for side in L.SIDES:
            try:
                why = _cell(pname, dname, side, twin)
            except Exception as ex:  # noqa: BLE001  (one run names the whole set)
                why = f"{type(ex).__name__}: {ex}"
            if why:
                bad.append(f"({pname}, {dname}, {side}) [{L.EXPECT[(pname, dname, side)][0]}]: {why}")
    assert not bad, f"{len(bad)} cells fail:\n" + "\n".join(bad)


@pytest.mark.parametrize("pname", list(L.PRODUCERS))
def test_lifetime(pname):
    _sweep(pname, list(L.DISTURBERS))


@pytest.mark.parametrize("pname", list(L.PRODUCERS))
def test_lifetime_through_the_twin(pname):
    """the clouds are shared: a re-sort driven through the twin lane obeys the same row"""
    _sweep(pname, L.RESORT, twin=True)


# ----------------------------------------------------------------------------------------------------------- empty slab uploads
SLAB_LEGAL = {"nn1", "mme"}  # H:me_set_slab names the 1-NN and the MME passes; every other producer is "single GPU only"


def _slab_results(e, names):
    """make + fetch of every named producer on slot 0 -> (results, names refused).  Only the slab-mode refusal is caught: an error
    whose text names the slab mode, at make or at fetch; anything else propagates."""
    from cloud_map_evaluation_amd.engine import MapEvalError

    out, refused = {}, set()
    for name in names:
        P = L.PRODUCERS[name]
        try:
            P["make"](e, 0)
            out[name] = {k: np.ascontiguousarray(v) for k, v in P["fetch"](e, 0).items()}
        except MapEvalError as ex:
            if not re.search(r"\[-[13]\].*slab", str(ex)):
                raise
            refused.add(name)
    return out, refused


@pytest.mark.parametrize("path", ["filter", "prefiltered"])
def test_empty_slab_upload_drops_everything(path):
    import torch

    from cloud_map_evaluation_amd.engine import Engine

    def fill(e):
        e.set_slab(0, 0.0, 2.0, 0.125)  # the whole unit cube
        for s in (0, 1):
            e.upload(s, L.points(s), cell_size=L.CELL)

    with Engine(0) as fresh:
        fill(fresh)
        ref, refused = _slab_results(fresh, list(L.PRODUCERS))
    assert set(ref) == SLAB_LEGAL and refused == set(L.PRODUCERS) - SLAB_LEGAL, (sorted(ref), sorted(refused))
    with Engine(0) as e:
        fill(e)
        assert set(_slab_results(e, sorted(SLAB_LEGAL))[0]) == SLAB_LEGAL
        e.set_slab(0, 5.0, 6.0, 0.125)  # nothing of the cloud
        if path == "filter":
            e.upload(0, L.points(0), cell_size=L.CELL)
        else:
            e.upload_slab(0, torch.empty((0, 3), dtype=torch.float64, device="cuda:0"), cell_size=L.CELL)
        assert e.size(0) == 0
        bad = []
        for name in sorted(SLAB_LEGAL):
            got, err = _fetch(L.PRODUCERS[name], e, 0)
            if got is not None or not re.search(r"\[-3\]", err):
                bad.append(f"{name}: {'a fetch succeeded on the empty slot' if got is not None else err}")
        got, err = _fetch(L.PRODUCERS["nn1"], e, 1)  # (slot 1 had searched in the cloud that is gone)
        if got is not None or not re.search(r"\[-3\]", err):
            bad.append("nn1 of slot 1, which searched in the replaced cloud, is still fetchable")
        assert not bad, "\n".join(bad)
        fill(e)
        again = _slab_results(e, sorted(SLAB_LEGAL))[0]
        assert set(again) == SLAB_LEGAL
        assert all(_same(again[k], ref[k]) for k in ref), [k for k in ref if not _same(again[k], ref[k])]


# ------------------------------------------------------------------------------- the requested cell size across a borrowed rebuild
def _rebuilds(e, slot, radius):
    """does me_local_geometry(radius) re-sort the slot?  Its documented rule: kept iff radius (1 + 2^-20) <= cell <= 1.5 radius (1 + 2^-20)"""
    e.timers_enable(True)
    m0 = e.timer("morton")[1]
    e.local_geometry(slot, radius, 5)
    return e.timer("morton")[1] > m0


def _suite_from(e, s):
    from cloud_map_evaluation_amd.engine import Param

    e.run_suite_from(None, None, Param(icp_max_distance_=1.0, nn_radius_=L.R_FAR, vmd_voxel_size_=L.VOX), overlap=False)


BORROWERS = {"cluster_dbscan": L.DISTURBERS["cluster_dbscan"]["act"], "mme": L.DISTURBERS["mme"]["act"],
             "run_suite": L.DISTURBERS["run_suite"]["act"], "run_suite_from": _suite_from}


@pytest.mark.parametrize("borrower,cell_after", [("cluster_dbscan", L.CELL), ("mme", L.R_FAR), ("run_suite", L.R_FAR), ("run_suite_from", L.R_FAR)])
def test_requested_cell_size_after_a_rebuild_at_another_radius(borrower, cell_after):
    """me_cluster_dbscan borrows the index and restores the cell size asked for at the upload; me_mme and the two suite calls adopt
    their radius (header, me_mme INDEX): the index me_transform_cloud builds afterwards has that cell"""
    from cloud_map_evaluation_amd.engine import Engine

    T = np.eye(4)
    T[:3, 3] = (0.5, 0.25, -0.125)
    with Engine(0) as e:
        L.base(e)
        BORROWERS[borrower](e, 0)
        e.transform_cloud(0, T)
        assert not _rebuilds(e, 0, cell_after), f"the index after the transform is not at {cell_after}"
        other = L.R_FAR if cell_after == L.CELL else L.CELL
        assert _rebuilds(e, 0, other)  # (the probe discriminates)
        e.transform_cloud(0, np.linalg.inv(T))  # ... and the request still stands after the probe's own borrowed rebuild
        assert not _rebuilds(e, 0, cell_after)
    with Engine(0) as e, Engine(0) as f:
        L.base(e)
        BORROWERS[borrower](e, 0)
        e.transform_cloud(0, T)
        L.base(f, cell=cell_after)
        f.transform_cloud(0, T)
        for a, b in zip(e.nn1(0, 1), f.nn1(0, 1)):
            assert np.array_equal(a, b)
        for a, b in zip(e.mme(0, cell_after, 5)[1:3], f.mme(0, cell_after, 5)[1:3]):
            assert a.tobytes() == b.tobytes()  # (sums in the sorted order: equal bytes only on the same index)
