"""me_perturb_cloud on the MI355X (csrc/me_perturb.hip) at its exact edges, against the cases of tests/_perturb_edge_cases.py (the
numpy model, the region rule's signs from mpmath).  The largest cloud has 20 001 points.

EXACT (np.array_equal on the uint64 views): every geometry-decided keep pattern at 1 .. 20 001 points under both ratio assignments;
the survivors at the region borders (products of 0, x == +-k region, survey offsets, fl(k 0.3)); the copies of the deformation
(d == R, d == 0, R = NaN); every point count and every outlier count m; every outlier at range 0 against the downloaded survivor
the model's base index names; every seed's survivor set (the 64-bit Philox key).  WITHIN THE BOUNDS OF test_gpu_perturb.py
(_perturb_ref.survivor_bound / outlier_bound): the moved deform points, the noise and the non-zero outlier offsets.  Then: the
result does not depend on the launch shape, in place equals out of place at 1 / 257 / 4097 points, a refused call leaves dst with
its 1-NN result and normals, an uploaded but empty source is refused, and a borrowed dst buffer is replaced, not written."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _perturb_edge_cases as E  # noqa: E402
import _perturb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

EST, GT = 0, 1
CELL = 0.2


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _run(eng, src, kw, dst=EST, cell=CELL):
    eng.upload(GT, src, cell_size=cell)
    n = eng.perturb(dst, GT, **kw)
    out = eng.download(dst)
    assert len(out) == n == eng.size(dst)
    return out


def _refused(eng, src, kw, match):
    from cloud_map_evaluation_amd.engine import MapEvalError

    eng.upload(GT, src, cell_size=CELL)
    with pytest.raises(MapEvalError, match=match):
        eng.perturb(EST, GT, **kw)


def _check_against_model(c, out):
    """the whole result of a case: counts exactly, survivors and outliers within the bounds test_gpu_perturb.py uses"""
    ref, kw = c["ref"], c["kw"]
    nk, m = ref["n_kept"], len(ref["bases"])
    assert len(out) == nk + m, f"{c['name']}: point count"
    kept, outl = out[:nk], out[nk:]
    bound = R.survivor_bound(kw.get("noise_std", 0.0), ref["deformed"], kw.get("deform_strength", 0.0))
    np.testing.assert_array_less(np.abs((kept - ref["deformed"]) - ref["noise"]), bound, err_msg=c["name"])
    if m:
        rng = kw["outlier_range"]
        off = outl - kept[ref["bases"]]
        if rng == 0.0:
            assert _same(outl, kept[ref["bases"]]), f"{c['name']}: an outlier at range 0 is not its base point"
        else:
            np.testing.assert_array_less(np.abs(off - R.outlier_offsets(m, rng, kw["seed"])), R.outlier_bound(rng, outl), err_msg=c["name"])


# ---- the compaction -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.SIZES)
def test_keep_patterns_compact_bit_for_bit_in_source_order(eng, n):
    for c in E.pattern_cases(n):
        if c["expect"] is None:  # nobody kept: refused, whatever the size
            _refused(eng, c["src"], c["kw"], "no point")
            continue
        out = _run(eng, c["src"], c["kw"])
        assert len(out) == int(c["pattern"].sum()), f"{c['name']}: n_kept"
        assert _same(out, c["expect"]), c["name"]


# ---- the region rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("region", [1.0, 0.3])
def test_region_borders_keep_the_models_survivors(eng, region):
    for c in E.border_cases():
        if c["kw"]["region_size"] != region:
            continue
        out = _run(eng, c["src"], c["kw"], cell=c["cell"])
        want = c["src"][c["ref"]["src_index"]]
        if not _same(out, want):  # name the points that changed sides
            got = {p.tobytes() for p in out}
            exp = {p.tobytes() for p in want}
            wrong = [tuple(p) for p in c["src"] if (p.tobytes() in got) != (p.tobytes() in exp)]
            raise AssertionError(f"{c['name']}: {len(wrong)} points on the wrong side, the first {wrong[:6]}")


# ---- the deformation --------------------------------------------------------------------------------------------------------------------
def test_deform_edges(eng):
    for c in E.deform_cases():
        out = _run(eng, c["src"], c["kw"], cell=c["cell"])
        _check_against_model(c, out)
        for i in c.get("copies", ()):
            assert np.array_equal(_bits(out[i]), _bits(c["src"][i])), f"{c['name']}: {c['names'][i]} is no bit-exact copy"
        if c["name"] == "deform/inf_R":  # w = 1: pushed by exactly strength along the direction
            far = [i for i, k in enumerate(c["names"]) if k != "centre"]
            np.testing.assert_allclose(np.linalg.norm(out[far] - c["src"][far], axis=1), 0.3, rtol=0, atol=1e-14)
        if "flips" in c:  # the keep decision is the deformed point's: the survivor set is the model's, exactly
            assert len(out) == len(c["ref"]["src_index"]) == (1 if c["flips"] == "kept_to_dropped" else 2)
            assert _same(out[-1:], c["src"][2:3])  # the kept bystander, untouched


def test_nan_region_size_switches_the_density_stage_off(eng):
    src = E.lattice(257, np.arange(257) % 2 == 0)
    out = _run(eng, src, dict(sparse_ratio=0.0, dense_ratio=0.0, region_size=float("nan"), seed=7))
    assert _same(out, src)


# ---- outliers ---------------------------------------------------------------------------------------------------------------------------
def test_outlier_counts_and_bases(eng):
    for c in E.outlier_cases():
        out = _run(eng, c["src"], c["kw"])
        nk, m = c["ref"]["n_kept"], len(c["ref"]["bases"])
        assert len(out) - nk == m, f"{c['name']}: m"
        if c["m"] is not None:
            assert len(out) - nk == c["m"], f"{c['name']}: m"
        _check_against_model(c, out)
        if "noise_std" not in c["kw"] and "deform_radius" not in c["kw"]:  # no arithmetic on the survivors: copies of the source
            assert _same(out[:nk], c["src"][c["ref"]["src_index"]]), c["name"]


# ---- the 64-bit key ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", E.SEEDS)
def test_seed_survivor_set(eng, seed):
    c = next(c for c in E.seed_cases() if c["kw"]["seed"] == seed)
    out = _run(eng, c["src"], c["kw"])
    assert _same(out, c["src"][c["ref"]["src_index"]])


# ---- nothing depends on the launch shape -------------------------------------------------------------------------------------------
def test_prefix_of_the_cloud_gives_the_prefix_of_the_result(eng):
    i = np.arange(4097)
    src = E.lattice(4097, i % 3 != 0)
    kw = dict(noise_std=0.05, deform_radius=1.0, deform_strength=0.3, deform_center=(0.25, 0.5, 0.125), seed=(1 << 40) + 3)
    full = _run(eng, src, kw)
    _check_against_model({"name": "full cloud", "ref": R.perturb(src, **kw), "kw": kw}, full)
    assert np.all(full != src)  # every coordinate noised
    for n in (257, 64):
        part = _run(eng, src[:n], kw)
        assert _same(part, full[:n]), n
    dens = dict(kw, sparse_ratio=0.4, dense_ratio=0.7, region_size=0.25)
    ref = R.perturb(src, **dens)
    full = _run(eng, src, dens)
    assert len(full) == ref["n_kept"]
    part = _run(eng, src[:257], dens)
    k = int((ref["src_index"] < 257).sum())
    assert 50 < k < 257 and len(part) == k
    assert _same(part, full[:k])


# ---- in place at small sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_in_place_equals_out_of_place(eng, n):
    src = E.lattice(n)
    for what, kw in (("shrinks", dict(sparse_ratio=0.5, dense_ratio=0.5, region_size=1.0, seed=3)),  # (seed 3 keeps source point 0, the cloud of n = 1)
                     ("grows", dict(outlier_ratio=1.0, outlier_range=0.5, seed=7)),
                     ("same size", dict(noise_std=0.05, deform_radius=1.0, deform_strength=-0.2, deform_center=(0.5, 0.5, 0.0), seed=7))):
        ref = R.perturb(src, **kw)
        want = {"shrinks": ref["n_kept"], "grows": 2 * n, "same size": n}[what]
        assert want == len(ref["points"]) and (what != "shrinks" or n == 1 or want < n)
        a = _run(eng, src, kw)
        eng.upload(EST, src, cell_size=CELL)
        assert eng.perturb(EST, EST, **kw) == want
        b = eng.download(EST)
        assert _same(a, b), (what, n)
        assert _same(eng.download(GT), src)  # (and the source of the out-of-place call is still the source)


# ---- a refused call -------------------------------------------------------------------------------------------------------------------
def _dst_state(eng):
    idx, d2 = eng.nn_fetch(EST)
    return eng.download(EST), idx, d2, eng.get_normals(EST)


def _assert_state(eng, before, what):
    after = _dst_state(eng)
    for a, b in zip(before, after):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"dst changed by a refused call: {what}"


def test_a_refused_call_leaves_dst_as_it_was(eng):
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import MapEvalError

    nan, inf = float("nan"), float("inf")
    src = E.lattice(300)
    dst = E.lattice(500, np.arange(500) % 5 != 0) + [0.0, 0.0, 0.03125]
    eng.upload(GT, src, cell_size=CELL)
    eng.upload(EST, dst, cell_size=CELL)
    eng.nn1(EST, GT)
    eng.estimate_normals(EST, knn=8)
    before = _dst_state(eng)
    assert _same(before[0], dst) and np.isfinite(before[3]).all()
    on = dict(deform_radius=1.0, deform_strength=0.3)
    bad = [dict(noise_std=-1.0), dict(noise_std=inf), dict(noise_std=nan), dict(sparse_ratio=1.5), dict(sparse_ratio=nan),
           dict(dense_ratio=-0.1), dict(outlier_ratio=2.0), dict(outlier_ratio=nan), dict(outlier_range=-1.0), dict(outlier_range=inf),
           dict(on, deform_strength=nan), dict(on, deform_strength=inf), dict(on, deform_strength=-inf),
           dict(on, deform_center=(nan, 0, 0)), dict(on, deform_center=(0, inf, 0)), dict(on, deform_center=(0, 0, -inf)),
           dict(on, deform_radius=inf, deform_center=(0, 0, nan))]
    for kw in bad:
        with pytest.raises(MapEvalError, match=r"\[-1\]"):
            eng.perturb(EST, GT, **kw)
        _assert_state(eng, before, kw)
    with pytest.raises(MapEvalError, match=r"\[-1\].*no point"):  # no survivor
        eng.perturb(EST, GT, sparse_ratio=0.0, dense_ratio=0.0, region_size=1.0)
    _assert_state(eng, before, "no survivor")
    n = C.c_int64(-5)
    pp = _lib.PerturbParams(sparse_ratio=1.0, dense_ratio=1.0)
    assert eng._L.me_perturb_cloud(eng._ctx, EST, GT, None, C.byref(n)) == -1 and n.value == -5  # p NULL
    assert eng._L.me_perturb_cloud(eng._ctx, EST, 2, C.byref(pp), C.byref(n)) == -1                # a bad slot
    _assert_state(eng, before, "NULL / bad slot")
    eng.set_shard(0, 2)
    with pytest.raises(MapEvalError, match="shard"):
        eng.perturb(EST, GT, noise_std=0.01)
    eng.set_shard(0, 1)
    _assert_state(eng, before, "shard mode")
    # a non-finite centre or strength is nobody's business while the deform stage is off; NaN radius: off
    assert eng.perturb(EST, GT, deform_radius=0.0, deform_strength=nan, deform_center=(nan, nan, nan)) == len(src)
    assert _same(eng.download(EST), src)
    assert eng.perturb(EST, GT, deform_radius=nan, deform_strength=0.3, deform_center=(inf, 0, 0)) == len(src)
    assert _same(eng.download(EST), src)
    # ... and the next good call succeeds
    assert eng.perturb(EST, GT, noise_std=0.01, deform_radius=inf, deform_strength=0.1, seed=3) == len(src)
    assert np.isfinite(eng.download(EST)).all()


# ---- the empty source -----------------------------------------------------------------------------------------------------------------
def test_an_uploaded_but_empty_source_is_refused():
    """A me_mesh_scan without a hit leaves its slot uploaded with 0 points.  me_perturb_cloud refuses it before any allocation, launch
    or read (with the density stage on it would read the scan's entry n - 1), as every other single-GPU entry does."""
    from cloud_map_evaluation_amd.engine import Engine, MapEvalError

    dst = E.lattice(300, np.arange(300) % 2 == 0)
    with Engine(0) as eng:
        eng.upload(EST, dst, cell_size=CELL)
        eng.estimate_normals(EST, knn=8)
        before = (eng.download(EST), eng.get_normals(EST))
        eng.mesh_upload(np.array([[0.0, 0.0, 5.0], [1.0, 0.0, 5.0], [0.0, 1.0, 5.0]]), np.array([[0, 1, 2]], np.int32))
        beams = np.array([[0.0, 0.0, -1.0], [0.6, 0.0, -0.8], [0.0, -0.6, -0.8]])  # away from the triangle at z = 5
        res = eng.mesh_scan(GT, np.eye(4)[None], beams)
        assert res["n_hit"] == 0 and res["n_rays"] == 3 and eng.size(GT) == 0
        for kw in (dict(sparse_ratio=0.5, dense_ratio=0.5, region_size=1.0), {}, dict(noise_std=0.1, outlier_ratio=0.5, outlier_range=1.0)):
            for d in (EST, GT):  # into the other slot, and in place
                with pytest.raises(MapEvalError, match=r"\[-3\].*the slot's cloud is empty"):
                    eng.perturb(d, GT, **kw)
                after = (eng.download(EST), eng.get_normals(EST))
                assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and eng.size(GT) == 0
        # the context is as good as before: a real source perturbs
        src = E.lattice(65)
        eng.upload(GT, src, cell_size=CELL)
        assert eng.perturb(EST, GT, sparse_ratio=1.0, dense_ratio=0.0, region_size=1.0) == 65
        assert _same(eng.download(EST), src)


# ---- a borrowed dst buffer --------------------------------------------------------------------------------------------------------------
def test_a_borrowed_dst_buffer_is_replaced_not_written():
    import torch

    from cloud_map_evaluation_amd.engine import Engine

    mine = E.lattice(4097, np.arange(4097) % 2 == 0) + [0.0, 0.0, 0.03125]
    src = E.lattice(257)
    kw = dict(noise_std=0.05, outlier_ratio=0.5, outlier_range=0.0, seed=1 << 63)
    ref = R.perturb(src, **kw)
    t = torch.from_numpy(mine.copy()).cuda()
    with Engine(0, borrow_device_input=True) as eng:
        eng.upload(EST, t, cell_size=CELL)  # me_upload_cloud_device: read where it lies (room for the whole result, were it written)
        eng.upload(GT, src, cell_size=CELL)
        assert eng.perturb(EST, GT, **kw) == len(ref["points"]) == 257 + 128
        out = eng.download(EST)
        torch.cuda.synchronize()
        assert _same(t.cpu().numpy(), mine), "the caller's tensor was written"
    c = {"name": "borrowed", "ref": ref, "kw": kw}
    _check_against_model(c, out)
