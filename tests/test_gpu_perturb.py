"""me_perturb_cloud on the GPU: each stage alone and all four together against the numpy model (tests/_perturb_ref.py) on a
1 M-point synth scene, the identity, in place, determinism, the counter-based noise, the untouched source, the suite on the result,
the index build it costs, argument errors, and one 50 M-point timing."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _perturb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

EST, GT = 0, 1
NN_RADIUS = 0.2
SEED = 7


@pytest.fixture(scope="module")
def scene():
    from cloud_map_evaluation_amd import synth

    return synth.campus_scene(1_000_000, seed=21).numpy()


def _cases(src):
    c = tuple(float(v) for v in src.mean(axis=0))
    deform = dict(deform_radius=4.0, deform_strength=0.3, deform_center=c)
    density = dict(sparse_ratio=0.3, dense_ratio=0.9, region_size=2.0)
    noise = dict(noise_std=0.05)
    outliers = dict(outlier_ratio=0.05, outlier_range=1.0)
    return {"deform": deform, "density": density, "noise": noise, "outliers": outliers,
            "all": {**deform, **density, **noise, **outliers}}


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run(eng, src, kw, seed=SEED):
    eng.upload(GT, src, cell_size=NN_RADIUS)
    n = eng.perturb(EST, GT, seed=seed, **kw)
    out = eng.download(EST)
    assert len(out) == n
    return out


@pytest.mark.parametrize("case", ["deform", "density", "noise", "outliers", "all"])
def test_stage_matches_the_numpy_model(scene, case):
    kw = _cases(scene)[case]
    ref = R.perturb(scene, seed=SEED, **kw)
    with _engine() as eng:
        out = _run(eng, scene, kw)
    nk = ref["n_kept"]
    assert len(out) == len(ref["points"]), "point count"
    kept, outl = out[:nk], out[nk:]
    # survivor k of the device is the model's survivor k (source index src_index[k]): its offset from the model's deformed point is the
    # model's noise of that source index, within 1e-12 sigma plus the rounding of the subtraction (and of a cos that may differ by an ulp)
    sigma = kw.get("noise_std", 0.0)
    np.testing.assert_array_less(np.abs((kept - ref["deformed"]) - ref["noise"]),
                                 R.survivor_bound(sigma, ref["deformed"], kw.get("deform_strength", 0.0)))
    if case == "density":  # no arithmetic on the survivors at all: bit-exact copies of the source points
        assert np.array_equal(_bits(kept), _bits(scene[ref["src_index"]]))
        assert nk < len(scene)
    if case == "deform":
        moved = np.any(kept != scene, axis=1)
        assert 1000 < moved.sum() < len(scene)
    m = len(ref["bases"])
    assert len(outl) == m
    if m:  # the outliers' base indices: outlier j - its model base point = the model's N(0, range^2) offset
        off = outl - kept[ref["bases"]]
        rng = kw["outlier_range"]
        np.testing.assert_array_less(np.abs(off - R.outlier_offsets(m, rng, SEED)), R.outlier_bound(rng, outl))
        assert m == int(nk * kw["outlier_ratio"])


def test_all_stages_off_is_a_bit_exact_copy(scene):
    with _engine() as eng:
        out = _run(eng, scene, {})
        assert np.array_equal(_bits(out), _bits(scene))
        assert eng.perturb(EST, GT, noise_std=0.0, deform_radius=3.0, deform_strength=0.0, outlier_ratio=0.0) == len(scene)
        assert np.array_equal(_bits(eng.download(EST)), _bits(scene))


def test_in_place_equals_out_of_place(scene):
    kw = _cases(scene)["all"]
    with _engine() as eng:
        a = _run(eng, scene, kw)
        eng.upload(EST, scene, cell_size=NN_RADIUS)
        n = eng.perturb(EST, EST, seed=SEED, **kw)
        b = eng.download(EST)
        assert n == len(a) and np.array_equal(_bits(a), _bits(b))
        # the in-place result is a cloud like any other: index rebuilt, a second in-place pass runs on it
        eng.perturb(EST, EST, seed=SEED + 1, noise_std=0.01)
        assert eng.size(EST) == n


def test_deterministic_and_seeded(scene):
    kw = _cases(scene)["all"]
    with _engine() as eng:
        a = _run(eng, scene, kw)
        b = _run(eng, scene, kw)
        c = _run(eng, scene, kw, seed=SEED + 1)
    assert np.array_equal(_bits(a), _bits(b))
    assert len(c) != len(a) or not np.array_equal(_bits(a), _bits(c))


def test_survivor_noise_does_not_depend_on_the_density_stage(scene):
    kw = dict(noise_std=0.05, dense_ratio=0.9, region_size=2.0)
    r1 = R.perturb(scene, seed=SEED, sparse_ratio=0.3, **kw)
    r2 = R.perturb(scene, seed=SEED, sparse_ratio=0.6, **kw)
    with _engine() as eng:
        o1 = _run(eng, scene, dict(sparse_ratio=0.3, **kw))
        o2 = _run(eng, scene, dict(sparse_ratio=0.6, **kw))
    assert len(o1) == r1["n_kept"] and len(o2) == r2["n_kept"] and len(o1) < len(o2)
    common, i1, i2 = np.intersect1d(r1["src_index"], r2["src_index"], return_indices=True)
    assert len(common) > len(scene) // 4
    assert np.array_equal(_bits(o1[i1]), _bits(o2[i2]))


def test_source_slot_is_untouched(scene):
    kw = _cases(scene)["all"]
    with _engine() as eng:
        eng.upload(GT, scene, cell_size=NN_RADIUS)
        eng.mme(GT, NN_RADIUS, 5, per_point=False)
        before = eng.download(GT)
        e0, v0 = eng.mme_fetch(GT)
        eng.perturb(EST, GT, seed=SEED, **kw)
        assert np.array_equal(_bits(eng.download(GT)), _bits(before))
        e1, v1 = eng.mme_fetch(GT)
        assert np.array_equal(_bits(e0), _bits(e1)) and np.array_equal(v0, v1)
        assert np.array_equal(_bits(before), _bits(scene))


def _scalars(o):
    vals = []
    for st in (o.est_gt, o.gt_est):
        vals += [st.n_src, st.n_corr, st.mean_nn_dist] + [getattr(st, f)[k] for f in ("mean", "rmse", "fitness", "sigma", "number")
                                                          for k in range(5)]
    vals += [o.full_chamfer, o.mme_est, o.mme_gt, o.mme_est_valid, o.mme_gt_valid, o.awd, o.scs, o.n_w_voxels]
    return np.array([float(v) for v in vals])


def _param():
    from cloud_map_evaluation_amd.engine import Param

    return Param(icp_max_distance_=1.0, nn_radius_=NN_RADIUS, vmd_voxel_size_=3.0)


def test_suite_on_the_resident_result_equals_the_suite_from_its_download(scene):
    kw = _cases(scene)["all"]
    p = _param()
    with _engine() as eng:
        eng.upload(GT, scene, cell_size=NN_RADIUS)
        eng.perturb(EST, GT, seed=SEED, **kw)
        est = eng.download(EST)
        a = eng.run_suite(p)
    with _engine() as eng:
        b = eng.run_suite_from(est, scene, p, overlap=True)
    sa, sb = _scalars(a), _scalars(b)
    assert np.array_equal(_bits(sa), _bits(sb)), np.nonzero(sa != sb)


def test_a_perturb_plus_suite_costs_one_index_build(scene):
    """A sweep level on resident clouds (perturb + suite) indexes the new map once and nothing else: the same index-build launches
    ("morton", "sort") as handing the suite that map by a fresh upload of its download."""
    kw = _cases(scene)["all"]
    p = _param()
    keys = ("morton", "sort")
    with _engine() as eng:
        eng.upload(GT, scene, cell_size=NN_RADIUS)
        eng.perturb(EST, GT, seed=SEED, **kw)
        eng.run_suite_from(None, None, p, overlap=False)  # (warm: the ground truth's products exist)
        eng.timers_enable(True)
        eng.timers_reset()
        eng.perturb(EST, GT, seed=SEED + 1, **kw)
        d_perturb = {k: eng.timer(k)[1] for k in keys + ("perturb",)}
        eng.run_suite_from(None, None, p, overlap=False)
        d_sweep = {k: eng.timer(k)[1] for k in keys}
        est = eng.download(EST)
        eng.timers_reset()
        eng.upload(EST, est, cell_size=NN_RADIUS)
        d_upload = {k: eng.timer(k)[1] for k in keys}
        eng.run_suite_from(None, None, p, overlap=False)
        d_upload_suite = {k: eng.timer(k)[1] for k in keys}
    assert d_perturb["perturb"] == 1 and d_perturb["morton"] == 1
    assert {k: d_perturb[k] for k in keys} == d_upload, (d_perturb, d_upload)  # one cloud's index build
    assert d_sweep == d_upload_suite, (d_sweep, d_upload_suite)                  # ... and the suite rebuilds nothing on top


def test_errors(scene):
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import MapEvalError

    small = scene[:20_000]
    with _engine() as eng:
        eng.upload(GT, small, cell_size=NN_RADIUS)
        for bad in (dict(sparse_ratio=1.5), dict(dense_ratio=-0.1), dict(outlier_ratio=2.0), dict(noise_std=-1.0),
                    dict(outlier_range=-1.0), dict(sparse_ratio=float("nan")), dict(noise_std=float("inf"))):
            with pytest.raises(MapEvalError, match=r"\[-1\]"):
                eng.perturb(EST, GT, **bad)
        with pytest.raises(MapEvalError, match="no point"):  # the density stage dropped everything
            eng.perturb(EST, GT, sparse_ratio=0.0, dense_ratio=0.0, region_size=1.0)
        n = C.c_int64(-5)
        assert eng._L.me_perturb_cloud(eng._ctx, EST, GT, None, C.byref(n)) == -1
        assert b"NULL" in eng._L.me_last_error(eng._ctx) and n.value == -5
        pp = _lib.PerturbParams(sparse_ratio=1.0, dense_ratio=1.0)
        assert eng._L.me_perturb_cloud(eng._ctx, 2, GT, C.byref(pp), C.byref(n)) == -1
        assert eng._L.me_perturb_cloud(eng._ctx, EST, EST, C.byref(pp), C.byref(n)) == -3  # EST was never uploaded
        # a refused call leaves nothing behind: the source is intact, a good call still works
        assert eng.perturb(EST, GT, noise_std=0.01) == len(small)
        eng.set_slab(0, -1e9, 1e9, 1.0)
        with pytest.raises(MapEvalError, match="slab"):
            eng.perturb(EST, GT, noise_std=0.01)
        eng.set_slab(-1)
        eng.set_shard(0, 2)
        with pytest.raises(MapEvalError, match="shard"):
            eng.perturb(EST, GT, noise_std=0.01)
        eng.set_shard(0, 1)
        assert eng.perturb(EST, GT, noise_std=0.01) == len(small)


def test_timing_50m():
    import torch

    from cloud_map_evaluation_amd import synth

    src = synth.campus_scene(50_000_000, seed=5, device="cuda")
    kw = dict(noise_std=0.05, sparse_ratio=0.5, dense_ratio=0.9, region_size=2.0, outlier_ratio=0.05, outlier_range=1.0,
              deform_radius=20.0, deform_strength=0.3, deform_center=tuple(src.mean(dim=0).tolist()))
    with _engine() as eng:
        eng.upload(GT, src, cell_size=NN_RADIUS)
        del src
        torch.cuda.empty_cache()
        eng.perturb(EST, GT, seed=1, **kw)
        eng.timers_enable(True)
        for noise_only in (False, True):
            eng.timers_reset()
            t0 = time.perf_counter()
            reps = 3
            for r in range(reps):
                n = eng.perturb(EST, GT, seed=r, **({"noise_std": 0.05} if noise_only else kw))
            wall = (time.perf_counter() - t0) * 1e3 / reps
            ms, cnt = eng.timer("perturb")
            print(f"\n50 M points, {'noise only' if noise_only else 'all four stages'}: perturb passes {ms / cnt:.3f} ms (device), "
                  f"call incl. the index build {wall:.1f} ms, {n} points out")
