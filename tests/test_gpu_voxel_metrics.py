"""me_voxel_metrics on the GPU: the per-voxel AC / COM / CD / MME sums against the device's own per-point products grouped in numpy,
against the CPU oracle, their invariants (rows add up to me_nn_partial_sums and the MME), hand-built edge cases, errors, determinism,
a 20 M + 20 M pair, and the host's voxel_metrics.txt."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _voxel_metrics_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

EST, GT = 0, 1
LE, LT = 0, 1
TRUNC = (0.2, 0.1, 0.08, 0.05, 0.01)
EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")


def _rot_T():
    T = np.eye(4)
    th = 0.01
    T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    T[:3, 3] = [0.05, -0.03, 0.02]
    return T


@pytest.fixture(scope="module")
def pair():
    from cloud_map_evaluation_amd import synth

    est, gt = synth.multisession_pair(400_000, 3, density=2500.0, seed=11)
    return est.numpy(), gt.numpy()


def _param(T, vs=3.0):
    from cloud_map_evaluation_amd.engine import Param

    return Param(icp_max_distance_=1.0, nn_radius_=0.2, vmd_voxel_size_=vs, initial_matrix_=T)


def _check_sums(eng, slot, got, gate, mode, trunc):
    tot = eng.nn_partial_sums(slot, gate, mode, trunc)
    assert got["n_query"].sum() == tot.n_query == eng.size(slot)
    assert got["n_corr"].sum() == tot.n_corr
    assert list(got["n_inl"].sum(axis=0)) == list(tot.n_inl)
    np.testing.assert_allclose(got["sum_d"].sum(axis=0), list(tot.sum_d), rtol=1e-12)
    np.testing.assert_allclose(got["sum_d2"].sum(axis=0), list(tot.sum_d2), rtol=1e-12)
    np.testing.assert_allclose(got["sum_sqrt_all"].sum(), tot.sum_sqrt_all, rtol=1e-12)


@pytest.mark.parametrize("identity", [True, False])
def test_rows_equal_the_grouped_device_products_and_add_up(pair, identity):
    from cloud_map_evaluation_amd.engine import Engine

    est, gt = pair
    T = np.eye(4) if identity else _rot_T()
    with Engine(0) as eng:
        out = eng.run_suite_from(est, gt, _param(T), overlap=True)
        xyz = [eng.download(EST), eng.download(GT)]  # the map in the transformed frame
        d2 = [eng.nn_fetch(EST)[1], eng.nn_fetch(GT)[1]]
        mme = [eng.mme_fetch(EST), eng.mme_fetch(GT)]
        cases = [(3.0, 1.0, LE, TRUNC), (0.5, 1.0, LT, TRUNC), (7.0, 0.3, LE, (0.2, 0.1, 0.08, 0.5, 1.5)),
                 (3.0, 0.3, LT, (2.0, 0.1, 0.08, 0.05, 0.01))]  # (trunc levels above the gate: only gated points count)
        for vs, gate, mode, trunc in cases:
            for slot in (EST, GT):
                got = eng.voxel_metrics(slot, vs, gate, mode, trunc)
                assert got["have_mme"]
                want = ref.group(xyz[slot], d2[slot], vs, gate, mode, trunc, mme[slot][0], mme[slot][1])
                ref.assert_rows_equal(got, want, rtol=1e-12)
                keys, n, *_ = eng.voxel_gaussians(slot, vs)  # the rows of the voxel table, key for key
                np.testing.assert_array_equal(got["keys"], keys)
                np.testing.assert_array_equal(got["n_query"], n)
                _check_sums(eng, slot, got, gate, mode, trunc)
                nv = out.mme_est_valid if slot == EST else out.mme_gt_valid
                assert got["n_H"].sum() == nv
                mean = out.mme_est if slot == EST else out.mme_gt
                np.testing.assert_allclose(got["sum_H"].sum() / got["n_H"].sum(), mean, rtol=1e-12)


def test_rows_against_the_oracle(pair):
    import oracle
    from cloud_map_evaluation_amd.engine import Engine

    est, gt = pair
    T = _rot_T()
    est_t = oracle.transform(est, T)
    vs = 3.0
    with Engine(0) as eng:
        eng.run_suite_from(est, gt, _param(T, vs), overlap=True)
        got = [eng.voxel_metrics(s, vs, 1.0, LE, TRUNC) for s in (EST, GT)]
    # 1-NN of the oracle's KD-tree, entropies of oracle.mme on the clouds as loaded (the map before its transform, map_eval.cpp:56)
    d2e = oracle.nn1(gt, est_t)[1]
    d2g = oracle.nn1(est_t, gt)[1]
    me = oracle.mme(est, 0.2, 10)
    mg = oracle.mme(gt, 0.2, 5)
    for g, xyz, d2, m in ((got[0], est_t, d2e, me), (got[1], gt, d2g, mg)):
        want = ref.group(xyz, d2, vs, 1.0, LE, TRUNC, m[1], m[2])
        ref.assert_rows_equal(g, want, rtol=1e-9)


def _two(eng, est, gt, cell=0.5):
    eng.upload(EST, est, cell_size=cell)
    eng.upload(GT, gt, cell_size=cell)
    eng.nn1(EST, GT, fetch=False)
    eng.nn1(GT, EST, fetch=False)


def test_hand_built_edge_cases():
    from cloud_map_evaluation_amd.engine import Engine

    rng = np.random.default_rng(3)
    with Engine(0) as eng:
        # one voxel, no MME run: have_mme == 0 and zero entropy columns
        est = rng.uniform(0.05, 0.95, (5000, 3))
        gt = rng.uniform(0.05, 0.95, (5000, 3))
        _two(eng, est, gt)
        got = eng.voxel_metrics(EST, 1.0, 0.5, LE, TRUNC)
        assert got["keys"].tolist() == [[0, 0, 0]] and got["n_query"].tolist() == [5000]
        assert not got["have_mme"] and got["n_H"].tolist() == [0] and got["sum_H"].tolist() == [0.0]
        _check_sums(eng, EST, got, 0.5, LE, TRUNC)
        # points exactly on voxel faces and negative coordinates; a far cluster whose voxels have no gated correspondence
        vs = 0.25
        grid = np.stack(np.meshgrid(*[np.arange(-8, 8) * vs] * 3, indexing="ij"), -1).reshape(-1, 3)
        far = rng.uniform(-30.0, -29.0, (2000, 3))
        est = np.concatenate([grid, grid + rng.normal(0, 0.01, grid.shape), far])
        gt = np.concatenate([grid * 1.0, rng.uniform(-2.0, 2.0, (3000, 3))])
        _two(eng, est, gt)
        for slot, xyz in ((EST, est), (GT, gt)):
            got = eng.voxel_metrics(slot, vs, 0.5, LT, TRUNC)
            want = ref.group(xyz, eng.nn_fetch(slot)[1], vs, 0.5, LT, TRUNC)
            ref.assert_rows_equal(got, want)
            keys, n, *_ = eng.voxel_gaussians(slot, vs)
            np.testing.assert_array_equal(got["keys"], keys)
            np.testing.assert_array_equal(got["n_query"], n)
        got = eng.voxel_metrics(EST, vs, 0.5, LT, TRUNC)
        lonely = got["keys"][:, 0] < -100
        assert lonely.any() and np.all(got["n_corr"][lonely] == 0) and np.all(got["n_query"][lonely] > 0)
        assert np.all(got["sum_d"][lonely] == 0) and np.all(got["sum_sqrt_all"][lonely] > 0)
        assert (got["keys"] < 0).any()


def test_errors_capacity_and_slab_mode():
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import Engine, MapEvalError

    rng = np.random.default_rng(5)
    est, gt = rng.uniform(-3, 3, (20000, 3)), rng.uniform(-3, 3, (20000, 3))
    tr = np.ascontiguousarray(TRUNC, np.float64)
    with Engine(0) as eng:
        eng.upload(EST, est, cell_size=0.5)
        eng.upload(GT, gt, cell_size=0.5)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):  # no me_nn1 with this slot as the query
            eng.voxel_metrics(EST, 1.0, 0.5, LE, TRUNC)
        eng.nn1(EST, GT, fetch=False)
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            eng.voxel_metrics(GT, 1.0, 0.5, LE, TRUNC)
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):
            eng.voxel_metrics(EST, 0.0, 0.5, LE, TRUNC)
        with pytest.raises(MapEvalError, match=r"^\[-1\]"):  # keys outside the packed range
            eng.voxel_metrics(EST, 1e-6, 0.5, LE, TRUNC)
        V = eng.voxel_metrics(EST, 1.0, 0.5, LE, TRUNC)["keys"].shape[0]
        assert V == 216
        L = _lib.load()
        keys = np.empty((V, 3), np.int32)
        nv = C.c_int64(V - 1)
        hm = C.c_int(-1)
        rc = L.me_voxel_metrics(eng._ctx, EST, 1.0, 0.5, LE, tr.ctypes.data, keys.ctypes.data, 0, 0, 0, C.byref(hm), C.byref(nv))
        assert rc == _lib.ME_ERR_CAPACITY and nv.value == V and hm.value == 0
        eng.upload(EST, est, cell_size=0.5)  # a new upload discards the 1-NN result
        with pytest.raises(MapEvalError, match=r"^\[-3\]"):
            eng.voxel_metrics(EST, 1.0, 0.5, LE, TRUNC)
    with Engine(0) as eng:
        eng.set_slab(0, -1.0, 1.0, 0.5)
        _two(eng, est, gt)
        with pytest.raises(MapEvalError, match=r"^\[-3\].*slab"):
            eng.voxel_metrics(EST, 1.0, 0.5, LE, TRUNC)


def _bits(d):
    return {k: (v.view(np.int64) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for k, v in d.items()}


def test_bit_identical_across_calls_and_lanes(pair):
    from cloud_map_evaluation_amd.engine import Engine

    est, gt = pair
    res = []
    for overlap in (True, False):
        with Engine(0) as eng:
            eng.run_suite_from(est, gt, _param(_rot_T()), overlap=overlap)
            for _ in range(2):
                res.append([_bits(eng.voxel_metrics(s, 3.0, 1.0, LE, TRUNC)) for s in (EST, GT)])
    for r in res[1:]:
        for a, b in zip(res[0], r):
            assert a.keys() == b.keys()
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_full_size_20m_pair():
    import torch

    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine

    est, gt = synth.multisession_pair(20_000_000, 3, density=2500.0, seed=100, device="cuda")
    vs = 3.0
    with Engine(0) as eng:
        eng.run_suite_from(est, gt, _param(np.eye(4), vs), overlap=True)
        del est, gt
        torch.cuda.empty_cache()
        eng.voxel_metrics(EST, vs, 1.0, LE, TRUNC)  # (warm: first-call allocations)
        t0 = time.perf_counter()
        got = [eng.voxel_metrics(s, vs, 1.0, LE, TRUNC) for s in (EST, GT)]
        dt = time.perf_counter() - t0
        assert dt < 10.0, f"two 20 M-point voxel_metrics calls took {dt:.2f} s"
        for slot, g in zip((EST, GT), got):
            want = ref.group(eng.download(slot), eng.nn_fetch(slot)[1], vs, 1.0, LE, TRUNC, *eng.mme_fetch(slot))
            np.testing.assert_array_equal(g["keys"], want["keys"])
            for f in ref.INT_FIELDS:
                np.testing.assert_array_equal(g[f], want[f], err_msg=f)
            np.testing.assert_allclose(g["sum_sqrt_all"], want["sum_sqrt_all"], rtol=1e-9)
            _check_sums(eng, slot, g, 1.0, LE, TRUNC)


# ---- the host executable -----------------------------------------------------------------------------------------------
def _write_pcd(path, pts):
    n = len(pts)
    hdr = (f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH {n}\nHEIGHT 1\n"
           f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())


def _cfg(est_dir, gt_path, T, initial=True, key=None):
    rows = "\n".join("  - [" + ", ".join(repr(float(v)) for v in T[i]) + "]" for i in range(4))
    extra = "" if key is None else f"save_voxel_metrics: {'true' if key else 'false'}\n"
    return f"""registration_methods: 0
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix:
{rows}
estimate_map_path: {est_dir}
gt_map_path: {gt_path}
scene_name: vm
save_immediate_result: true
evaluate_mme: true
use_tbb_mme: true
evaluate_gt_mme: true
nn_radius: 0.1
evaluate_using_initial: {'true' if initial else 'false'}
evaluate_noise_gt: false
vmd_voxel_size: 0.5
downsample_size: 0.0
use_visualization: false
enable_debug: false
""" + extra


def _run_host(tmp_path, name, est, gt, T, initial, key):
    d = tmp_path / name
    est_dir = d / "est"
    est_dir.mkdir(parents=True)
    _write_pcd(est_dir / "map.pcd", est)
    _write_pcd(d / "gt.pcd", gt)
    (d / "config.yaml").write_text(_cfg(est_dir, d / "gt.pcd", T, initial, key))
    r = subprocess.run([EXE, str(d / "config.yaml")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return est_dir / "map_results"


def _folder(path):
    out = {}
    for f in sorted(os.listdir(path)):
        data = open(path / f, "rb").read().replace(str(path.parent.parent).encode(), b"<run>")  # (each run has its own folder)
        if f == "map_results.txt":  # (the header's date and the timing lines differ from run to run)
            data = b"\n".join(l for l in data.split(b"\n") if b"=====================" not in l and b"Time" not in l)
        out[f] = data
    return out


@pytest.mark.parametrize("initial", [True, False])
def test_host_writes_the_joined_table(tmp_path, initial):
    from cloud_map_evaluation_amd import synth
    from cloud_map_evaluation_amd.engine import Engine, Param

    assert os.path.exists(EXE), "build the host first (__graft_entry__.build())"
    est, gt = synth.cube_pair(100_000, seed=42)
    est, gt = est.numpy(), gt.numpy()
    T = np.eye(4)
    T[:3, 3] = [0.004, -0.002, 0.001]
    with_key = _run_host(tmp_path, "on", est, gt, T, initial, True)
    tab = np.loadtxt(with_key / "voxel_metrics.txt")
    assert tab.ndim == 2 and tab.shape[1] == 44
    assert tab[:, 3].sum() == len(est) and tab[:, 4].sum() == len(gt)
    if initial:  # the one-call path: equal to the Python joined table of the same pass, number for number
        with Engine(0) as eng:
            eng.run_suite_from(est, gt, Param(icp_max_distance_=1.0, nn_radius_=0.1, vmd_voxel_size_=0.5, initial_matrix_=T))
            want = eng.voxel_metrics_table(0.5, 1.0, LE, TRUNC)
        np.testing.assert_array_equal(tab, want)
    else:  # the registration path: the rows add up to the statistics and the entropies the host wrote
        txt = open(with_key / "map_results.txt").read()
        comp = [float(v) for v in txt.split("Comp: ")[1].split("\n")[0].split()]
        np.testing.assert_allclose(tab[:, 6:11].sum(axis=0) / len(est), comp, rtol=0, atol=2e-15)
        ent = np.loadtxt(with_key / "map_entropy.txt")
        assert tab[:, 39].sum() == ent[:, 1].sum() > 0
        h = ent[ent[:, 1] > 0, 0]  # (written with six significant digits)
        np.testing.assert_allclose(tab[:, 40].sum(), h.sum(), rtol=0, atol=1e-5 * np.abs(h).sum())
        assert tab[:, 41].sum() > 0
    # without the key (absent, or explicitly false): the same files with the same bytes; with it: voxel_metrics.txt besides
    off = _folder(_run_host(tmp_path, "off", est, gt, T, initial, False))
    absent = _folder(_run_host(tmp_path, "absent", est, gt, T, initial, None))
    assert off == absent
    on = _folder(with_key)
    assert set(on) == set(off) | {"voxel_metrics.txt"}
    for f in off:
        assert on[f] == off[f], f
