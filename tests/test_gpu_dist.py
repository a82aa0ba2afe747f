"""Distributed-input multi-GPU step (north-star shape) exercised on ONE GPU.

1. the device primitives against numpy: the multi-split of the halo exchange (me_halo_pack_device), the exact transform on
   a raw buffer, the Chan merge of voxel partial rows (me_voxel_merge_device) against the single-context table;
2. the real driver (cloud_map_evaluation_amd.dist.suite_step_dist) with TWO processes sharing this GPU, each starting with
   half of each (shuffled) cloud, gloo collectives on the CPU — the code path the 8-GPU run takes with RCCL — against the oracle;
3. a one-rank `nccl` group with ME_FORCE_COLLECTIVES=1: every collective of the step (all-to-all included) through RCCL on
   device tensors must reproduce the plain single-GPU step.
"""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TRUNC = (0.2, 0.1, 0.08, 0.05, 0.01)


def _scene(n=120_000):
    from cloud_map_evaluation_amd import synth

    est, gt = synth.campus_pair(n, density=2500.0, seed=5, origin=(100.0, -50.0, 3.0))
    return est.numpy(), gt.numpy()


def test_halo_pack_is_the_numpy_multi_split():
    import torch

    from cloud_map_evaluation_amd.engine import Engine

    rng = np.random.default_rng(3)
    p = rng.uniform(-5, 5, (300_001, 3))
    cuts = [-np.inf, -2.5, -2.4, 0.7, 3.0, np.inf]  # one very thin slab: its halo reaches over several neighbours
    dev = torch.device("cuda", 0)
    with Engine(0) as eng:
        for axis, halo in ((0, 0.3), (2, 0.0), (1, 1.5)):
            out, counts = eng.halo_pack(torch.from_numpy(p).to(dev), axis, cuts, halo)
            v = p[:, axis]
            exp = [p[(v >= cuts[k] - halo) & (v < cuts[k + 1] + halo)] for k in range(5)]
            assert counts == [len(e) for e in exp]
            assert np.array_equal(out.cpu().numpy(), np.concatenate(exp))  # destination-major, input order inside a destination
            if halo == 0.0:
                assert sum(counts) == len(p)  # without a halo the slabs partition the cloud
        out, counts = eng.halo_pack(torch.zeros((0, 3), dtype=torch.float64, device=dev), 0, cuts, 0.5)
        assert counts == [0] * 5 and out.shape == (0, 3)
        out, counts = eng.halo_pack(torch.from_numpy(p[:77]).to(dev), 1, [-np.inf, np.inf], 0.5)
        assert counts == [77] and np.array_equal(out.cpu().numpy(), p[:77])


def test_lattice_histograms_and_the_plan_they_give_against_numpy_and_halo_pack():
    """me_lattice_histograms_device == its numpy restatement (tests/test_dist_gloo.py) on ragged inputs — negative coordinates, points
    ON bin edges, extents that force a coarser level, -inf / +inf / NaN, an empty buffer — and the lean exchange's promise on the
    device: the per-destination counts lattice_plan predicts from the histograms are what me_halo_pack_device packs with the plan's cuts."""
    import torch

    from cloud_map_evaluation_amd import dist as medist
    from cloud_map_evaluation_amd.engine import Engine
    from test_dist_gloo import numpy_lattice_histograms

    rng = np.random.default_rng(11)
    dev = torch.device("cuda", 0)
    w = 2.0 ** -6
    a = rng.uniform(-40, 90, (200_003, 3)) * [1, 0.2, 0.05]
    a[:5000] = np.round(a[:5000] / w) * w
    a[7, 0], a[8, 0], a[9, 0], a[10, 2] = -np.inf, np.inf, np.nan, -np.inf
    clouds = {"mixed": a, "huge": rng.uniform(-7000, 12000, (50_000, 3)), "empty": np.zeros((0, 3)), "one": np.array([[0.5, -0.25, 3.0]])}
    with Engine(0) as eng:
        for name, p in clouds.items():
            for e0 in (-4, -8, 1):
                level, origin, ninf, hist = eng.lattice_histograms(torch.from_numpy(p).to(dev), e0)
                l2, o2, n2, h2 = numpy_lattice_histograms(p, e0)
                assert (level, list(origin), list(ninf)) == (l2, list(o2), list(n2)), (name, e0)
                assert np.array_equal(hist.cpu().numpy(), h2.numpy()), (name, e0)
                assert int(hist.sum()) == int(np.isfinite(p).sum())
        # the two-piece form (what the step calls): the same rows, header included
        for pa, pb in ((clouds["mixed"], clouds["huge"]), (clouds["empty"], clouds["one"]), (clouds["one"], clouds["empty"])):
            ta, tb = torch.from_numpy(pa).to(dev), torch.from_numpy(pb).to(dev)
            got = eng.lattice_messages([ta, tb], -4).cpu().numpy()
            for row, p in zip(got, (pa, pb)):
                l2, o2, n2, h2 = numpy_lattice_histograms(p, -4)
                assert list(row[:8]) == [l2, *o2, len(p), *n2] and np.array_equal(row[8:], h2.numpy().reshape(-1))
            assert np.array_equal(eng.lattice_messages([ta], -4).cpu().numpy()[0], got[0])
        # four ranks' parts of two clouds -> plan -> what halo_pack really packs
        world, halo = 4, 0.3
        parts = [[torch.from_numpy(rng.uniform(-3, 9, (30_000 + 1000 * r, 3)) * [1, 0.3, 0.1]).to(dev) for _ in range(2)] for r in range(world)]
        e0 = medist.lattice_e0(halo)
        allm = torch.stack([medist.lattice_message(eng, pr, e0) for pr in parts])
        axis, cuts, halo_eff, counts, totals = medist.lattice_plan(allm, world, halo, e0)
        assert axis == 0 and halo <= halo_eff <= halo * 17 / 16 and totals == [sum(int(pr[c].shape[0]) for pr in parts) for c in range(2)]
        for r in range(world):
            for c in range(2):
                assert eng.halo_pack(parts[r][c], axis, cuts, halo_eff)[1] == [int(x) for x in counts[r][c]]
        # me_lattice_plan_device (what the step runs on the GPU) == dist.lattice_plan's torch form (what the CPU tests run), on ragged sets
        from test_dist_gloo import numpy_lattice_histograms as nlh  # noqa: F401

        def both(parts_np, world, halo):
            e0 = medist.lattice_e0(halo)
            allm = torch.stack([medist.lattice_message(eng, [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in pr], e0) for pr in parts_np])
            a = medist.lattice_plan(allm, world, halo, e0)
            b = medist.lattice_plan(allm, world, halo, e0, eng=eng)
            assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3]) and a[4] == b[4], (a[:3], b[:3])

        both([[p.cpu().numpy() for p in pr] for pr in parts], 4, 0.3)
        a = rng.uniform(0, 10, (2000, 3))
        a[5, 0], a[6, 0], a[7, 0], a[8, 1] = -np.inf, np.inf, np.nan, -np.inf
        both([[a, rng.uniform(0, 10, (1500, 3))], [np.zeros((0, 3)), rng.uniform(0, 10, (900, 3))], [rng.uniform(0, 10, (10, 3)), np.zeros((0, 3))],
              [np.zeros((0, 3)), np.zeros((0, 3))]], 4, 0.3)
        both([[rng.uniform(0, 60, (2000, 3)) + [0, 400.0 * r, 0], rng.uniform(0, 60, (2000, 3)) + [0, 400.0 * r, 0]] for r in range(8)], 8, 1.0)
        both([[rng.uniform(-4000, 9000, (3000, 3)), np.zeros((0, 3))] for _ in range(3)], 3, 0.11)   # no ground truth anywhere
        both([[np.tile([[1.0, 2.0, 3.0]], (500, 1)), np.tile([[1.0, 2.0, 3.0]], (400, 1))] for _ in range(5)], 5, 0.3)
        both([[rng.uniform(0, 5, (100, 3)), rng.uniform(0, 5, (80, 3))]], 1, 0.3)


def test_transform_points_device_is_the_upload_transform():
    import torch

    import oracle
    from cloud_map_evaluation_amd.engine import Engine

    est, _ = _scene(20_000)
    T = np.array([[0.999, -0.02, 0.01, 0.3], [0.02, 0.9995, 0.003, -0.2], [-0.01, -0.003, 0.9999, 0.05], [0, 0, 0, 1.0]])
    with Engine(0) as eng:
        got = eng.transform_points(torch.from_numpy(est).to("cuda:0"), T).cpu().numpy()
    assert np.array_equal(got, oracle.transform(est, T))  # Open3D's operation order, bit for bit


def test_voxel_merge_device_reproduces_the_whole_table():
    import torch

    from cloud_map_evaluation_amd import dist as medist
    from cloud_map_evaluation_amd.engine import Engine

    est, gt = _scene()
    world = 4
    with Engine(0) as eng:
        eng.upload(0, est, cell_size=0.1)
        eng.upload(1, gt, cell_size=0.1)
        whole = {s: eng.voxel_gaussians(s, 1.0) for s in (0, 1)}
        whole_v = eng.calculateVMD(1.0)
        axis, cuts = medist.dist_slab_cuts(torch.from_numpy(gt), None, torch.device("cpu"), world)
        rows = {0: [], 1: []}
        for rank in range(world):
            eng.set_slab(axis, cuts[rank], cuts[rank + 1], 0.5)
            eng.upload(0, est, cell_size=0.1)
            eng.upload(1, gt, cell_size=0.1)
            for s in (0, 1):
                r = eng.voxel_partial_rows(s, 1.0)
                # what the padded all-gather delivers: this rank's rows + padding rows (n == 0)
                rows[s].append(torch.cat([r, torch.zeros((7, 16), dtype=torch.float64, device=r.device)]))
        for s in (0, 1):
            eng.voxel_merge(s, 1.0, torch.cat(rows[s]))
        v = eng.calculateVMD(1.0)  # runs on the merged tables (the clouds are still in slab mode)
        eng.set_slab(-1)
        assert v["n_rows"] == whole_v["n_rows"] > 50 and v["counts"] == whole_v["counts"]
        np.testing.assert_allclose(v["awd"], whole_v["awd"], rtol=1e-10)
        np.testing.assert_allclose(v["scs"], whole_v["scs"], rtol=1e-10)
        from tests._tol import assert_voxel_rows_close

        assert_voxel_rows_close(v["rows"], whole_v["rows"], rtol=1e-8)
        assert np.array_equal(v["rows"][:, :6], whole_v["rows"][:, :6]) and np.array_equal(v["rows"][:, 10:12], whole_v["rows"][:, 10:12])
        # and the numpy restatement of the merge (dist.merge_voxel_partials, what the CPU stand-in of the gloo tests uses)
        for s in (0, 1):
            keys, n, mu, sig = medist.merge_voxel_partials(torch.cat(rows[s]).cpu().numpy())
            wk, wn, wmu, wsig, _ = whole[s]
            assert np.array_equal(keys, wk) and np.array_equal(n, wn)
            np.testing.assert_allclose(mu, wmu, rtol=1e-13)
        # an empty gather (a cloud nobody holds) leaves an empty table, not an error
        eng.voxel_merge(0, 1.0, torch.zeros((5, 16), dtype=torch.float64, device="cuda:0"))
        assert eng.calculateVMD(1.0)["n_rows"] == 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, est, gt, T, q, overlap, backend="gloo"):
    import torch
    import torch.distributed as dist

    from cloud_map_evaluation_amd import dist as medist
    from cloud_map_evaluation_amd.engine import Engine, Param

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if backend == "nccl":
        os.environ["ME_FORCE_COLLECTIVES"] = "1"  # one rank, but every collective of the step goes through RCCL
    if os.environ.get("ME_TEST_CROSS_CAP"):  # force the overflow path of the cross-rank message (lean step: the redo after the statistics gather)
        medist._CROSS_CAP = int(os.environ["ME_TEST_CROSS_CAP"])
    if os.environ.get("ME_TEST_VOX_CAP"):
        medist._VOX_CAP = int(os.environ["ME_TEST_VOX_CAP"])
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        P = Param(icp_max_distance_=1.0, nn_radius_=0.1, trunc_dist_=TRUNC, vmd_voxel_size_=1.0, initial_matrix_=T)
        dev = torch.device("cuda", 0)
        comm = dev if backend == "nccl" else torch.device("cpu")
        be, ee = medist.shard_range(len(est), rank, world)
        bg, eg = medist.shard_range(len(gt), rank, world)
        with Engine(0) as eng:
            res = medist.suite_step_dist(eng, dist, comm, torch.from_numpy(est[be:ee].copy()).to(dev),
                                         torch.from_numpy(gt[bg:eg].copy()).to(dev), P, rank, world, halo=0.5, overlap=overlap)
        q.put((rank, {k: (v if not isinstance(v, dict) else {kk: np.asarray(vv) for kk, vv in v.items()}) for k, v in res.items()}))
    finally:
        dist.destroy_process_group()


def _check_against_oracle(results, est, gt, T, world, min_cross):
    import oracle

    est_t = oracle.transform(est, T)
    o_eg = oracle.reg_stats(est_t, gt, 1.0, 0, TRUNC)
    o_ge = oracle.reg_stats(gt, est_t, 1.0, 0, TRUNC)
    o_me = oracle.mme(est_t, 0.1, 10)
    o_mg = oracle.mme(gt, 0.1, 5)
    o_v = oracle.awd_scs(oracle.VoxelMap(gt, 1.0), oracle.VoxelMap(est_t, 1.0))
    for rank in range(world):
        r = results[rank]
        assert r["n_est"] == len(est) and r["n_gt"] == len(gt)
        assert r["n_cross_rank_queries"] >= min_cross
        for got, exp in ((r["est_gt"], o_eg), (r["gt_est"], o_ge)):
            assert got["n_corr"] == exp.n_corr
            assert np.array_equal(got["number"], exp.number)          # bit-exact inlier counts
            for k in ("mean", "rmse", "sigma"):
                np.testing.assert_allclose(got[k], getattr(exp, k), rtol=1e-9)
        np.testing.assert_allclose(r["cd"], oracle.chamfer(est_t, gt), rtol=1e-9)
        assert r["mme_valid"] == o_me[3]
        np.testing.assert_allclose(r["mme_est"], o_me[0], rtol=1e-9)
        np.testing.assert_allclose(r["mme_gt"], o_mg[0], rtol=1e-9)
        assert r["n_w"] == len(o_v["rows"])
        np.testing.assert_allclose(r["awd"], o_v["awd"], rtol=1e-9)
        np.testing.assert_allclose(r["scs"], o_v["scs"], rtol=1e-9)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("overlap,variant", [(False, "lean"), (True, "lean"), (True, "lean_overflows"), (True, "classic")])
def test_two_process_distributed_suite_matches_oracle(overlap, variant, monkeypatch):
    """lean: the round-6 step (lattice plan -> halo all-to-all -> cross message gather, answered without a host read -> min-reduce ->
    statistics + voxel rows in one gather -> last all-reduce); lean_overflows: 16 open queries / 8 voxel rows per message, so that the
    exact-size cross-rank path AND the exact-size voxel gather run after the optimistic ones; classic: ME_DIST_LEAN=0, rounds 2 - 5."""
    import torch.multiprocessing as mp

    if variant == "lean_overflows":
        monkeypatch.setenv("ME_TEST_CROSS_CAP", "16")
        monkeypatch.setenv("ME_TEST_VOX_CAP", "8")
    if variant == "classic":
        monkeypatch.setenv("ME_DIST_LEAN", "0")

    est, gt = _scene(100_000)
    est = np.concatenate([est, est[:150] + np.array([2.0, 0.0, 30.0])])  # far points: the cross-rank 1-NN step
    rng = np.random.default_rng(9)
    est = est[rng.permutation(len(est))]
    T = np.eye(4)
    T[:3, 3] = [0.003, -0.002, 0.001]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, est, gt, T, q, overlap)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=500) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    _check_against_oracle(results, est, gt, T, 2, 100)


@pytest.mark.timeout(600)
def test_four_process_lean_step_matches_oracle():
    """Four ranks sharing this GPU (gloo): three cuts, a count matrix of 4 x 2 x 4, slabs whose halo reaches more than one neighbour
    where the scene is thin — the lean step's plan at a world size the two-process test cannot show."""
    import torch.multiprocessing as mp

    est, gt = _scene(100_000)
    est = np.concatenate([est, est[:150] + np.array([2.0, 0.0, 30.0])])
    rng = np.random.default_rng(19)
    est, gt = est[rng.permutation(len(est))], gt[rng.permutation(len(gt))]
    T = np.eye(4)
    T[:3, 3] = [0.003, -0.002, 0.001]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 4, port, est, gt, T, q, True)) for r in range(4)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=500) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    _check_against_oracle(results, est, gt, T, 4, 100)


@pytest.mark.timeout(600)
def test_one_rank_distributed_step_through_rccl_matches_oracle_and_plain_step():
    """One GPU: the RCCL calls cannot cross ranks, but a one-rank `nccl` group with ME_FORCE_COLLECTIVES=1 still sends the
    all-reduces, the all-to-alls and the all-gathers of the step through RCCL on device tensors."""
    import torch
    import torch.multiprocessing as mp

    from cloud_map_evaluation_amd import dist as medist
    from cloud_map_evaluation_amd.engine import Engine, Param

    est, gt = _scene(60_000)
    T = np.eye(4)
    T[:3, 3] = [0.003, -0.002, 0.001]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(0, 1, _free_port(), est, gt, T, q, True, "nccl"))
    p.start()
    rank, r = q.get(timeout=500)
    p.join(timeout=60)
    assert p.exitcode == 0 and rank == 0
    _check_against_oracle({0: r}, est, gt, T, 1, 0)
    # the plain single-GPU step (no slabs, no process group): counts identical, sums to rounding
    P = Param(icp_max_distance_=1.0, nn_radius_=0.1, trunc_dist_=TRUNC, vmd_voxel_size_=1.0, initial_matrix_=T)
    with Engine(0) as eng:
        ref = medist.suite_step(eng, None, torch.device("cuda", 0), est, gt, P, overlap=True)
    assert r["mme_valid"] == ref["mme_valid"] and r["n_w"] == ref["n_w"]
    for d in ("est_gt", "gt_est"):
        assert np.array_equal(np.asarray(r[d]["number"]), np.asarray(ref[d]["number"]))
    for k in ("cd", "mme_est", "mme_gt", "awd", "scs"):
        np.testing.assert_allclose(r[k], ref[k], rtol=1e-12)


@pytest.mark.timeout(900)
def test_bench_py_two_rank_path_runs_end_to_end():
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one process per rank), with both ranks on this one
    GPU and gloo collectives (test hooks; RCCL refuses two ranks on a device): the line it prints must carry the contract's
    fields and the same scalars as the single-GPU run of the same workload."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--workload", "campus", "--points", "400000", "--steps", "2", "--warmup", "1", "--full", "--cpu-baseline", "off", "--no-h2d"]
    env = dict(os.environ, ME_BENCH_BACKEND="gloo", ME_BENCH_SINGLE_DEVICE="1")
    for attempt in range(3):  # (a rendezvous can fail on a busy box — port taken between probe and bind; the RESULTS are never retried)
        r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                             "127.0.0.1", "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                            capture_output=True, text=True, timeout=800, env=env, cwd=root)
        if r2.returncode == 0:
            break
    assert r2.returncode == 0, r2.stdout[-1500:] + r2.stderr[-3000:]
    line2 = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][-1])
    r1 = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common, capture_output=True, text=True, timeout=800, cwd=root)
    assert r1.returncode == 0, r1.stderr[-3000:]
    line1 = json.loads([l for l in r1.stdout.splitlines() if l.startswith("{")][-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in line2, k
    assert line2["n_gpus"] == 2 and line1["n_gpus"] == 1 and line2["scaling"] == "strong" and line2["steps"] == 2
    assert line2["config"]["n_est"] == line1["config"]["n_est"] == 400000  # the whole job's size, not a rank's share
    ra, rb = line1["results"], line2["results"]
    assert ra["MME_valid"] == rb["MME_valid"] and ra["W_voxels"] == rb["W_voxels"]
    assert ra["COM"] == rb["COM"]  # inlier counts / N: bit-exact across the two drivers
    for k in ("CD", "MME_est", "MME_gt", "AWD", "SCS"):
        np.testing.assert_allclose(rb[k], ra[k], rtol=1e-9)
    np.testing.assert_allclose(rb["AC"], ra["AC"], rtol=1e-9)


def test_prefiltered_slab_upload_equals_filtered_upload_and_copes_with_an_empty_slab():
    """me_upload_slab_device (what the distributed step uses for the points the exchange delivered) against the filtering
    upload on the same slab; and a rank whose slab holds nothing of a cloud."""
    import torch

    from cloud_map_evaluation_amd.engine import Engine

    est, gt = _scene(60_000)
    dev = torch.device("cuda", 0)
    lo, hi, halo = float(np.quantile(gt[:, 0], 0.3)), float(np.quantile(gt[:, 0], 0.6)), 0.5
    with Engine(0) as eng:
        eng.set_slab(0, lo, hi, halo)
        eng.upload(0, est, cell_size=0.1)
        eng.upload(1, gt, cell_size=0.1)
        a = (eng.mme(0, 0.1, 10, per_point=False)[3:], eng.size(0), eng.size(1))
        eng.nn1(0, 1, fetch=False)
        pa = eng.nn_partial_sums(0, 1.0, 0, TRUNC)
        keep = lambda p: torch.from_numpy(p[(p[:, 0] >= lo - halo) & (p[:, 0] < hi + halo)]).to(dev)
        eng.upload_slab(0, keep(est), cell_size=0.1)
        eng.upload_slab(1, keep(gt), cell_size=0.1)
        b = (eng.mme(0, 0.1, 10, per_point=False)[3:], eng.size(0), eng.size(1))
        eng.nn1(0, 1, fetch=False)
        pb = eng.nn_partial_sums(0, 1.0, 0, TRUNC)
        assert a == b and pa.n_corr == pb.n_corr and list(pa.n_inl) == list(pb.n_inl) and pa.sum_sqrt_all == pb.sum_sqrt_all
        # nothing of the map in this rank's slab
        eng.upload_slab(0, torch.zeros((0, 3), dtype=torch.float64, device=dev), cell_size=0.1)
        assert eng.size(0) == 0 and eng.mme(0, 0.1, 10, per_point=False)[3:] == (0, 0.0)
        eng.nn1(0, 1, fetch=False)
        assert eng.nn_partial_sums(0, 1.0, 0, TRUNC).n_corr == 0 and eng.nn_unresolved_count(0) == 0
        eng.nn1(1, 0, fetch=False)  # every owned ground-truth point is unresolved: its neighbour lives on another rank
        assert eng.nn_unresolved_count(1) > 0
        assert eng.voxel_partial_rows(0, 1.0).shape == (0, 16)
        eng.set_slab(-1)
