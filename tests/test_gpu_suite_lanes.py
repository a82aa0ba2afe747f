"""me_run_suite_from with device input: the two-lane schedule whose second lane queues the tail of the ground truth's index build
(gather, level histogram, block counts, scans, cell tables) on a priority stream and builds the map's octree (csrc/me_suite.hip,
csrc/me_index.hip: IndexTail) — against the single-lane call, EXACTLY: every scalar and both directions' five-level vectors.

Nothing arithmetic differs between the two schedules, so any difference is a race.  The shapes are the ones at which the
cross-stream ordering can go wrong: a map that is over long before the ground truth is indexed (the main lane truly waits), the
reverse (indexed before the map's MME is queued), ground truths below / at / just above one 2048-point block of the cell kernels,
pairs of changing sizes back to back on one fresh engine (a table left by the previous pair must not hide a read before write: the
previous pair is never the same cloud), a pair with thin neighbourhoods (k_mme_refine runs between the two MMEs), and a second lane
that fails.  Clouds: seeded synth cubes, device-resident (the priority stream is used for device input only)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VEC = ("mean", "rmse", "fitness", "sigma", "number")
SCALARS = ("full_chamfer", "mme_est", "mme_gt", "mme_est_valid", "mme_gt_valid", "awd", "scs", "n_w_voxels")


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda", 0)


@pytest.fixture()
def eng(dev):
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _param():
    from cloud_map_evaluation_amd.engine import Param

    return Param(icp_max_distance_=1.0, nn_radius_=0.1, vmd_voxel_size_=0.5)


def _cube(n, seed, dev, which, scale=0.5):
    """which: 0 the noisy copy, 1 the surface sample of synth.cube_pair; scaled so that nn_radius 0.1 finds its neighbours."""
    import torch

    from cloud_map_evaluation_amd import synth

    return (synth.cube_pair(n, seed=seed)[which] * scale).to(torch.float64).contiguous().to(dev)


def _same(a, b):
    for k in SCALARS:
        assert getattr(a, k) == getattr(b, k), k
    for side in ("est_gt", "gt_est"):
        x, y = getattr(a, side), getattr(b, side)
        assert x.n_src == y.n_src and x.n_corr == y.n_corr and x.mean_nn_dist == y.mean_nn_dist, side
        for k in VEC:
            assert list(getattr(x, k)) == list(getattr(y, k)), (side, k)


def _single_lane(est, gt, P):
    """The pair through a fresh engine, one lane."""
    from cloud_map_evaluation_amd.engine import Engine

    with Engine(0) as e:
        return e.run_suite_from(est, gt, P, overlap=False)


@pytest.mark.parametrize("n_est,n_gt", [(20_000, 600_000), (600_000, 20_000)])
def test_unequal_clouds(eng, dev, n_est, n_gt):
    """20 k vs 600 k: the map's MME has ended before the ground truth's gather starts — the main lane waits for the cell tables, and for
    the map's octree, which the second lane builds after them.  600 k vs 20 k: the ground truth is indexed, and both octrees exist,
    before the map's MME is queued."""
    est, gt = _cube(n_est, 3, dev, 0), _cube(n_gt, 4, dev, 1)
    P = _param()
    want = _single_lane(est, gt, P)
    assert want.mme_est_valid > 0 and want.mme_gt_valid > 0 and want.n_w_voxels > 0
    for _ in range(3):  # (a schedule bug shows as a flaky difference)
        _same(want, eng.run_suite_from(est, gt, P, overlap=True))


@pytest.mark.parametrize("n_gt", [1_500, 2_048, 2_049])
def test_ground_truth_around_one_block(eng, dev, n_gt):
    """A ground truth of less than one gather block and one 2048-point block of k_level_hist_rows / k_cell_fill, of exactly one, and of
    one point more (a second block with a single point)."""
    est, gt = _cube(20_000, 5, dev, 0, scale=0.2), _cube(n_gt, 6, dev, 1, scale=0.2)
    P = _param()
    want = _single_lane(est, gt, P)
    assert want.mme_gt_valid > 0 and want.gt_est.n_corr == n_gt
    for _ in range(3):
        _same(want, eng.run_suite_from(est, gt, P, overlap=True))


def test_three_pairs_back_to_back_on_a_fresh_engine(eng, dev):
    """Sizes that change both ways: every table of the second pair is larger than the first's (fresh allocations, stale bytes), every
    table of the third smaller (the previous pair's entries lie behind its end).  Each against a fresh single-lane engine."""
    P = _param()
    for k, (n_est, n_gt) in enumerate([(60_000, 40_000), (250_000, 300_000), (30_000, 9_000)]):
        est, gt = _cube(n_est, 10 + k, dev, 0), _cube(n_gt, 20 + k, dev, 1)
        got = eng.run_suite_from(est, gt, P, overlap=True)
        _same(_single_lane(est, gt, P), got)


def _sheet(n, seed, dev):
    """A square sheet at 2500 pts/m^2 with +-10 um of relief, tilted against all three axes: every neighbourhood is thin."""
    import torch

    rng = np.random.default_rng(seed)
    side = np.sqrt(n / 2500.0)
    p = np.stack([rng.uniform(0, side, n), rng.uniform(0, side, n), rng.uniform(-1e-5, 1e-5, n)], 1)
    a = np.deg2rad(30.0)
    c, s = np.cos(a), np.sin(a)
    rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return torch.from_numpy(np.ascontiguousarray(p @ (rz @ rx).T + np.array([3.0, -2.0, 1.5]))).to(dev)


def test_thin_neighbourhoods_refined_between_the_two_mmes(eng, dev):
    """Two samples of one flat sheet: k_mme3 flags every query of both clouds, and the refine pass of the map's MME (and its second
    mailbox read) runs on the main stream before the ground truth's MME is queued."""
    est, gt = _sheet(100_000, 31, dev), _sheet(80_000, 32, dev)
    P = _param()
    want = _single_lane(est, gt, P)
    eng.timers_reset()
    got = eng.run_suite_from(est, gt, P, overlap=True)
    assert eng.timer("mme_refined")[1] > 0.9 * (len(est) + len(gt)), "the pair should exercise k_mme_refine in both MMEs"
    _same(want, got)
    _same(want, eng.run_suite_from(est, gt, P, overlap=True))


def test_a_failing_second_lane_returns_its_error_and_leaves_the_engine_usable(eng, dev):
    import torch

    from cloud_map_evaluation_amd.engine import MapEvalError

    est, gt = _cube(50_000, 41, dev, 0), _cube(50_000, 42, dev, 1)
    P = _param()
    want = eng.run_suite_from(est, gt, P, overlap=True)
    bad = gt.clone()
    bad[123, 1] = -float("inf")  # (found by the second lane's bounding box, before its sort)
    with pytest.raises(MapEvalError, match="NaN"):
        eng.run_suite_from(est, bad, P, overlap=True)
    with pytest.raises(MapEvalError):
        eng.run_suite_from(est, gt[:0], P, overlap=True)  # an empty ground truth (map_eval.cpp:32-35 returns -1)
    bad = est.clone()
    bad[5, 0] = float("inf")  # ... and a failing main lane while the second one is on its priority stream
    with pytest.raises(MapEvalError, match="NaN"):
        eng.run_suite_from(bad, gt, P, overlap=True)
    torch.cuda.synchronize()
    _same(want, eng.run_suite_from(est, gt, P, overlap=True))
    _same(want, eng.run_suite_from(est, gt, P, overlap=False))
