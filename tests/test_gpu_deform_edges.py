"""me_voxel_deformation at its edges: partial rows and block edges, rows of many runs (the overflow regions and their retry), one
voxel over many rows, points on voxel faces, floor(x / vs) where x * (1 / vs) rounds the other way, the strict distance gate, the
min_pairs threshold, voxels without pairs, degenerate sources, and a 1-NN result without neighbour indices.  Every case goes through
the common checks of tests/_deform_checks.py."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _deform_checks as dc  # noqa: E402
import _deform_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
EST, GT = dc.EST, dc.GT
EYE = np.eye(3)


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _moved(est, seed, shift=(0.003, -0.002, 0.001), noise=0.002):
    return est + shift + noise * np.random.default_rng(seed).standard_normal(est.shape)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 400_000])
def test_cloud_sizes(eng, n):
    rng = np.random.default_rng(n)
    box = 6.0 if n > 10_000 else 2.0  # (216 voxels of ~1850 points; 8 voxels)
    est = rng.uniform(0.0, box, (n, 3))
    got, m, idx, d2 = dc.run(eng, est, _moved(est, n + 1), 1.0, 0.05, min_pairs=3, cell_size=0.1)
    assert got["n_pairs"].sum() > 0


def test_a_row_cut_into_many_voxels_and_the_overflow_retry(eng):
    """64 points = one row of 64 sorted points; 8 voxels: >= 4 runs, the overflow region of the row; every point its own voxel: 62
    further runs, more than a region holds at this size (17): the pass runs again with larger regions and must give the same rows."""
    rng = np.random.default_rng(1)
    est = rng.uniform(0.0, 1.0, (64, 3))
    got, *_ = dc.run(eng, est, _moved(est, 2), 0.5, 0.05, min_pairs=3)
    assert got["n_voxels"] == 8
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    est = 0.25 * g + rng.uniform(0.05, 0.2, (64, 3))
    got, *_ = dc.run(eng, est, _moved(est, 3), 0.25, 0.05, min_pairs=3)
    assert got["n_voxels"] == 64 and (got["n_pairs"] == 1).all() and (got["flags"] == 0).all()


def test_one_voxel_over_many_rows(eng):
    rng = np.random.default_rng(4)
    est = rng.uniform(0.5, 9.5, (4097, 3))
    got, *_ = dc.run(eng, est, _moved(est, 5), 10.0, 0.5)
    assert got["n_voxels"] == 1 and got["n_pairs"][0] == 4097 and got["flags"][0] == ref.FIT | ref.ROT_OK


@pytest.mark.parametrize("vs", [0.1, 0.25])
def test_points_on_voxel_faces(eng, vs):
    """Coordinates exactly on faces (k vs as the double the product gives), negative ones included, and for 0.1 the textbook point 0.3
    (0.3 / 0.1 = 2.9999999999999996 but 0.3 * 10 = 3.0000000000000004): the case of tests/test_gpu_voxel_records.py."""
    rng = np.random.default_rng(6)
    k = rng.integers(-4, 5, (600, 3)).astype(np.float64)
    est = k * vs
    est[200:] += rng.uniform(0.0, vs, (400, 3)) * (rng.random((400, 3)) < 0.5)  # some coordinates on a face, some inside
    est = np.concatenate([est, [[0.3, 0.35, -0.3]]])
    assert np.floor(0.3 / 0.1) == 2.0 and np.floor(0.3 * (1.0 / 0.1)) == 3.0
    got, *_ = dc.run(eng, est, _moved(est, 7), vs, 0.05, min_pairs=3)
    if vs == 0.1:
        assert (got["keys"] == [2, 3, -3]).all(1).any()


def test_the_distance_gate_is_strict(eng):
    """d2 == max_distance^2 exactly is no pair; d2 one ulp below is."""
    dy = 1.5 * 2.0 ** -29
    est = np.array([[0.0, 0.0, 0.0], [0.0, 8.0, 0.0]])
    gt = np.array([[0.25, 0.0, 0.0], [0.25 - 2.0 ** -55, 8.0 + dy, 0.0]])
    got, m, idx, d2 = dc.run(eng, est, gt, 1.0, 0.25, min_pairs=3)
    assert d2[0] == 0.0625 and d2[1] == np.nextafter(0.0625, 0.0) and idx.tolist() == [0, 1]
    assert got["n_pairs"].tolist() == [0, 1]
    got = eng.deformation_field(EST, 1.0, np.nextafter(0.25, 1.0), min_pairs=3)
    assert got["n_pairs"].tolist() == [1, 1]
    got = eng.deformation_field(EST, 1.0, math.inf, min_pairs=3)
    assert got["n_pairs"].tolist() == [1, 1]


def test_min_pairs_threshold(eng):
    rng = np.random.default_rng(8)
    est = np.concatenate([rng.uniform(0.1, 0.9, (29, 3)), rng.uniform(0.1, 0.9, (30, 3)) + [3.0, 0.0, 0.0]])
    got, *_ = dc.run(eng, est, _moved(est, 9), 1.0, 0.05)
    assert got["n_pairs"].tolist() == [29, 30] and got["flags"].tolist() == [0, ref.FIT | ref.ROT_OK]
    assert got["n_fit"] == 1 and got["max_row"] == 1
    assert np.array_equal(got["R"][0], EYE) and np.array_equal(got["u"][0], got["t0"][0]) and got["e_R"][0] == got["e_t"][0]


def test_voxels_without_pairs(eng):
    rng = np.random.default_rng(10)
    est = rng.uniform(0.0, 3.0, (3000, 3))
    got, *_ = dc.run(eng, est, _moved(est, 11) + 100.0, 1.0, 1.0)  # the reference cloud far away: no pair at all
    assert got["n_voxels"] == 27 and got["n_with_pairs"] == 0 and got["n_pairs"].sum() == 0 and got["max_row"] == -1 and got["max_key"] is None
    assert not got["sums"].any() and not got["t0"].any() and not got["u"].any() and (got["R"] == EYE).all()
    assert not got["e0"].any() and not got["e_t"].any() and not got["e_R"].any()
    assert math.isnan(got["share_translation"]) and math.isnan(got["share_rigid"]) and math.isnan(got["mean_disp"])
    gt = _moved(est, 11)
    gt = gt[est[:, 0] < 0.9]  # a reference under the first slab of voxels only (and 9 cm inside it: no pair across the face)
    got, *_ = dc.run(eng, est, gt, 1.0, 0.02)
    assert got["n_voxels"] == 27 and 0 < got["n_with_pairs"] <= 9 and (got["n_pairs"][9:] == 0).all()


def test_collinear_and_coincident_sources(eng):
    line = 0.5 + np.outer(np.linspace(-0.4, 0.4, 40), [1.0, 0.5, 0.25])
    dot = np.full((40, 3), 0.25) + [2.0, 0.0, 0.0]
    est = np.concatenate([line, dot])
    gt = np.concatenate([line + [0.001, 0.002, -0.001], dot[:1] + [0.0, 0.001, 0.0]])
    got, *_ = dc.run(eng, est, gt, 1.0, 0.05)
    assert got["n_pairs"].tolist() == [40, 40] and got["flags"].tolist() == [ref.FIT, ref.FIT] and got["n_rot"] == 0
    assert (got["R"] == EYE).all() and np.array_equal(got["u"], got["t0"]) and np.array_equal(got["e_R"], got["e_t"])


def test_a_result_without_neighbour_indices(eng):
    """me_set_nn_result carries distances only (the indices are -1): none of its pairs is used, whatever the sign of d2."""
    rng = np.random.default_rng(12)
    est = rng.uniform(0.0, 2.0, (1000, 3))
    gt = _moved(est, 13)
    dc.run(eng, est, gt, 1.0, 0.05)
    _, d2 = eng.nn_fetch(EST)
    d2 = np.where(rng.random(1000) < 0.3, -1.0, d2)
    eng.set_nn_result(EST, GT, d2)
    idx, back = eng.nn_fetch(EST)
    assert (idx == -1).all() and np.array_equal(back, d2)
    got = eng.deformation_field(EST, 1.0, 0.05)
    dc.check(eng, est, gt, idx, d2, got, 1.0, 0.05, 30, None, searched=False)
    assert got["n_voxels"] == 8 and got["n_pairs"].sum() == 0 and not got["sums"].any()
