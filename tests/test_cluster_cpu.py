"""DBSCAN contract without a GPU: the numpy / scipy model of tests/_cluster_ref.py against the literal Open3D loop (three pop orders) and
sklearn's brute DBSCAN, its edges (strict radius, min_points extremes, relabelling under a permutation), and the host's config keys."""
import json
import os
import subprocess

import numpy as np
import pytest

import _cluster_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloud_map_evaluation_amd", "host", "map_eval")


def _bridge(offset):
    """Two rows of points 0.05 apart along x and one point between their ends, 0.3 from each: at eps 0.31 and min_points 5 every row
    point is core (7 .. 13 neighbours), the point between has 3 neighbours — a border point adjacent to two clusters."""
    a = np.stack([-np.arange(21) * 0.05, np.zeros(21), np.zeros(21)], 1)
    b = np.stack([0.6 + np.arange(21) * 0.05, np.zeros(21), np.zeros(21)], 1)
    return np.concatenate([a, [[0.3, 0.0, 0.0]], b]) + np.asarray(offset, np.float64)


def _two_cluster_border_points(xyz, eps, min_points, labels, counts):
    nbs = R.brute_neighbours(xyz, eps)
    core = counts >= min_points
    return [i for i in range(len(xyz)) if not core[i] and len({int(labels[j]) for j in nbs[i] if core[j]}) >= 2]


def _cloud(seed):
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([R.blobs(rng, 5, 90, 0.12, 2.0, 100), _bridge((10.0, 10.0, 10.0))])
    return xyz[rng.permutation(len(xyz))]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("eps,min_points", [(0.31, 5), (0.21, 8), (0.12, 4), (0.31, 14)])
def test_model_equals_open3d_loop_and_sklearn(seed, eps, min_points):
    from sklearn.cluster import DBSCAN

    xyz = _cloud(seed)
    assert len(xyz) <= 600
    labels, counts, m = R.dbscan(xyz, eps, min_points)
    for pop_seed in (0, 1, 2):
        l2, c2, m2 = R.brute_open3d(xyz, eps, min_points, seed=pop_seed)
        assert np.array_equal(counts, c2) and m == m2
        assert np.array_equal(labels, l2), (pop_seed, np.nonzero(labels != l2)[0][:10])
    sk = DBSCAN(eps=eps, min_samples=min_points, algorithm="brute").fit(xyz)
    # (sklearn's ball is closed and its distances come from the dot-product form: on these clouds no pair lies within rounding of eps)
    d2 = R.d2_exact(xyz[:, None, :], xyz[None, :, :])
    assert np.abs(np.sqrt(d2) - eps).min() > 1e-9
    assert np.array_equal(labels, sk.labels_.astype(np.int32))
    assert labels.max() + 1 == m and set(np.unique(labels[labels >= 0])) == set(range(m))
    if (eps, min_points) == (0.31, 5):
        two = _two_cluster_border_points(xyz, eps, min_points, labels, counts)
        assert len(two) >= 1  # the case takes the path it names
        nbs = R.brute_neighbours(xyz, eps)
        for i in two:
            assert labels[i] == min(int(labels[j]) for j in nbs[i] if counts[j] >= min_points)


def test_min_points_extremes():
    xyz = _cloud(4)
    labels, counts, m = R.dbscan(xyz, 0.21, 1)
    assert (labels >= 0).all() and (counts >= 1).all()  # every point is core: no noise, no border
    l2, _, m2 = R.brute_open3d(xyz, 0.21, 1)
    assert np.array_equal(labels, l2) and m == m2
    labels, counts, m = R.dbscan(xyz, 0.21, int(counts.max()) + 1)
    assert m == 0 and (labels == -1).all()
    assert np.array_equal(R.brute_open3d(xyz, 0.21, int(counts.max()) + 1)[0], labels)


def _lattice(spacing, k=5):
    g = np.arange(k, dtype=np.float64) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def test_strict_radius_on_a_lattice():
    eps = 0.25
    xyz = _lattice(eps)  # spacing exactly eps: d2 == eps^2 does not connect
    labels, counts, m = R.dbscan(xyz, eps, 2)
    assert (counts == 1).all() and m == 0 and (labels == -1).all()
    labels, counts, m = R.dbscan(xyz, eps, 1)
    assert m == len(xyz) and np.array_equal(labels, np.arange(len(xyz)))  # singletons, numbered in cloud order
    xyz = _lattice(eps * (1.0 - 2.0 ** -30))
    labels, counts, m = R.dbscan(xyz, eps, 2)
    assert m == 1 and (labels == 0).all() and counts.min() == 4 and counts.max() == 7
    assert np.array_equal(R.brute_open3d(xyz, eps, 2)[0], labels)


def test_relabelling_under_a_permutation():
    xyz = _cloud(5)
    eps, mp = 0.31, 5
    labels, counts, m = R.dbscan(xyz, eps, mp)
    perm = np.random.default_rng(9).permutation(len(xyz))
    lp, cp, mq = R.dbscan(xyz[perm], eps, mp)
    assert mq == m and np.array_equal(cp, counts[perm])
    back = np.empty_like(lp)
    back[perm] = lp  # labels of the permuted run, in the first run's order
    assert np.array_equal(back == -1, labels == -1)
    # the same partition of the core points (a border point between two clusters follows the NEW numbering: left out)
    core = counts >= mp
    pairs = set(zip(labels[core].tolist(), back[core].tolist()))
    assert len(pairs) == m and len({a for a, _ in pairs}) == m and len({b for _, b in pairs}) == m
    # ids follow the new smallest core index
    core_p = cp >= mp
    first = [int(np.nonzero(core_p & (lp == c))[0][0]) for c in range(mq)]
    assert first == sorted(first)


def test_cluster_keep_model():
    labels = np.array([0, 0, 0, 1, 1, -1, 2, 2, 2, 3], np.int32)
    assert R.cluster_sizes(labels, 4).tolist() == [3, 2, 3, 1]
    assert R.cluster_keep(labels, 4, 2).tolist() == [True] * 5 + [False] + [True] * 3 + [False]
    assert R.cluster_keep(labels, 4, 1, keep_largest=1).tolist() == [True] * 3 + [False] * 7  # tie 0 / 2: the smaller id
    assert R.cluster_keep(labels, 4, 3, keep_largest=3).tolist() == [True] * 3 + [False] * 3 + [True] * 3 + [False]


# ---- host: the config keys of remove_outliers: cluster ----
CONFIG = """registration_methods: 2
icp_max_distance: 1.0
accuracy_level: [0.2, 0.1, 0.08, 0.05, 0.01]
initial_matrix:
  - [1.0, 0.0, 0.0, 0.0]
  - [0.0, 1.0, 0.0, 0.0]
  - [0.0, 0.0, 1.0, 0.0]
  - [0.0, 0.0, 0.0, 1.0]
estimate_map_path: /a
gt_map_path: /b.pcd
scene_name: unit_test
save_immediate_result: true
evaluate_mme: true
evaluate_gt_mme: false
nn_radius: 0.1
evaluate_using_initial: true
vmd_voxel_size: 3.0
downsample_size: 0.0
enable_debug: false
"""


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.dirname(EXE), "-s"])
    return EXE


def _parse(exe, tmp_path, extra):
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG + extra)
    return subprocess.run([exe, "--parse-config", str(cfg)], capture_output=True, text=True, timeout=120)


def test_host_accepts_cluster_with_defaults_and_explicit_values(exe, tmp_path):
    r = _parse(exe, tmp_path, "remove_outliers: cluster\noutlier_eps: 0.1\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["remove_outliers"] == "cluster" and p["outlier_eps"] == 0.1
    assert (p["outlier_min_points"], p["outlier_min_cluster_size"], p["outlier_keep_largest"]) == (10, 1, 0)
    r = _parse(exe, tmp_path, "remove_outliers: cluster\noutlier_eps: 0.25\noutlier_min_points: 4\noutlier_min_cluster_size: 5000\n"
                              "outlier_keep_largest: 2\noutlier_filter_gt: true\n")
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert (p["outlier_eps"], p["outlier_min_points"], p["outlier_min_cluster_size"], p["outlier_keep_largest"]) == (0.25, 4, 5000, 2)
    assert p["outlier_filter_gt"] is True


@pytest.mark.parametrize("extra,word", [
    ("remove_outliers: cluster\n", "outlier_eps"),
    ("remove_outliers: cluster\noutlier_eps: 0.0\n", "outlier_eps"),
    ("remove_outliers: cluster\noutlier_eps: -0.1\n", "outlier_eps"),
    ("remove_outliers: cluster\noutlier_eps: 0.1\noutlier_min_points: 0\n", "outlier_min_points"),
    ("remove_outliers: cluster\noutlier_eps: 0.1\nnum_gpus: 2\n", "single GPU"),
    ("remove_outliers: cluster\noutlier_eps: 0.1\nevaluate_noised_gt: true\n", "evaluate_noised_gt"),
])
def test_host_refuses(exe, tmp_path, extra, word):
    r = _parse(exe, tmp_path, extra)
    assert r.returncode != 0 and word in r.stderr, (r.stdout, r.stderr)
