"""DBSCAN contract without a GPU: the numpy / scipy model of tests/_cluster_ref.py against the literal Open3D loop (three pop orders) and
sklearn's brute DBSCAN, its edges (strict radius, min_points extremes, relabelling under a permutation), the exact pair list and the
closed forms of the clouds of tests/_cluster_edge_cases.py (what tests/test_gpu_cluster_edges.py relies on), and the host's config keys."""
import json
import os
import subprocess

import numpy as np
import pytest

import _cluster_edge_cases as E
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


# ---- the exact pair list and the clouds of tests/_cluster_edge_cases.py: what test_gpu_cluster_edges.py relies on ----
def _classes(labels, counts, mp):
    core = counts >= mp
    return int(core.sum()), int(((labels >= 0) & ~core).sum()), int((labels < 0).sum())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_brute_pairs_equals_the_tree_and_the_open3d_loop(seed):
    rng = np.random.default_rng(seed)
    xyz = R.blobs(rng, 5, 90, 0.12, 2.0, 100)
    for eps in (0.12, 0.31):
        bp, tp = R.brute_pairs(xyz, eps, rows=97), R.pairs(xyz, eps)
        assert bp.dtype == tp.dtype == np.int64 and bp.shape == tp.shape and (bp[:, 0] < bp[:, 1]).all()
        assert np.array_equal(bp[np.lexsort((bp[:, 1], bp[:, 0]))], tp[np.lexsort((tp[:, 1], tp[:, 0]))])
        for mp in (1, 2, 5):
            l1, c1, m1 = R.dbscan(xyz, eps, mp, pr=bp)
            l2, c2, m2 = R.brute_open3d(xyz, eps, mp)
            assert np.array_equal(l1, l2) and np.array_equal(c1, c2) and m1 == m2
    assert R.brute_pairs(xyz[:1], 0.3).shape == (0, 2) and R.brute_pairs(xyz[:0], 0.3).shape == (0, 2)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 4097])
def test_clumpy_has_every_class(n):
    xyz, eps = E.clumpy(n)
    assert xyz.shape == (n, 3) and len(np.unique(xyz, axis=0)) == n
    pr = R.brute_pairs(xyz, eps)
    labels, counts, m = R.dbscan(xyz, eps, 1, pr)
    assert _classes(labels, counts, 1) == (n, 0, 0)  # min_points 1: every point is core
    labels, counts, m = R.dbscan(xyz, eps, n + 1, pr)
    assert m == 0 and _classes(labels, counts, n + 1) == (0, 0, n)
    if n >= 63:
        n_core, n_border, n_noise = _classes(*R.dbscan(xyz, eps, 4, pr)[:2], 4)
        assert n_core > 0 and n_border > 0 and n_noise > 0
        n_core, n_border, n_noise = _classes(*R.dbscan(xyz, eps, 2, pr)[:2], 2)
        assert n_core > 0 and n_border == 0 and n_noise > 0  # (count >= 2 IS core at min_points 2: no border point can exist)
    if n >= 1024:  # a 256-aligned block of the sorted order inside one cell, whatever the curve: >= 600 points of one cell
        cells = E.cell_index(xyz, eps)
        _, per_cell = np.unique(cells, axis=0, return_counts=True)
        assert per_cell.max() >= 600 >= 2 * 256 - 1


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), E.SURVEY, E.STRADDLE], ids=["origin", "survey", "straddle"])
def test_lattice_and_stencil_closed_forms(offset):
    xyz, eps, table = E.lattice_counts(5, offset)
    assert table == {8: (0, 0, 125, 0), 7: (27, 54, 44, 1), 6: (81, 36, 8, 1), 5: (117, 8, 0, 1), 4: (125, 0, 0, 1)}
    E.check_lattice_counts(xyz, eps)
    pr = R.brute_pairs(xyz, eps)
    for mp, want in table.items():
        labels, counts, m = R.dbscan(xyz, eps, mp, pr)
        assert _classes(labels, counts, mp) + (m,) == want
    xyz, eps, exact, inside = E.stencil_ties(offset)  # (asserts the ties, the one-ulp pairs, the cells and the 4 eps itself)
    assert eps == 0.9375 and len(xyz) == 104 and len(exact) == len(inside) == 26
    if any(offset):
        assert (xyz.min(0) < 0).any() and (np.abs(xyz).max(0) > 1).all()
    labels, counts, m = R.dbscan(xyz, eps, 2, R.brute_pairs(xyz, eps))
    assert m == 26 and np.array_equal(labels[inside], np.stack([np.arange(26)] * 2, 1))
    assert (labels[exact] == -1).all() and (counts[exact] == 1).all() and _classes(labels, counts, 2) == (52, 0, 52)
    if offset == E.STRADDLE:
        assert (E.cell_index(xyz, eps).min(0) < 0).all() and (E.cell_index(xyz, eps).max(0) > 0).all()


@pytest.mark.parametrize("kind", ["star", "u", "u_open", "ring", "comb", "dense"])
def test_shapes_closed_forms(kind):
    xyz, eps, want = E.shapes(kind)
    pr = R.brute_pairs(xyz, eps)
    if kind == "dense":
        assert len(xyz) == 4098
        for mp, m_want in want.items():
            labels, counts, m = R.dbscan(xyz, eps, mp, pr)
            assert m == m_want and sorted(np.unique(counts).tolist()) == [1, 4097]
        return
    labels, counts, m = R.dbscan(xyz, eps, 2, pr)
    assert m == want and (labels >= 0).all() and 2000 <= len(xyz) <= 4100
    if kind == "ring":
        assert (counts == 3).all()
    if kind == "u_open":
        assert R.cluster_sizes(labels, m).tolist() == [2000, 2000]
    for seed in (1, 2):  # the further permutations of the GPU test are other orders of the same points
        other = E.shapes(kind, seed)[0]
        assert not np.array_equal(other, xyz) and np.array_equal(np.unique(other, axis=0), np.unique(xyz, axis=0))


def test_border_rules_closed_forms():
    xyz, eps, parts = E.border_rules()
    mp = E.BORDER_MIN_POINTS
    pr = R.brute_pairs(xyz, eps)
    labels, counts, m = R.dbscan(xyz, eps, mp, pr)
    assert m == 3 and counts[parts["shared"]].tolist() == [4] and counts[parts["pair"]].tolist() == [2, 2] and counts[parts["lone"]].tolist() == [1]
    assert [labels[parts[f"blob{k}"]].tolist() for k in range(3)] == [[0] * 6, [1] * 6, [2] * 6] and (counts[:18] >= mp).all()
    assert labels[parts["shared"]].tolist() == [0] and (labels[parts["pair"]] == -1).all() and labels[parts["lone"]].tolist() == [-1]
    assert _classes(labels, counts, mp) == (18, 1, 3)
    # the shared point's core neighbours: one in each cluster
    nb = R.brute_neighbours(xyz, eps)[int(parts["shared"][0])]
    assert sorted(labels[j] for j in nb if counts[j] >= mp) == [0, 1, 2]
    # six orders: the winner is the blob that comes first; every blob wins twice, no two neighbouring orders agree
    winners = []
    for perm in E.border_permutations():
        assert sorted(perm.tolist()) == list(range(len(xyz)))
        lp, cp, mq = R.dbscan(xyz[perm], eps, mp, R.brute_pairs(xyz[perm], eps))
        back = np.empty_like(lp)
        back[perm] = lp
        assert mq == 3 and back[parts["shared"][0]] == 0 and (back[parts["pair"]] == -1).all()
        winners.append([k for k in range(3) if back[parts[f"blob{k}"][0]] == 0][0])
    assert winners == [0, 1, 2, 0, 1, 2]
    # min_points 3, the same cloud: P is core (4 >= 3) and the three chains are ONE cluster through it
    labels, counts, m = R.dbscan(xyz, eps, 3, pr)
    assert m == 1 and _classes(labels, counts, 3) == (19, 0, 3)


def test_skipped_launch_clouds_and_keep_clouds():
    xyz, eps = E.blobs_and_singletons()
    labels, counts, m = R.dbscan(xyz, eps, 3, R.brute_pairs(xyz, eps))
    assert m == 5 and not ((counts < 3) & (counts >= 2)).any() and _classes(labels, counts, 3) == (65, 0, 20)  # clusters, no candidate
    xyz, eps, mp = E.halo()
    labels, counts, m = R.dbscan(xyz, eps, mp, R.brute_pairs(xyz, eps))
    assert m == 1 and (labels == 0).all() and _classes(labels, counts, mp) == (8, 600, 0) and 600 >= 2 * 256 - 1  # one cluster of border points
    xyz, eps = E.many_pairs(257)
    pr = R.brute_pairs(xyz, eps)
    assert np.array_equal(pr, np.arange(514).reshape(257, 2))
    d2 = R.d2_exact(xyz[:, None, :], xyz[None, :, :])
    assert np.sort(d2, axis=1)[:, 2].min() >= (4.0 * eps) ** 2  # everything but the partner is >= 4 eps away
    labels, counts, m = R.dbscan(xyz, eps, 3, pr)
    assert m == 0 and (counts == 2).all() and (labels == -1).all()  # candidates, no cluster
    labels, counts, m = R.dbscan(xyz, eps, 2, pr)
    assert m == 257 and np.array_equal(labels, np.repeat(np.arange(257), 2))
    assert np.array_equal(np.flatnonzero(R.cluster_keep(labels, m, 1, 100)), np.arange(200))
    xyz, eps, sizes = E.tied_sizes()
    labels, counts, m = R.dbscan(xyz, eps, 1, R.brute_pairs(xyz, eps))
    assert m == 9 and sizes.tolist() == [5, 9, 9, 3, 9, 1, 1, 1, 1] and np.array_equal(R.cluster_sizes(labels, m), sizes)
    assert np.array_equal(labels, np.repeat(np.arange(9), sizes))
    assert np.unique(labels[R.cluster_keep(labels, m, 1, 2)]).tolist() == [1, 2]  # the tie in size cut by keep_largest: the smaller ids
    assert np.unique(labels[R.cluster_keep(labels, m, 1, 3)]).tolist() == [1, 2, 4]
    assert not R.cluster_keep(labels, m, 10, 0).any()


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
