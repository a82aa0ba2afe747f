"""numpy / scipy model of me_cluster_dbscan and me_cluster_keep (me_cluster.hip, include/mapeval_hip.h "clustering"), after Open3D 0.15's
PointCloud::ClusterDBSCAN.

The six rules of the header: neighbours by d2 = ((dx*dx + dy*dy) + dz*dz) < eps*eps in fp64 (strict, the point itself counted); core iff
count >= min_points; clusters = connected components of the core points under the neighbour relation, numbered by their smallest core
index; a border point takes the smallest cluster id among its core neighbours; everything else is -1.  Candidate pairs come from scipy's
cKDTree at eps (1 + 1e-9), their d2 is recomputed exactly, so the tree's own rounding never decides anything.  brute_open3d is the
literal loop of the library (O(n^2) neighbour lists, a frontier popped in a seeded random order) the tests hold the model to."""
from __future__ import annotations

import numpy as np


def d2_exact(q: np.ndarray, p: np.ndarray) -> np.ndarray:
    d = q - p
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def pairs(xyz: np.ndarray, eps: float) -> np.ndarray:
    """All i < j with d2 < eps^2, (m, 2) int64 (the costly part of the model: pass it to dbscan() when several min_points share an eps)."""
    from scipy.spatial import cKDTree

    tree = cKDTree(xyz)
    pr = tree.query_pairs(eps * (1.0 + 1e-9), output_type="ndarray")
    if len(pr) == 0:
        return np.zeros((0, 2), np.int64)
    ok = np.empty(len(pr), bool)
    step = 1 << 22
    for b in range(0, len(pr), step):
        s = pr[b:b + step]
        ok[b:b + step] = d2_exact(xyz[s[:, 0]], xyz[s[:, 1]]) < eps * eps
    return pr[ok].astype(np.int64)


def brute_pairs(xyz: np.ndarray, eps: float, rows: int = 256) -> np.ndarray:
    """All i < j with d2_exact < eps^2, (m, 2) int64 as pairs() returns them, from the O(n^2) definition in chunks of rows: no tree and
    no prefilter, so nothing but d2_exact decides at any coordinate magnitude.  Sorted by (i, j)."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    r2 = eps * eps
    out = []
    for b in range(0, n, rows):
        near = d2_exact(xyz[b:b + rows, None, :], xyz[None, :, :]) < r2
        i, j = np.nonzero(near)
        i += b
        m = i < j
        out.append(np.stack([i[m], j[m]], 1))
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 2), np.int64)


def dbscan(xyz: np.ndarray, eps: float, min_points: int, pr: np.ndarray | None = None):
    """-> labels (int32, cloud order), counts (int32, the point itself included), n_clusters.  pr: pairs(xyz, eps), when at hand."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    pr = pairs(xyz, eps) if pr is None else pr
    counts = (1 + np.bincount(pr[:, 0], minlength=n) + np.bincount(pr[:, 1], minlength=n)).astype(np.int32)
    core = counts >= min_points
    labels = np.full(n, -1, np.int32)
    if not core.any():
        return labels, counts, 0
    cc = pr[core[pr[:, 0]] & core[pr[:, 1]]]
    graph = coo_matrix((np.ones(len(cc), np.int8), (cc[:, 0], cc[:, 1])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    core_idx = np.nonzero(core)[0]
    # numbering: ascending smallest core index of the component
    first = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(first, comp[core_idx], core_idx)
    used = np.nonzero(first < n)[0]
    order = used[np.argsort(first[used], kind="stable")]
    cid = np.full(comp.max() + 1, -1, np.int64)
    cid[order] = np.arange(len(order))
    labels[core_idx] = cid[comp[core_idx]]
    # border: smallest id among the core neighbours' clusters
    best = np.full(n, np.iinfo(np.int64).max, np.int64)
    for a, b in ((0, 1), (1, 0)):
        m = ~core[pr[:, a]] & core[pr[:, b]]
        np.minimum.at(best, pr[m, a], labels[pr[m, b]].astype(np.int64))
    border = ~core & (best != np.iinfo(np.int64).max)
    labels[border] = best[border]
    return labels, counts, len(order)


def cluster_sizes(labels: np.ndarray, n_clusters: int) -> np.ndarray:
    return np.bincount(labels[labels >= 0], minlength=n_clusters).astype(np.int64)


def cluster_keep(labels: np.ndarray, n_clusters: int, min_cluster_size: int = 1, keep_largest: int = 0) -> np.ndarray:
    """keep[i] = label >= 0 && size >= min_cluster_size && (keep_largest == 0 || rank < keep_largest); rank: descending size, ties by
    ascending id."""
    size = cluster_sizes(labels, n_clusters)
    ok = size >= min_cluster_size
    if keep_largest > 0:
        order = np.lexsort((np.arange(n_clusters), -size))
        rank = np.empty(n_clusters, np.int64)
        rank[order] = np.arange(n_clusters)
        ok &= rank < keep_largest
    keep = np.zeros(len(labels), bool)
    m = labels >= 0
    keep[m] = ok[labels[m]]
    return keep


def brute_neighbours(xyz: np.ndarray, eps: float):
    xyz = np.ascontiguousarray(xyz, np.float64)
    d2 = d2_exact(xyz[:, None, :], xyz[None, :, :])
    return [np.nonzero(row < eps * eps)[0] for row in d2]


def brute_open3d(xyz: np.ndarray, eps: float, min_points: int, seed: int = 0):
    """The loop of PointCloud::ClusterDBSCAN, restated: points in index order; an unvisited core point opens the next cluster, whose
    frontier (a set, popped in an arbitrary order — here a seeded random one) labels every point it reaches that has no cluster yet
    and expands through core points only.  -> labels, counts, n_clusters."""
    rng = np.random.default_rng(seed)
    nbs = brute_neighbours(xyz, eps)
    n = len(nbs)
    counts = np.array([len(v) for v in nbs], np.int32)
    labels = np.full(n, -2, np.int64)  # -2 undefined, -1 noise
    cluster = 0
    for i in range(n):
        if labels[i] != -2:
            continue
        if len(nbs[i]) < min_points:
            labels[i] = -1
            continue
        labels[i] = cluster
        frontier = set(int(j) for j in nbs[i]) - {i}
        visited = set(frontier) | {i}
        while frontier:
            items = sorted(frontier)
            j = items[int(rng.integers(len(items)))]
            frontier.discard(j)
            if labels[j] == -1:
                labels[j] = cluster  # noise so far: a border point of this cluster
            if labels[j] != -2:
                continue
            labels[j] = cluster
            if len(nbs[j]) >= min_points:
                for q in nbs[j]:
                    q = int(q)
                    if q not in visited:
                        visited.add(q)
                        frontier.add(q)
        cluster += 1
    labels[labels == -2] = -1
    return labels.astype(np.int32), counts, cluster


def blobs(rng, n_blobs: int, per: int, sigma: float, spread: float, n_noise: int) -> np.ndarray:
    """Gaussian blobs in a box plus uniform noise, shuffled."""
    c = rng.uniform(0.0, spread, (n_blobs, 3))
    pts = [c[k] + rng.normal(0.0, sigma, (per, 3)) for k in range(n_blobs)]
    pts.append(rng.uniform(-0.2 * spread, 1.2 * spread, (n_noise, 3)))
    xyz = np.concatenate(pts)
    return xyz[rng.permutation(len(xyz))]
