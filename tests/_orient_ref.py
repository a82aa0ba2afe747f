"""The numpy model of me_orient_normals: a restatement of the definition in include/mapeval_hip.h ("consistent normal
orientation"), item by item, in pure numpy and Python.  Sized for N <= ~20 k.

    orient(xyz, normals, k, direction=(0, 0, 1), inward=False) -> dict
        the me_orient_out integers, `component` int32[N], `flipped` bool[N], `normals` (the oriented copy) and, for the
        hand-worked tests, `tree` (the forest's edges as (lo, hi) in the edge order) and `roots` (root of every component).
"""
from __future__ import annotations

from collections import deque

import numpy as np


def knn_lists(xyz: np.ndarray, kk: int) -> np.ndarray:
    """idx int32[N][kk]: the kk nearest of every point in its own cloud by (d2, index), -1 past the end; d2 = (dx*dx + dy*dy) + dz*dz."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    out = np.full((n, kk), -1, np.int32)
    m = min(kk, n)
    step = max(1, min(n, (1 << 22) // max(n, 1)))
    for b in range(0, n, step):
        q = xyz[b:b + step]
        dx = q[:, None, 0] - xyz[None, :, 0]
        dy = q[:, None, 1] - xyz[None, :, 1]
        dz = q[:, None, 2] - xyz[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        if m < n:  # the m smallest and everything tied with the m-th, then the exact (d2, index) order among those
            kth = np.partition(d2, m - 1, axis=1)[:, m - 1]
            for r in range(len(q)):
                cand = np.flatnonzero(d2[r] <= kth[r])
                o = cand[np.argsort(d2[r, cand], kind="stable")][:m]  # cand ascends, the sort is stable: ties by index
                out[b + r, :m] = o
        else:
            out[b:b + len(q), :m] = np.argsort(d2, axis=1, kind="stable")
    return out


def dot3(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def graph_edges(xyz: np.ndarray, normals: np.ndarray, k: int):
    """(lo, hi, c) of the undirected graph, in the edge order of item 3; valid bool[N]."""
    normals = np.ascontiguousarray(normals, np.float64)
    valid = np.any(normals != 0, axis=1)
    lists = knn_lists(xyz, k + 1)
    n = len(xyz)
    i = np.repeat(np.arange(n, dtype=np.int64), k + 1)
    j = lists.reshape(-1).astype(np.int64)
    keep = (j >= 0) & (j != i)
    keep[keep] &= valid[i[keep]] & valid[j[keep]]
    i, j = i[keep], j[keep]
    pairs = np.unique(np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1), axis=0) if len(i) else np.zeros((0, 2), np.int64)
    lo, hi = pairs[:, 0], pairs[:, 1]
    c = dot3(normals[lo], normals[hi])
    # |c| descending through the bit pattern of |c| (for every non-NaN value the numerical order), then (lo, hi)
    key = np.abs(c).view(np.uint64)
    order = np.lexsort((hi, lo, ~key))
    return lo[order], hi[order], c[order], valid


def orient(xyz, normals, k: int, direction=(0.0, 0.0, 1.0), inward: bool = False) -> dict:
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    n = len(xyz)
    d = np.asarray(direction, np.float64)
    lo, hi, c, valid = graph_edges(xyz, normals, k)
    # Kruskal in the edge order
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    tree = []
    adj = [[] for _ in range(n)]
    for e in range(len(lo)):
        a, b = find(int(lo[e])), find(int(hi[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            tree.append((int(lo[e]), int(hi[e])))
            neg = bool(c[e] < 0)
            adj[lo[e]].append((int(hi[e]), neg))
            adj[hi[e]].append((int(lo[e]), neg))
    # components by ascending lowest member
    component = np.full(n, -1, np.int32)
    rep = np.array([find(i) for i in range(n)])  # (the union keeps the smaller index on top: rep = lowest member)
    reps = np.unique(rep[valid])
    component[valid] = np.searchsorted(reps, rep[valid]).astype(np.int32)
    ncomp = len(reps)
    proj = dot3(xyz, d[None, :])
    flipped = np.zeros(n, bool)
    roots = []
    members = [[] for _ in range(ncomp)]
    for i in np.flatnonzero(valid):
        members[component[i]].append(int(i))
    for m in members:
        pm = proj[m]
        root = m[int(np.flatnonzero(pm == pm.max())[0])]  # m ascends: the lowest index among the holders
        roots.append(root)
        flipped[root] = bool(dot3(normals[root], d) < 0) != bool(inward)
        seen = {root}
        dq = deque([root])
        while dq:
            u = dq.popleft()
            for v, neg in adj[u]:
                if v not in seen:
                    seen.add(v)
                    flipped[v] = flipped[u] ^ neg
                    dq.append(v)
    out_n = normals.copy()
    out_n[flipped] = -out_n[flipped]
    inconsistent = int(np.count_nonzero((c < 0) ^ flipped[lo] ^ flipped[hi])) if len(lo) else 0
    sizes = np.bincount(component[valid], minlength=max(ncomp, 1)) if ncomp else np.zeros(1, np.int64)
    return {
        "n": n, "n_valid": int(valid.sum()), "n_components": ncomp, "largest_component": int(sizes.max()) if ncomp else 0,
        "n_tree_edges": len(tree), "n_graph_edges": len(lo), "n_flipped": int(flipped.sum()), "n_inconsistent_edges": inconsistent,
        "component": component, "flipped": flipped, "normals": out_n, "tree": tree, "roots": roots,
    }


FIELDS = ("n", "n_valid", "n_components", "largest_component", "n_tree_edges", "n_graph_edges", "n_flipped", "n_inconsistent_edges")


def torus(n: int, seed: int, R: float = 1.0, r: float = 0.4):
    """n points on the torus (R, r) about the z axis, their exact outward unit normals, and the same normals each negated by a seeded coin."""
    g = np.random.default_rng(seed)
    u, v = g.uniform(0, 2 * np.pi, n), g.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=1)
    xyz = np.stack([R * np.cos(u), R * np.sin(u), np.zeros(n)], axis=1) + r * nrm
    coin = g.integers(0, 2, n).astype(bool)
    return xyz, nrm, np.where(coin[:, None], -nrm, nrm)


def torus_distance(p: np.ndarray, R: float = 1.0, r: float = 0.4) -> np.ndarray:
    """unsigned distance of points to the torus surface"""
    rho = np.hypot(p[:, 0], p[:, 1])
    return np.abs(np.hypot(rho - R, p[:, 2]) - r)


def shells(n_each: int, seed: int, radii=(1.0, 2.0)):
    g = np.random.default_rng(seed)
    pts, nrm = [], []
    for rad in radii:
        v = g.normal(size=(n_each, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        pts.append(rad * v)
        nrm.append(v)
    xyz, nrm = np.concatenate(pts), np.concatenate(nrm)
    coin = g.integers(0, 2, len(xyz)).astype(bool)
    return xyz, nrm, np.where(coin[:, None], -nrm, nrm)
