"""Inputs for the DBSCAN kernels of me_cluster.hip at their edges: plain numpy, shared by tests/test_cluster_cpu.py (which proves, with
the model alone, that every cloud does what it is built for) and tests/test_gpu_cluster_edges.py (which holds the device to the model on
them).  Every builder returns (xyz, eps, ...) and, where stated, the closed-form expectation.  The coordinates of the exact cases are
dyadic: every d2 = ((dx*dx + dy*dy) + dz*dz) is exact in fp64, a tie with eps^2 is a tie for every implementation.

The index of a cloud (me_index.hip, cloud_build_index) has cells of edge cell_h = cell_size (1 + 2^-20) on the lattice of the multiples
of cell_h, whatever the cloud; DBSCAN at eps rebuilds it at cell_size = eps unless eps (1 + 2^-20) <= cell_h <= 1.5 eps (1 + 2^-20).
cell_index() restates that, the builders which rely on a point's cell assert it."""
from __future__ import annotations

import itertools
import math

import numpy as np

import _cluster_ref as R

SURVEY = (2.0 ** 19, -(2.0 ** 18), 64.0)  # dyadic: a dyadic cloud stays dyadic, |x| at survey magnitude
STRADDLE = (-3.0, -3.0, -3.0)  # cells on both sides of the origin in every axis


def cell_h_of(cell_size: float) -> float:
    return cell_size * (1.0 + 2.0 ** -20)


def cell_index(xyz: np.ndarray, cell_size: float) -> np.ndarray:
    """The cell of every point on the lattice cloud_build_index derives: origin = floor(lo / cell_h) cell_h per axis."""
    h = cell_h_of(cell_size)
    origin = np.floor(xyz.min(0) / h) * h
    return np.floor((xyz - origin) / h).astype(np.int64) + np.floor(xyz.min(0) / h).astype(np.int64)


# ---- the size sweep ----
def _stick(at, eps):
    """Six points 0.01 eps apart, then three more at steps of 0.9 eps: with min_points 4 the group and the first step are core (counts
    7 and 8), the second step has count 3 and a core neighbour (border), the third count 2 and none (noise)."""
    g = np.stack([np.arange(6) * 0.01 * eps, np.zeros(6), np.zeros(6)], 1)
    t = np.stack([0.05 * eps + np.arange(1, 4) * 0.9 * eps, np.zeros(3), np.zeros(3)], 1)
    return np.concatenate([g, t]) + np.asarray(at, np.float64)


def clumpy(n: int, seed: int = 0):
    """-> (xyz, eps = 0.1).  n >= 63: three tight blobs (each inside ONE cell of the grid at eps: centre (k + 0.5) cell_h, spread
    0.25 cell_h), a sparse sheet with about 1.5 neighbours per point, isolated points 10 eps apart and one _stick, shuffled: with
    min_points 4 core, border and noise points all occur, with min_points 2 core and noise (a point with a neighbour IS core then, a
    border point cannot exist).  n >= 1024: the first blob holds >= 600 points; one cell's points are contiguous in the sorted order,
    so at least one 256-aligned block lies wholly inside that cluster.  n < 63: n points in a box of 3 eps."""
    eps = 0.1
    rng = np.random.default_rng(1000 * seed + n)
    if n < 63:
        return rng.random((n, 3)) * 3.0 * eps, eps
    h = cell_h_of(eps)
    stick = _stick((5.0, 5.0, 5.0), eps)
    n_iso = max(4, n // 16)
    n_sheet = n // 4
    rest = n - len(stick) - n_iso - n_sheet
    big = max(600, rest // 2) if n >= 1024 else rest // 2
    small = (rest - big) // 2
    per = [big, small, rest - big - small]
    assert min(per) >= 4 and sum(per) == rest
    parts = [stick]
    for k, m in zip([(3, 3, 3), (13, 3, 3), (3, 13, 3)], per):
        parts.append((np.asarray(k) + 0.5) * h + (rng.random((m, 3)) - 0.5) * 0.5 * h)
    side = math.sqrt(n_sheet / 48.0)
    parts.append(np.concatenate([rng.random((n_sheet, 2)) * side, np.zeros((n_sheet, 1))], 1) + (0.0, 0.0, -2.0))
    g = np.arange(n_iso, dtype=np.float64)
    parts.append(np.stack([g % 16, g // 16, np.zeros(n_iso)], 1) * 10.0 * eps + (0.0, 0.0, -6.0))
    xyz = np.concatenate(parts)
    assert len(xyz) == n
    if n >= 1024:
        blob = parts[1]
        assert len(blob) >= 600 and (cell_index(blob, eps) == (3, 3, 3)).all()
        assert np.abs(blob - 3.5 * h).max() < 0.3 * h
    return xyz[rng.permutation(n)], eps


# ---- min_points at the count ----
def lattice_counts(k: int = 5, offset=(0.0, 0.0, 0.0)):
    """-> (xyz, eps, table).  k^3 lattice at spacing 1/4, eps 5/16: the neighbours are the six at 1/4 (the diagonal is 0.354), counts 7
    inside, 6 on a face, 5 on an edge, 4 at a corner.  table[min_points] = (n_core, n_border, n_noise, n_clusters), closed form."""
    g = np.arange(k, dtype=np.float64) * 0.25
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.asarray(offset, np.float64)
    i, f, e, c = (k - 2) ** 3, 6 * (k - 2) ** 2, 12 * (k - 2), 8
    assert k >= 3 and i + f + e + c == k ** 3
    table = {8: (0, 0, k ** 3, 0), 7: (i, f, e + c, 1), 6: (i + f, e, c, 1), 5: (i + f + e, c, 0, 1), 4: (k ** 3, 0, 0, 1)}
    return xyz, 0.3125, table


def check_lattice_counts(xyz, eps, k=5):
    """The counts of the lattice, from the exact pair list (re-run on a translated lattice)."""
    counts = R.dbscan(xyz, eps, 1, R.brute_pairs(xyz, eps))[1]
    assert np.bincount(counts, minlength=8).tolist() == [0, 0, 0, 0, 8, 12 * (k - 2), 6 * (k - 2) ** 2, (k - 2) ** 3]


# ---- the strict radius in all 26 directions ----
_SHAPES = {1: (15, 0, 0), 2: (9, 12, 0), 3: (2, 5, 14)}  # sixteenths: 225 = 15^2 = 9^2 + 12^2 = 2^2 + 5^2 + 14^2


def stencil_ties(offset=(0.0, 0.0, 0.0)):
    """-> (xyz, eps = 15/16, exact, inside).  For each of the 26 directions s in {-1, 0, 1}^3 \\ {0} two pairs (anchor, partner) with
    partner - anchor = s * o / 16, o a permutation-free assignment of the shape of that direction kind (face, edge, corner) to the
    non-zero axes: the pair `exact` lies at d2 == eps^2, the pair `inside` has ONE partner coordinate moved by one ulp towards the
    anchor (the axis where that changes d2 most), d2 < eps^2.  Every anchor lies within 1/16 of the faces of its cell that the
    direction crosses, so the partner is in the neighbouring cell in exactly that direction of the grid at eps; pairs are >= 4 eps
    apart.  exact, inside: (26, 2) point indices.  offset translates the skeleton BEFORE the one-ulp move, so the move is one ulp at
    the final magnitude.  min_points 2: 26 clusters of 2 (the inside pairs, in cloud order), 52 noise points."""
    eps = 0.9375
    h = cell_h_of(eps)
    offset = np.asarray(offset, np.float64)
    dirs = [s for s in itertools.product((-1, 0, 1), repeat=3) if any(s)]
    pts, exact, inside = [], [], []
    for d, s in enumerate(dirs):
        shape = iter(_SHAPES[sum(map(abs, s))])
        o = np.array([next(shape) if sa else 0 for sa in s], np.float64) / 16.0
        for which in range(2):
            site = offset + np.array([8 * (d % 6), 8 * (d // 6), 8 * which], np.float64) + 1.0  # pitch 8 > 4 eps + 2 eps
            a = np.empty(3)
            for ax in range(3):
                face = math.ceil(site[ax] / h) * h
                if s[ax] > 0:  # the last multiple of 1/16 below the face above
                    a[ax] = math.ceil(face * 16.0 - 1.0) / 16.0
                elif s[ax] < 0:  # the first multiple of 1/16 at or above the face below
                    a[ax] = math.ceil(face * 16.0) / 16.0
                else:  # well inside the cell
                    a[ax] = math.floor((face + 0.5 * h) * 16.0) / 16.0
            p = a + np.asarray(s) * o
            for ax in range(3):  # no point within rounding of a face it is meant to be beside
                lo = math.floor(a[ax] / h) * h
                assert min(a[ax] - lo, lo + h - a[ax]) > 1e-6 and min(abs(p[ax] - lo), abs(p[ax] - lo - h)) > 1e-6
            if which == 1:
                gain = [o[ax] * abs(np.nextafter(p[ax], a[ax]) - p[ax]) for ax in range(3)]
                ax = int(np.argmax(gain))
                p[ax] = np.nextafter(p[ax], a[ax])
            (exact, inside)[which].append((len(pts), len(pts) + 1))
            pts += [a, p]
    xyz, exact, inside = np.array(pts), np.array(exact), np.array(inside)
    check_stencil_ties(xyz, eps, exact, inside)
    cells = cell_index(xyz, eps)
    for pr in (exact, inside):
        assert np.array_equal(cells[pr[:, 1]] - cells[pr[:, 0]], np.array(dirs)), "a partner is not in the neighbouring cell"
    return xyz, eps, exact, inside


def check_stencil_ties(xyz, eps, exact, inside):
    assert (R.d2_exact(xyz[exact[:, 0]], xyz[exact[:, 1]]) == eps * eps).all()
    assert (R.d2_exact(xyz[inside[:, 0]], xyz[inside[:, 1]]) < eps * eps).all()
    pr = R.brute_pairs(xyz, eps)
    assert np.array_equal(pr, inside), "the inside pairs, and nothing else, are neighbours"
    d2 = R.d2_exact(xyz[:, None, :], xyz[None, :, :])
    far = np.ones_like(d2, bool)
    for a, b in np.concatenate([exact, inside]):
        far[a, b] = far[b, a] = far[a, a] = far[b, b] = False
    assert d2[far].min() >= (4.0 * eps) ** 2


# ---- union-find topologies ----
def shapes(kind: str, seed: int = 0):
    """-> (xyz, eps = 0.1, n_clusters): a few thousand points, spacing 0.6 eps along every chain (each chain point has its two chain
    neighbours within eps and the next but one at 1.2 eps), shuffled.  n_clusters: closed form at min_points 2; for "dense" a dict
    by min_points.  seed only changes the order of the points."""
    eps = 0.1
    s = 0.6 * eps
    rng = np.random.default_rng(seed)
    if kind == "star":  # 64 chains of 60 points meeting in a hub blob: 64 sets arrive at one root
        k = np.arange(64) + 0.5
        phi, ct = k * math.pi * (3.0 - math.sqrt(5.0)), 1.0 - 2.0 * k / 64.0
        st = np.sqrt(1.0 - ct * ct)
        u = np.stack([st * np.cos(phi), st * np.sin(phi), ct], 1)
        chains = (u[:, None, :] * (np.arange(1, 61) * s)[None, :, None]).reshape(-1, 3)
        hub = np.concatenate([np.zeros((1, 3)), (np.random.default_rng(64).random((31, 3)) - 0.5) * 0.4 * eps])
        xyz, m = np.concatenate([hub, chains]), 1
    elif kind in ("u", "u_open"):  # two trees of 2000 that meet at their far end only, or not at all
        x = np.arange(2000) * s
        a = np.stack([x, np.zeros(2000), np.zeros(2000)], 1)
        b = a + (0.0, 1.5 * eps, 0.0)
        bridge = np.array([[0.0, 0.6 * eps, 0.0], [0.0, 0.9 * eps, 0.0]])
        xyz, m = (np.concatenate([a, b, bridge]), 1) if kind == "u" else (np.concatenate([a, b]), 2)
    elif kind == "ring":  # a closed loop: the last edge joins the two ends of one set
        n = 3000
        r = s / (2.0 * math.sin(math.pi / n))
        t = 2.0 * math.pi * np.arange(n) / n
        xyz, m = np.stack([r * np.cos(t), r * np.sin(t), np.zeros(n)], 1), 1
    elif kind == "comb":  # a spine with 100 teeth of 20 points, 3 eps apart
        spine = np.stack([np.arange(500) * s, np.zeros(500), np.zeros(500)], 1)
        tx, ty = np.meshgrid(np.arange(100) * 5 * s, np.arange(1, 21) * s, indexing="ij")
        teeth = np.stack([tx.ravel(), ty.ravel(), np.zeros(2000)], 1)
        xyz, m = np.concatenate([spine, teeth]), 1
    elif kind == "dense":  # every pair an edge, far more points in one cell than a tile holds
        xyz = np.concatenate([np.tile([[0.375, 0.625, 0.125]], (4097, 1)), [[0.375 + 10.0 * eps, 0.625, 0.125]]])
        m = {1: 2, 2: 1, 4097: 1, 4098: 0}  # (min_points 1: the far point is a cluster of its own)
    else:
        raise ValueError(kind)
    return xyz[rng.permutation(len(xyz))], eps, m


# ---- border rules ----
BORDER_MIN_POINTS = 5


def border_rules():
    """-> (xyz, eps = 1, parts).  Three chains of six points 3/16 apart (counts 6 .. 7: core from min_points 5 down) pointing away
    from one shared point P, the nearest point of each 15/16 from P and the next 18/16: P has count 4, one core neighbour in each of
    three clusters.  A pair 1/2 apart and 16 from everything (count 2 >= 2: a border CANDIDATE with no core neighbour) and one isolated
    point.  parts: name -> indices (blob0, blob1, blob2, shared, pair, lone).
    A point next to three clusters has count >= 4, so it is non-core only from min_points 5 up: BORDER_MIN_POINTS = 5 is the
    smallest setting at which the shared BORDER point exists.  At min_points 3 the same cloud is one cluster through a core P."""
    r = np.arange(6) * 0.1875 + 0.9375
    z = np.zeros(6)
    blobs = [np.stack([r, z, z], 1), np.stack([-r, z, z], 1), np.stack([z, r, z], 1)]
    xyz = np.concatenate(blobs + [[[0.0, 0.0, 0.0]], [[16.0, 0.0, 0.0], [16.5, 0.0, 0.0]], [[0.0, 16.0, 0.0]]]) + 2.0
    parts = {"blob0": np.arange(0, 6), "blob1": np.arange(6, 12), "blob2": np.arange(12, 18), "shared": np.array([18]),
             "pair": np.array([19, 20]), "lone": np.array([21])}
    return xyz, 1.0, parts


def border_permutations():
    """Six cloud orders of border_rules(): the three blobs in each of their 3! orders (first blob 0, 1, 2, 0, 1, 2), the rest behind."""
    _, _, parts = border_rules()
    tail = np.concatenate([parts["pair"], parts["shared"], parts["lone"]])
    return [np.concatenate([parts[f"blob{k}"] for k in order] + [tail]) for order in [(0, 1, 2), (1, 0, 2), (2, 0, 1), (0, 2, 1), (1, 2, 0), (2, 1, 0)]]


def blobs_and_singletons():
    """-> (xyz, eps = 0.1): five tight blobs of 3 .. 40 points and 20 singletons 10 eps apart.  min_points 3: every blob point is core,
    every singleton has count 1: clusters and NO border candidate."""
    eps = 0.1
    rng = np.random.default_rng(8)
    parts = [np.array([4.0 * k, 0.0, 0.0]) * eps + rng.random((m, 3)) * 0.3 * eps for k, m in enumerate([3, 40, 7, 3, 12])]
    g = np.arange(20, dtype=np.float64)
    parts.append(np.stack([g % 5, 2.0 + g // 5, np.ones(20)], 1) * 10.0 * eps)
    xyz = np.concatenate(parts)
    return xyz[rng.permutation(len(xyz))], eps


def halo(k: int = 8, s: int = 600):
    """-> (xyz, eps = 0.125, min_points = k + s): k coincident points and s points on a sphere of radius 0.9 eps around them.  The centre
    has count k + s (core), a sphere point misses at least its antipode (1.8 eps away): count < k + s, a border point of the one
    cluster.  The s border candidates are the whole compacted list of k_cluster_border and all take label 0: whole blocks of 256
    with one key."""
    eps = 0.125
    j = np.arange(s) + 0.5
    phi, ct = j * math.pi * (3.0 - math.sqrt(5.0)), 1.0 - 2.0 * j / s
    st = np.sqrt(1.0 - ct * ct)
    shell = np.stack([st * np.cos(phi), st * np.sin(phi), ct], 1) * 0.9 * eps
    xyz = np.concatenate([np.zeros((k, 3)), shell]) + (1.0, 2.0, 3.0)
    return xyz[np.random.default_rng(k + s).permutation(k + s)], eps, k + s


def many_pairs(m: int = 257):
    """-> (xyz, eps = 0.25): m pairs 0.5 eps apart on a lattice of pitch 4.5 eps, pair k = points 2k, 2k + 1.  min_points 2: m clusters
    of size 2, cluster k = pair k; min_points 3: every point a border candidate, no cluster."""
    eps = 0.25
    k = np.arange(m)
    base = np.stack([k % 8, (k // 8) % 8, k // 64], 1) * 4.5 * eps
    return np.stack([base, base + (0.5 * eps, 0.0, 0.0)], 1).reshape(-1, 3), eps


def tied_sizes(k: int = 4):
    """-> (xyz, eps = 0.25, sizes): tight rows of 5, 9, 9, 3, 9 points and k single points, 8 eps apart, in that cloud order.
    min_points 1: every point is core, cluster id = position in that list, sizes as returned."""
    eps = 0.25
    sizes = [5, 9, 9, 3, 9] + [1] * k
    xyz = np.concatenate([np.stack([8.0 * eps * c + np.arange(m) * 0.0625 * eps, np.zeros(m), np.full(m, 0.5)], 1)
                          for c, m in enumerate(sizes)])
    return xyz, eps, np.array(sizes, np.int64)
