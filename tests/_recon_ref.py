"""The model of the surface reconstruction (include/mapeval_hip.h "surface reconstruction"), restated in
plain Python / numpy: the implicit-moving-least-squares field on the sparse voxel lattice and its zero set by marching tetrahedra.
Every number is an IEEE fp64 operation in the order the header states; the two sums of the field use math.fsum."""
from __future__ import annotations

import itertools
import math

import numpy as np

# the 7 edge directions out of a node, `dir` 0 .. 6
DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
DIR_INDEX = {d: i for i, d in enumerate(DIRS)}
# the 6 Kuhn tetrahedra around the diagonal (0,0,0)-(1,1,1): one per permutation of the axes, lexicographic
PERMS = sorted(itertools.permutations(range(3)))


def _unit(a):
    return tuple(1 if d == a else 0 for d in range(3))


def _add(u, v):
    return (u[0] + v[0], u[1] + v[1], u[2] + v[2])


def _sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def kuhn_tets():
    """The 4 corners (cell-local lattice offsets) of each of the 6 tetrahedra."""
    out = []
    for a, b, c in PERMS:
        v0 = (0, 0, 0)
        v1 = _add(v0, _unit(a))
        v2 = _add(v1, _unit(b))
        v3 = _add(v2, _unit(c))
        out.append((v0, v1, v2, v3))
    return out


TETS = kuhn_tets()


def det3(u, v, w):
    return (u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0]))


def tet_triangles(corners, inside):
    """Triangles of one tetrahedron as triples of edges; an edge is a pair of tetrahedron-local corner indices (lo, hi).  The winding
    ((B - A) x (C - A) from inside to outside) is decided by the sign of an integer determinant of the lattice vectors."""
    ins = [j for j in range(4) if inside[j]]
    outs = [j for j in range(4) if not inside[j]]
    E = lambda x, y: (min(x, y), max(x, y))
    if len(ins) in (0, 4):
        return []
    if len(ins) in (1, 3):
        p = ins[0] if len(ins) == 1 else outs[0]
        q = [j for j in range(4) if j != p]
        tri = [E(p, q[0]), E(p, q[1]), E(p, q[2])]
        d = det3(_sub(corners[q[0]], corners[p]), _sub(corners[q[1]], corners[p]), _sub(corners[q[2]], corners[p]))
        keep = d > 0 if len(ins) == 1 else d < 0
        return [tuple(tri)] if keep else [(tri[0], tri[2], tri[1])]
    p, q = ins
    r, s = outs
    quad = [E(p, r), E(p, s), E(q, s), E(q, r)]
    d = det3(_sub(corners[r], corners[p]), _sub(corners[s], corners[p]), _sub(corners[q], corners[p]))
    tris = [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    if not d > 0:
        tris = [(t[0], t[2], t[1]) for t in tris]
    return tris


def clamp01(t):
    if t < 0.0:
        return 0.0
    if t > 1.0:
        return 1.0
    return t


def isosurface(node_ijk, f, valid, voxel, cells=None):
    """Marching tetrahedra of a sparse lattice field.  node_ijk (n,3) ints, f (n,) float64, valid (n,) bool.  A cell (named by its
    corner 0) is extracted iff all 8 corners are present and valid, and, when `cells` (a set of (i, j, k)) is given, it is in the set.
    Returns dict(vertices (V,3) f8, vertex_edge (V,4) i4, triangles (T,3) i4, n_cells_extracted); cells in ascending (i, j, k) order."""
    node_ijk = np.asarray(node_ijk, np.int64).reshape(-1, 3)
    f = np.asarray(f, np.float64)
    valid = np.asarray(valid).astype(bool)
    h = float(voxel)
    index = {}
    for n, ijk in enumerate(map(tuple, node_ijk.tolist())):
        if ijk in index:
            raise ValueError("duplicate node")
        index[ijk] = n
    corners8 = [(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)]
    verts, vedge, tris, vid = [], [], [], {}
    n_cells = 0
    for o in sorted(index):
        if cells is not None and o not in cells:
            continue
        idx = [index.get(_add(o, c), -1) for c in corners8]
        if min(idx) < 0 or not all(valid[j] for j in idx):
            continue
        n_cells += 1
        for tet in TETS:
            nodes = [_add(o, c) for c in tet]
            fv = [float(f[index[nd]]) for nd in nodes]
            inside = [v < 0.0 for v in fv]
            for tri in tet_triangles(tet, inside):
                ids = []
                for lo, hi in tri:
                    a, b = nodes[lo], nodes[hi]
                    key = a + (DIR_INDEX[_sub(b, a)],)
                    if key not in vid:
                        fa, fb = fv[lo], fv[hi]
                        t = clamp01(fa / (fa - fb))
                        p = []
                        for d in range(3):
                            xa, xb = float(a[d]) * h, float(b[d]) * h
                            p.append(xa + t * (xb - xa))
                        vid[key] = len(verts)
                        verts.append(p)
                        vedge.append(key)
                    ids.append(vid[key])
                tris.append(ids)
    return {"vertices": np.array(verts, np.float64).reshape(-1, 3), "vertex_edge": np.array(vedge, np.int32).reshape(-1, 4),
            "triangles": np.array(tris, np.int32).reshape(-1, 3), "n_cells_extracted": n_cells}


def lattice(points, voxel, band):
    """(occupied cells, active cells, nodes) as sorted lists of (i, j, k)."""
    h = float(voxel)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    occ = set(map(tuple, np.floor(pts / h).astype(np.int64).tolist()))
    rng = range(-band, band + 1)
    act = {(c[0] + dx, c[1] + dy, c[2] + dz) for c in occ for dx in rng for dy in rng for dz in rng}
    nodes = {(c[0] + dx, c[1] + dy, c[2] + dz) for c in act for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
    return sorted(occ), sorted(act), sorted(nodes)


def field(points, normals, voxel, radius, min_k, band):
    """The IMLS field on the nodes of the active cells.  Returns dict(node_ijk (n,3) i4 ascending, f, k, valid, occupied, active)."""
    h, R = float(voxel), float(radius)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    nrm = np.asarray(normals, np.float64).reshape(-1, 3)
    occ, act, nodes = lattice(pts, h, band)
    ok = np.isfinite(nrm).all(axis=1) & ~(nrm == 0.0).all(axis=1)
    P, N = pts[ok], nrm[ok]
    R2 = R * R
    f = np.zeros(len(nodes))
    k = np.zeros(len(nodes), np.int32)
    valid = np.zeros(len(nodes), bool)
    for n, ijk in enumerate(nodes):
        x = np.array([float(ijk[0]) * h, float(ijk[1]) * h, float(ijk[2]) * h])
        box = (np.abs(P - x) < R).all(axis=1)  # (a prefilter only: |d| < R per axis is necessary for d2 < R*R)
        d = x - P[box]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        m = d2 < R2
        d, d2, nn = d[m], d2[m], N[box][m]
        q = 1.0 - d2 / R2
        w = (q * q) * (q * q)
        s = (nn[:, 0] * d[:, 0] + nn[:, 1] * d[:, 1]) + nn[:, 2] * d[:, 2]
        W = math.fsum(w.tolist())
        S = math.fsum((w * s).tolist())
        k[n] = int(m.sum())
        valid[n] = k[n] >= min_k and W > 0
        if valid[n]:
            f[n] = S / W
    return {"node_ijk": np.array(nodes, np.int32).reshape(-1, 3), "f": f, "k": k, "valid": valid, "occupied": occ, "active": act}


def field_bound(k, radius):
    """|f_device - f_model| on a valid node with unit normals: the device's two sums run in stream order, (k - 1) additions each,
    error <= (k - 1) u sum|terms| with |w s| <= w R; through the quotient that is 2 (k - 1) u R, one more u R for the device's division,
    3 u R for the model's two fsum roundings and its division; u = 2^-53.  (2k + 2) u R to first order; (2k + 4) u R covers the rest."""
    return (2.0 * np.asarray(k, np.float64) + 4.0) * 2.0 ** -53 * float(radius)


# ---- mesh predicates shared by the tests ----
def directed_edges(triangles):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def boundary_edges(triangles):
    """Directed edges (a, b) whose reverse (b, a) does not occur exactly once (or that occur more than once themselves)."""
    e = directed_edges(triangles)
    from collections import Counter

    cnt = Counter(map(tuple, e.tolist()))
    return [ab for ab, c in cnt.items() if c != 1 or cnt.get((ab[1], ab[0]), 0) != 1]


def euler_characteristic(n_vertices, triangles):
    e = directed_edges(triangles)
    und = {(min(a, b), max(a, b)) for a, b in e.tolist()}
    return n_vertices - len(und) + len(np.asarray(triangles).reshape(-1, 3))


def oriented_set(vertex_edge, triangles):
    """The triangles as a sorted list of oriented triples of (i, j, k, dir) keys, each rotated to start at its smallest key: what two
    implementations with different vertex and triangle orders must agree on."""
    ve = [tuple(r) for r in np.asarray(vertex_edge).reshape(-1, 4).tolist()]
    out = []
    for a, b, c in np.asarray(triangles).reshape(-1, 3).tolist():
        t = [ve[a], ve[b], ve[c]]
        m = t.index(min(t))
        out.append(tuple(t[m:] + t[:m]))
    return sorted(out)


def sphere_field(n=17, radius=5.3, centre=(8.1, 7.9, 8.2)):
    g = np.arange(n)
    ijk = np.array([(i, j, k) for i in g for j in g for k in g], np.int32)
    d = ijk - np.array(centre)
    return ijk, np.sqrt((d * d).sum(1)) - radius


def torus_field(n=17, major=4.6, minor=1.9, centre=(8.1, 7.9, 8.2)):
    g = np.arange(n)
    ijk = np.array([(i, j, k) for i in g for j in g for k in g], np.int32)
    d = ijk - np.array(centre)
    ring = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2) - major
    return ijk, np.sqrt(ring ** 2 + d[:, 2] ** 2) - minor
