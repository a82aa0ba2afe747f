"""numpy model of me_mesh_topology and me_mesh_signed_distance (include/mapeval_hip.h), operation by operation, the
generalized winding number as an independent oracle, and the small meshes the tests share.  The closest point is tests/_mesh_ref.py's."""
from __future__ import annotations

import math

import numpy as np

import _mesh_ref as R

BOUNDARY, NONMANIFOLD, INCONSISTENT, ZERO, TAINTED = 1, 2, 4, 8, 16
ON, UNSIGNED, UNRELIABLE = 1, 2, 4
EDGE_BAD = BOUNDARY | NONMANIFOLD | INCONSISTENT


def faces(vertices, triangles):
    """(n[T,3], nhat[T,3] (0 where degenerate), ang[T,3], degenerate[T]) from the corners."""
    v = np.asarray(vertices, np.float64)[np.asarray(triangles)]
    A, B, C = v[:, 0], v[:, 1], v[:, 2]
    n = R.cross(B - A, C - A)
    deg = (n == 0.0).all(axis=1)
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    with np.errstate(all="ignore"):
        nhat = np.where(deg[:, None], 0.0, n / ln[:, None])
    ang = np.stack([np.arctan2(ln, R._dot(B - A, C - A)), np.arctan2(ln, R._dot(C - B, A - B)), np.arctan2(ln, R._dot(A - C, B - C))], -1)
    ang = np.where(deg[:, None], 0.0, ang)
    return n, nhat, ang, deg


def topology(vertices, triangles, vertex_weight="angle"):
    """The model of me_mesh_topology.  vertex_weight="equal" is the mutation (weights 1 in place of the angles)."""
    tri = np.asarray(triangles, np.int64)
    nv, nt = len(vertices), len(tri)
    n, nhat, ang, deg = faces(vertices, tri)
    edges = {}  # (lo, hi) -> list of (t, e, dir) in ascending (t, e)
    eid = -np.ones((nt, 3), np.int64)
    for t in range(nt):
        i = tri[t]
        if i[0] == i[1] or i[1] == i[2] or i[2] == i[0]:
            continue
        for e in range(3):
            a, b = int(i[e]), int(i[(e + 1) % 3])
            edges.setdefault((min(a, b), max(a, b)), []).append((t, e, a < b))
    keys = sorted(edges)
    e_n = np.zeros((len(keys), 3))
    e_fl = np.zeros(len(keys), np.uint8)
    for k, key in enumerate(keys):
        inc = edges[key]
        s = np.zeros(3)
        nf = 0
        for t, e, _ in inc:
            eid[t, e] = k
            if not deg[t]:
                nf += 1
                s = s + nhat[t]
        m = len(inc)
        f = 0
        if m == 1:
            f |= BOUNDARY
        if m > 2:
            f |= NONMANIFOLD
        if m == 2 and inc[0][2] == inc[1][2]:
            f |= INCONSISTENT
        if nf == 0 or (s == 0.0).all():
            f |= ZERO
        e_n[k], e_fl[k] = s, f
    v_n = np.zeros((nv, 3))
    v_fl = np.full(nv, ZERO, np.uint8)
    v_sum_ang = np.zeros(nv)
    valence = np.zeros(nv, np.int64)
    referenced = np.zeros(nv, bool)
    acc = {}
    for t in range(nt):
        for c in range(3):
            acc.setdefault(int(tri[t, c]), []).append((t, c))
    for v, inc in acc.items():
        s = np.zeros(3)
        nf = 0
        bad = 0
        for t, c in inc:
            if not deg[t]:
                nf += 1
                w = ang[t, c] if vertex_weight == "angle" else 1.0
                s = s + w * nhat[t]
                v_sum_ang[v] += ang[t, c]
            for e in (eid[t, c], eid[t, (c + 2) % 3]):
                if e >= 0:
                    bad |= int(e_fl[e])
        f = 0
        if nf == 0 or (s == 0.0).all():
            f |= ZERO
        if bad & EDGE_BAD:
            f |= TAINTED
        v_n[v], v_fl[v], valence[v], referenced[v] = s, f, len(inc), True
    cnt = {
        "n_edges": len(keys), "n_boundary_edges": int(((e_fl & BOUNDARY) != 0).sum()),
        "n_nonmanifold_edges": int(((e_fl & NONMANIFOLD) != 0).sum()), "n_inconsistent_edges": int(((e_fl & INCONSISTENT) != 0).sum()),
        "n_zero_edges": int(((e_fl & ZERO) != 0).sum()), "n_zero_vertices": int(((v_fl & ZERO) != 0).sum()),
        "n_tainted_vertices": int(((v_fl & TAINTED) != 0).sum()), "n_unreferenced_vertices": int((~referenced).sum()),
    }
    cnt["closed"] = cnt["n_boundary_edges"] == 0
    cnt["oriented_manifold"] = not (e_fl & EDGE_BAD).any()
    # per (triangle, local edge), as me_mesh_topology_fetch lays them out
    te_n = np.where((eid >= 0)[..., None], e_n[np.maximum(eid, 0)] if len(keys) else 0.0, 0.0)
    te_fl = np.where(eid >= 0, e_fl[np.maximum(eid, 0)] if len(keys) else 0, ZERO).astype(np.uint8)
    return {"counts": cnt, "n": n, "deg": deg, "eid": eid, "edge_normal": te_n, "edge_flags": te_fl, "vertex_normal": v_n,
            "vertex_flags": v_fl, "vertex_sum_ang": v_sum_ang, "valence": valence}


def signed(points, vertices, triangles, dist=None, topo=None, edge_rule="pseudo"):
    """The model of me_mesh_signed_distance per point, from a mesh-distance result (the model's own when None): dict of signed_d, flags,
    g and N.  edge_rule="face" is the mutation (the winning triangle's own normal on edges)."""
    pts = np.asarray(points, np.float64)
    tri = np.asarray(triangles, np.int64)
    dist = R.distance(pts, vertices, tri) if dist is None else dist
    topo = topology(vertices, tri) if topo is None else topo
    t, r = dist["tri"].astype(np.int64), dist["region"].astype(np.int64)
    N = topo["n"][t].copy()
    tf = np.zeros(len(pts), np.uint8)
    e = (r >= 1) & (r <= 3)
    if edge_rule == "pseudo":
        N[e] = topo["edge_normal"][t[e], r[e] - 1]
    tf[e] = topo["edge_flags"][t[e], r[e] - 1]
    v = r >= 4
    vi = tri[t[v], r[v] - 4]
    N[v] = topo["vertex_normal"][vi]
    tf[v] = topo["vertex_flags"][vi]
    d = pts - dist["closest"]
    g = (d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]
    d2 = dist["d2"]
    root = np.sqrt(d2)
    on = d2 == 0.0
    structural = topo["deg"][t] | ((tf & ZERO) != 0)  # unsigned whatever g is
    unsg = ~on & (structural | ~((g > 0) | (g < 0)))
    sd = np.where(on, 0.0, np.where(unsg, np.nan, np.where(g > 0, root, -root)))
    fl = (on * ON + unsg * UNSIGNED + ((tf & (EDGE_BAD | TAINTED)) != 0) * UNRELIABLE).astype(np.uint8)
    return {"signed_d": sd, "flags": fl, "g": g, "N": N, "d2": d2, "region": r, "structural": structural}


def totals(d2, region, sd, fl, max_distance=math.inf):
    """me_mesh_sign_out from per-point values; the sums with math.fsum."""
    m = d2 <= max_distance * max_distance
    s = m & ((fl & UNSIGNED) == 0)
    idx = np.flatnonzero(s)
    out = {"n_query": len(d2), "n_matched": int(m.sum()), "n_signed": int(s.sum()), "n_inside": int((s & (sd < 0)).sum()),
           "n_outside": int((s & (sd > 0)).sum()), "n_on": int((s & ((fl & ON) != 0)).sum()), "n_unsigned": int((m & ~s).sum()),
           "n_unreliable": int((m & ((fl & UNRELIABLE) != 0)).sum()),
           "n_by_region": [int((m & (region == 0)).sum()), int((m & (region >= 1) & (region <= 3)).sum()), int((m & (region >= 4)).sum())],
           "sum_signed": math.fsum(sd[s]), "sum_abs_signed": math.fsum(np.abs(sd[s])), "sum_signed2": math.fsum(sd[s] * sd[s]),
           "min_signed": 0.0, "argmin": -1, "max_signed": 0.0, "argmax": -1}
    if len(idx):
        out["argmin"], out["argmax"] = int(idx[np.argmin(sd[idx])]), int(idx[np.argmax(sd[idx])])  # (first occurrence: the smaller index)
        out["min_signed"], out["max_signed"] = float(sd[out["argmin"]]), float(sd[out["argmax"]])
    return out


def winding(points, vertices, triangles):
    """Generalized winding number: the solid angles of all triangles (van Oosterom and Strackee) summed, over 4 pi.  1 inside a closed
    mesh whose normals point outward, 0 outside.  Brute force; shares nothing with the pseudo-normal path."""
    p = np.asarray(points, np.float64)[:, None, :]
    v = np.asarray(vertices, np.float64)[np.asarray(triangles)][None]
    a, b, c = v[:, :, 0] - p, v[:, :, 1] - p, v[:, :, 2] - p
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    num = np.einsum("...i,...i", a, np.cross(b, c))
    den = la * lb * lc + np.einsum("...i,...i", a, b) * lc + np.einsum("...i,...i", b, c) * la + np.einsum("...i,...i", c, a) * lb
    return (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * math.pi)


# ---- the meshes ----
def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64) + np.array([0.1, 0.2, 0.3])
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


def prism(poly, z0=0.0, z1=1.0):
    """Closed prism over a counter-clockwise polygon, caps by a fan from the ear-free triangulation given with the polygon."""
    pts, cap = poly
    n = len(pts)
    v = np.array([[x, y, z0] for x, y in pts] + [[x, y, z1] for x, y in pts], np.float64)
    t = []
    for a, b, c in cap:
        t.append([a, c, b])              # bottom, outward = -z
        t.append([n + a, n + b, n + c])  # top
    for i in range(n):
        j = (i + 1) % n
        t += [[i, j, n + j], [i, n + j, n + i]]
    return v, np.array(t, np.int32)


def cube(offset=(0.0, 0.0, 0.0)):
    v, t = prism(([(0, 0), (1, 0), (1, 1), (0, 1)], [(0, 1, 2), (0, 2, 3)]))
    return v + np.asarray(offset, np.float64), t


def l_prism():
    """L-shaped prism: the re-entrant edge is the vertical one at (1, 1)."""
    pts = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]
    return prism((pts, [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]))


def torus(nu=20, nw=10, R0=1.0, r0=0.35):
    u = np.arange(nu) * (2 * math.pi / nu)
    w = np.arange(nw) * (2 * math.pi / nw)
    U, W = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R0 + r0 * np.cos(W)) * np.cos(U), (R0 + r0 * np.cos(W)) * np.sin(U), r0 * np.sin(W)], -1).reshape(-1, 3)
    t = []
    for i in range(nu):
        for j in range(nw):
            a, b = i * nw + j, ((i + 1) % nu) * nw + j
            c, d = ((i + 1) % nu) * nw + (j + 1) % nw, i * nw + (j + 1) % nw
            t += [[a, b, c], [a, c, d]]
    return v, np.array(t, np.int32)


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    t = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, t


def subdivide(v, t):
    """Every triangle into 4 by its edge midpoints (shared per edge): a closed surface stays closed."""
    v = [tuple(x) for x in np.asarray(v, np.float64)]
    mid = {}

    def m(a, b):
        k = (min(a, b), max(a, b))
        if k not in mid:
            mid[k] = len(v)
            v.append(tuple((np.array(v[a]) + np.array(v[b])) / 2.0))
        return mid[k]
    out = []
    for a, b, c in np.asarray(t):
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
    return np.array(v, np.float64), np.array(out, np.int32)


def surface_prefix(n_triangles):
    """The first n_triangles triangles of the octahedron subdivided until it has that many: closed iff n_triangles is 8 * 4^k (a closed
    manifold has an even count), otherwise open along the cut, with unreferenced vertices."""
    v, t = octahedron()
    while len(t) < n_triangles:
        v, t = subdivide(v, t)
    return v, np.ascontiguousarray(t[:n_triangles])


def with_degenerate(v, t):
    """Split the edge AB of triangle 0 at its midpoint M on ONE side only (triangle 0 becomes A M C and M B C) and fill the T-junction with
    the degenerate triangle (A, B, M) traversed against the neighbour across AB: closed, +2 triangles, one of them degenerate."""
    v, t = np.asarray(v, np.float64), [list(x) for x in np.asarray(t)]
    a, b, c = t[0]
    m = len(v)
    v = np.vstack([v, (v[a] + v[b]) / 2.0])
    t[0] = [a, m, c]
    t += [[m, b, c], [a, b, m]]
    return v, np.array(t, np.int32)


def fan(k=70):
    """k triangles round the apex (vertex 0) of a shallow open cone: one vertex run of k corner records."""
    a = np.arange(k) * (2 * math.pi / k)
    v = np.vstack([[0.0, 0.0, 0.3], np.stack([np.cos(a), np.sin(a), np.zeros(k)], -1)])
    return v, np.array([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], np.int32)


def sliver_fan():
    """A closed, convex double pyramid with sharp apexes (vertices 0 and 1) that see wide faces on one side and 11 slivers on the other:
    equal weights pull the vertex normal towards the slivers, whose normals make more than 90 degrees with the wide faces'; the angles
    do not."""
    a = np.array([0.0, 2.0] + list(math.pi + 0.9 + np.arange(12) * 0.01))  # wide gaps, then slivers
    ring = np.stack([np.cos(a), np.sin(a), np.zeros(len(a))], -1)
    v = np.vstack([[0.0, 0.0, 3.0], [0.0, 0.0, -3.0], ring])
    n = len(a)
    t = []
    for i in range(n):
        j = (i + 1) % n
        t += [[0, 2 + i, 2 + j], [1, 2 + j, 2 + i]]
    return v, np.array(t, np.int32)


def fin():
    """5 faces on the edge (0, 1)."""
    a = np.arange(5) * (2 * math.pi / 5)
    v = np.vstack([[0, 0, 0], [0, 0, 1], np.stack([np.cos(a), np.sin(a), 0.5 * np.ones(5)], -1)]).astype(np.float64)
    return v, np.array([[0, 1, 2 + i] for i in range(5)], np.int32)


def inconsistent_pair():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.2]], np.float64)
    return v, np.array([[0, 1, 2], [1, 2, 3]], np.int32)  # both traverse 1 -> 2


def queries(vertices, triangles, n, seed, inflate=0.5):
    """n continuous random draws in the bounding box of the referenced vertices inflated by `inflate` of its diagonal."""
    v = np.asarray(vertices, np.float64)[np.unique(triangles)]
    lo, hi = v.min(0), v.max(0)
    pad = inflate * float(np.linalg.norm(hi - lo))
    return np.random.default_rng(seed).uniform(lo - pad, hi + pad, size=(n, 3))


# ---- the record lists of the topology build: k_topo_face's keys, the stable sorts, the serial walks of k_topo_edges / k_topo_verts ----
def key_bits(nv):
    """topo_build's `bits`: the smallest value with nv < 2^bits"""
    bits = 1
    while (1 << bits) <= nv:
        bits += 1
    return bits


def edge_records(triangles, nv):
    """(sorted keys, sorted values 3 t + e, no_edge, bits): the edge records of k_topo_face (key = lo << bits | hi, no_edge for a
    triangle that names a vertex twice) after the stable sort over the low 2 * bits bits."""
    tri = np.asarray(triangles, np.int64)
    bits = key_bits(nv)
    no_edge = (nv << bits) | nv
    a, b = tri, np.roll(tri, -1, axis=1)
    twice = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0])
    key = np.where(twice[:, None], no_edge, (np.minimum(a, b) << bits) | np.maximum(a, b)).reshape(-1)
    order = np.argsort(key & ((1 << (2 * bits)) - 1), kind="stable")
    return key[order], order, no_edge, bits


def corner_records(triangles, nv):
    """(sorted keys, sorted values 3 t + c): the corner records (key = vertex) after the stable sort over the low `bits` bits."""
    key = np.asarray(triangles, np.int64).reshape(-1)
    order = np.argsort(key & ((1 << key_bits(nv)) - 1), kind="stable")
    return key[order], order


def record_topology(vertices, triangles):
    """me_mesh_topology the way the device builds it: from the sorted records, the head of every run walking its run.  The same dict
    as topology() plus edge_runs / vertex_runs: (position of the head in the sorted list, run length, key) per run."""
    tri = np.asarray(triangles, np.int64)
    nv, nt = len(vertices), len(tri)
    n3 = 3 * nt
    n, nhat, ang, deg = faces(vertices, tri)
    key, val, no_edge, _ = edge_records(tri, nv)
    head = np.array([key[i] != no_edge and (i == 0 or key[i - 1] != key[i]) for i in range(n3)])
    rank = np.cumsum(head) - head  # (the exclusive scan: the edge id)
    n_edges = int(head.sum())
    e_n, e_fl = np.zeros((max(n_edges, 1), 3)), np.zeros(max(n_edges, 1), np.uint8)
    eid = -np.ones((nt, 3), np.int64)
    edge_runs = []
    for i in np.flatnonzero(head):
        s, m, nf, dir0, same, j = np.zeros(3), 0, 0, False, False, int(i)
        while j < n3 and key[j] == key[i]:
            t, e = divmod(int(val[j]), 3)
            d = bool(tri[t, e] < tri[t, (e + 1) % 3])
            if m == 0:
                dir0 = d
            elif m == 1:
                same = d == dir0
            m += 1
            if not deg[t]:
                nf += 1
                s = s + nhat[t]
            eid[t, e] = rank[i]
            j += 1
        f = (BOUNDARY if m == 1 else 0) | (NONMANIFOLD if m > 2 else 0) | (INCONSISTENT if m == 2 and same else 0)
        if nf == 0 or (s == 0.0).all():
            f |= ZERO
        e_n[rank[i]], e_fl[rank[i]] = s, f
        edge_runs.append((int(i), m, int(key[i])))
    vkey, vval = corner_records(tri, nv)
    v_n, v_fl = np.zeros((nv, 3)), np.full(nv, ZERO, np.uint8)
    referenced = np.zeros(nv, bool)
    vertex_runs = []
    for i in range(n3):
        if i and vkey[i - 1] == vkey[i]:
            continue
        s, nf, bad, j = np.zeros(3), 0, 0, i
        while j < n3 and vkey[j] == vkey[i]:
            t, c = divmod(int(vval[j]), 3)
            if not deg[t]:
                nf += 1
                s = s + ang[t, c] * nhat[t]
            for e in (eid[t, c], eid[t, (c + 2) % 3]):
                if e >= 0:
                    bad |= int(e_fl[e])
            j += 1
        f = (ZERO if nf == 0 or (s == 0.0).all() else 0) | (TAINTED if bad & EDGE_BAD else 0)
        v_n[vkey[i]], v_fl[vkey[i]], referenced[vkey[i]] = s, f, True
        vertex_runs.append((i, j - i, int(vkey[i])))
    fl = e_fl[:n_edges]
    cnt = {
        "n_edges": n_edges, "n_boundary_edges": int(((fl & BOUNDARY) != 0).sum()), "n_nonmanifold_edges": int(((fl & NONMANIFOLD) != 0).sum()),
        "n_inconsistent_edges": int(((fl & INCONSISTENT) != 0).sum()), "n_zero_edges": int(((fl & ZERO) != 0).sum()),
        "n_zero_vertices": int(((v_fl & ZERO) != 0).sum()), "n_tainted_vertices": int(((v_fl & TAINTED) != 0).sum()),
        "n_unreferenced_vertices": int((~referenced).sum()),
    }
    cnt["closed"] = cnt["n_boundary_edges"] == 0
    cnt["oriented_manifold"] = not (fl & EDGE_BAD).any()
    te_n = np.where((eid >= 0)[..., None], e_n[np.maximum(eid, 0)], 0.0)
    te_fl = np.where(eid >= 0, e_fl[np.maximum(eid, 0)], ZERO).astype(np.uint8)
    return {"counts": cnt, "n": n, "deg": deg, "eid": eid, "edge_normal": te_n, "edge_flags": te_fl, "vertex_normal": v_n, "vertex_flags": v_fl,
            "edge_runs": edge_runs, "vertex_runs": vertex_runs}
