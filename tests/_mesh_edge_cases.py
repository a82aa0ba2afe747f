"""The inputs of tests/test_mesh_edges_cpu.py, tests/test_gpu_mesh_edges.py and tests/test_gpu_mesh_sign_edges.py: meshes and queries
built to reach, exactly, the places of csrc/me_mesh.hip and csrc/me_meshsign.hip that random heightfields and random queries do not.
Pure numpy.  Every coordinate is dyadic (a small integer over a power of two, case H's heights included), so differences, dot and
cross products and therefore d2 and g = dot(p - c, N) are exact in fp64 and the tests compare bits.  Each generator returns a dict with
the vertices "v", the triangles "t", the queries "q" and the facts the tests assert."""
from __future__ import annotations

import functools
import math

import numpy as np

import _mesh_ref as R
import _mesh_sign_ref as S

ROUND = 256 * 1024  # the lanes of one round of k_mesh_final / k_sign_final: kMdBlocks = kMsBlocks = 1024 blocks of 256
INF = math.inf


def sheet(cells, step, z=0.0):
    """A flat cells x cells grid in the plane `z` from the origin, two triangles per cell split along the same diagonal, normals +z."""
    k = cells + 1
    ix, iy = np.meshgrid(np.arange(k, dtype=np.float64), np.arange(k, dtype=np.float64), indexing="ij")
    v = np.stack([ix * step, iy * step, np.full_like(ix, z)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij")
    v00 = (i * k + j).reshape(-1)
    v10, v01, v11 = v00 + k, v00 + 1, v00 + k + 1
    t = np.stack([np.stack([v00, v10, v11], -1), np.stack([v00, v11, v01], -1)], 1).reshape(-1, 3).astype(np.int32)
    return v, t


def band(sign_model, d2):
    """The rounding band of test_gpu_mesh_sign._check_sign, on a model result."""
    g, N = sign_model["g"], sign_model["N"]
    return ~(np.abs(g) > 2.0 ** -40 * np.sqrt(d2) * np.linalg.norm(N, axis=1)) & (d2 > 0) & ~sign_model["structural"]


def models(v, t, q, chunk=256):
    """(distance model, topology model, sign model) of one case."""
    dist = R.distance(q, v, t, chunk=chunk)
    topo = S.topology(v, t)
    return dist, topo, S.signed(q, v, t, dist, topo)


# ---- A: the strided totals and the gates at equality ----
A_SIZES = (ROUND + 1, 2 * ROUND + 300)
A_GATE = 13.0 / 8.0  # D: D * D = 169/64 is exact, and no lattice point has it (169 is no sum of three squares <= 8^2)
A_THRESHOLDS = (3.0 / 8.0, 5.0 / 4.0)


def _off_faces(d):
    """four points at distance d off the interior of four different faces of the unit cube: d2 == d * d exactly"""
    return np.array([[0.25, 0.5, -d], [-d, 0.25, 0.75], [0.75, -d, 0.25], [1.0 + d, 0.5, 0.25]])


def _in_faces(depth):
    """four points inside the unit cube whose nearest face (one each, four different ones) is `depth` away"""
    return np.array([[depth, 0.5, 0.5625], [1.0 - depth, 0.5, 0.4375], [0.5, depth, 0.5625], [0.5625, 0.5, 1.0 - depth]])


def tie_slots(n, j):
    """The four original indices of tie group j: in the first round of a block, a later round of the same block where n has one,
    another block, and one of the last indices (n - 1 for group 0)."""
    first = 257 * j
    slots = [first, first + ROUND if first + ROUND < n else 256 * (900 + j) + 200, 256 * (500 + j) + 100, n - 1 - j]
    if len(set(slots)) < 4:  # (n = ROUND + 1: index ROUND is both the only later round and n - 1)
        slots.append(256 * (900 + j) + 200)
    return np.array(sorted(set(slots)), np.int64)


def _ulp_triple(T):
    """Three points beyond the cube's vertex at the origin, whose closest point is that vertex (c = 0, so p - c = p exactly):
    d2 == T * T, d2 == the next double above, d2 == the next double below.  Found by search over (dx, dy, dz) with dx, dy powers of two
    and dz within 3 ulp of T, evaluated as the routine does: (dx dx + dy dy) + dz dz."""
    T2 = T * T
    want = {"eq": T2, "above": np.nextafter(T2, INF), "below": np.nextafter(T2, 0.0)}
    out = {"eq": np.array([0.0, 0.0, -T])}
    u = np.spacing(T)
    for name in ("above", "below"):
        for k in range(0, 4):
            dz = T - k * u if name == "below" else T + k * u
            for a in range(-20, -45, -1):
                for b in [None] + list(range(a, -45, -1)):
                    dx, dy = 2.0 ** a, 0.0 if b is None else 2.0 ** b
                    if (dx * dx + dy * dy) + dz * dz == want[name] and name not in out:
                        out[name] = np.array([-dx, -dy, -dz])
    assert set(out) == set(want), (T, sorted(out))
    return out


@functools.lru_cache(maxsize=None)
def case_a(n):
    """n queries against the 12-triangle unit cube, in an order no spatial sort keeps (the lattice is drawn at random, so the cloud's
    sorted order differs from the upload order)."""
    v, t = S.cube()
    rng = np.random.default_rng(n)
    q = rng.integers(-8, 17, size=(n, 3)).astype(np.float64) / 8.0  # the dyadic lattice of step 1/8 over [-1, 2]^3
    deep = ((q >= 0.375) & (q <= 0.625)).all(axis=1)  # deeper than 1/4 inside: moved out, the smallest signed distance is the group's
    q[deep, 0] += 1.0
    on = np.vstack([v, (v[t][:, 0] + v[t][:, 1]) / 2.0])  # d2 == +0.0: the vertices and the midpoints of the edges
    q[3000:3000 + len(on)] = on
    groups = {"max_d": (_off_faces(2.0), tie_slots(n, 0)), "gate": (_off_faces(A_GATE), tie_slots(n, 1)),
              "min_signed": (_in_faces(0.3125), tie_slots(n, 2))}
    for pts, slots in groups.values():
        q[slots] = pts
    ulp, at = {}, 2000
    for name, T in (("gate", A_GATE), ("t_lo", A_THRESHOLDS[0]), ("t_hi", A_THRESHOLDS[1])):
        tr = _ulp_triple(T)
        ulp[name] = {"T": T, "eq": at, "above": at + 1, "below": at + 2}
        q[at], q[at + 1], q[at + 2] = tr["eq"], tr["above"], tr["below"]
        at += 3
    return {"v": v, "t": t, "q": np.ascontiguousarray(q), "groups": {k: s for k, (_, s) in groups.items()}, "ulp": ulp,
            "gate": A_GATE, "thresholds": A_THRESHOLDS}


@functools.lru_cache(maxsize=None)
def case_a_models(n):
    """The 12-column brute force over case A's queries, computed once per process and shared (read-only)."""
    c = case_a(n)
    return models(c["v"], c["t"], c["q"], chunk=8192)


# ---- B: bit-equal distances to triangles in different subtrees ----
B_ORDERS = ("as_generated", "reversed", "permuted")


@functools.lru_cache(maxsize=None)
def case_b(shifted=False):
    """Two parallel 16 x 16-cell sheets (cells of 1/4) at z = 0 and z = 1: 1024 triangles, depth 4; the Morton code's top z bit parts
    the sheets, so a query at z = 1/2 has bit-equal minima in the two halves of the tree.  "orders": the caller's triangle list as
    generated, reversed (the lower caller index is in the box visited later) and in a fixed random permutation.  Within one flat sheet
    the closest point is unique, so its two far ends never tie by themselves; the queries far outside on the mid plane (`far`) tie the
    near rim of one sheet with that of the other, across the root's children."""
    v0, t0 = sheet(16, 0.25, 0.0)
    v1, t1 = sheet(16, 0.25, 1.0)
    v, t = np.vstack([v0, v1]), np.vstack([t0, t1 + len(v0)]).astype(np.int32)
    c = (np.arange(16) + 0.5) / 4.0
    k = np.arange(17) / 4.0
    grid = lambda x, y: np.stack(np.meshgrid(x, y, indexing="ij"), -1).reshape(-1, 2)
    xy = np.vstack([grid(c, c), grid(k, k), grid(c, k), grid(k, c), grid(c + 0.0625, c - 0.0625)])  # centres, corners, edge midpoints, faces
    out = np.array([-0.5, 4.5])
    rim = np.vstack([grid(out, np.arange(-1, 10) / 2.0), grid(np.arange(-1, 10) / 2.0, out)])  # beyond the rims and the corners
    far = np.array([[2.0, -6.0], [2.0, 10.0], [-6.0, 2.0], [10.0, 2.0], [-6.0, -6.0], [10.0, 10.0], [-6.0, 10.0], [10.0, -6.0]])
    mid = np.vstack([xy, rim, far])
    q = np.vstack([np.column_stack([mid, np.full(len(mid), 0.5)]),  # the mid plane: equidistant from the two sheets
                   np.column_stack([grid(c[::2], c[::2]), np.full(64, 0.25)]), np.column_stack([grid(k[::2], k[::2]), np.full(81, 0.75)])])
    if shifted:
        off = np.array([1024.0, -1024.0, 1024.0])
        v, q = v + off, q + off
    orders = {"as_generated": np.arange(len(t)), "reversed": np.arange(len(t))[::-1].copy(),
              "permuted": np.random.default_rng(20).permutation(len(t))}
    return {"v": v, "t": t, "q": np.ascontiguousarray(q), "orders": orders, "n_mid": len(mid)}


@functools.lru_cache(maxsize=None)
def case_b_model(shifted, order):
    c = case_b(shifted)
    return R.distance(c["q"], c["v"], np.ascontiguousarray(c["t"][c["orders"][order]]), chunk=128)


# ---- C and D: g == 0 beside a flat sheet, and the sheet with every triangle added again reversed ----
def _around_unit_square():
    """in the plane z = 0 beyond the rim of [0, 1]^2 (off an edge's interior: 1/8, 1/2, 7/8; off a grid vertex: 1/4) and its corners"""
    out = []
    for s in (0.125, 0.25, 0.5, 0.875):
        out += [[-0.5, s], [1.5, s], [s, -0.5], [s, 1.5]]
    out += [[-0.5, -0.5], [1.5, 1.5], [-0.5, 1.5], [1.5, -0.5], [-0.25, -0.5], [1.0, 1.5], [1.5, 0.0]]
    return np.array(out)


def case_c():
    """One flat 4 x 4-cell sheet over [0, 1]^2.  "plane": in-plane queries (p - c lies in the sheet's plane, every pseudo-normal there is
    (0, 0, w) with w != 0, so g == 0 exactly: the last `else` of k_mesh_sign); "up" / "down": the same lifted by +-1/8."""
    v, t = sheet(4, 0.25)
    xy = _around_unit_square()
    z = np.zeros(len(xy))
    return {"v": v, "t": t, "plane": np.column_stack([xy, z]), "up": np.column_stack([xy, z + 0.125]), "down": np.column_stack([xy, z - 0.125])}


def case_d():
    """The sheet of C as triangle soup (three private vertices per triangle) and every triangle once more reversed over the same three
    indices: every edge has m == 2 with opposite directions (closed, consistent, oriented_manifold), and every edge sum and vertex sum
    is n^ - n^ == 0 exactly.  (Over welded vertices an inner edge would carry four triangles and be NONMANIFOLD.)  The front copy
    (normal +z) has the lower caller index, so it wins the bit-equal tie with its reverse: a face query is signed as by a one-sided sheet."""
    sv, st = sheet(4, 0.25)
    v = sv[st].reshape(-1, 3)
    front = np.arange(3 * len(st), dtype=np.int32).reshape(-1, 3)
    t = np.vstack([front, front[:, [0, 2, 1]]]).astype(np.int32)
    corner = np.stack(np.meshgrid(np.arange(4) / 4.0, np.arange(4) / 4.0, indexing="ij"), -1).reshape(-1, 2)
    inner = np.vstack([corner + [0.1875, 0.0625], corner + [0.0625, 0.1875]])  # strictly inside the lower and the upper triangle of a cell
    z = np.zeros(len(inner))
    xy = _around_unit_square()
    node = np.array([[0.25, 0.25], [0.5, 0.75], [0.375, 0.25], [0.375, 0.375]])  # over a soup vertex, an edge midpoint, a diagonal
    off = np.vstack([np.column_stack([xy, np.zeros(len(xy))]), np.column_stack([xy, np.full(len(xy), 0.125)]),
                     np.column_stack([node, np.full(4, 0.125)]), np.column_stack([node, np.full(4, -0.125)])])
    return {"v": v, "t": t, "n_front": len(st), "face_up": np.column_stack([inner, z + 0.125]), "face_down": np.column_stack([inner, z - 0.125]),
            "on": np.column_stack([np.vstack([inner, node]), np.zeros(len(inner) + 4)]), "off": off}


# ---- E: runs of equal keys longer than a block ----
E_RUN = 300


def _ring():
    """300 dyadic points counter-clockwise round the square |x|, |y| <= 1: 75 per side, 1/64 apart from the side's first corner"""
    s = np.arange(75) / 64.0
    one = np.ones(75)
    return np.vstack([np.column_stack([-1 + s, -one]), np.column_stack([one, -1 + s]), np.column_stack([1 - s, one]), np.column_stack([-one, 1 - s])])


def _padding(n_pad, n_unref):
    """n_unref unreferenced vertices, then n_pad small far-away triangles over 3 n_pad vertices of their own: 3 n_pad edge records and
    3 n_pad corner records whose keys are below every key of the mesh that follows"""
    unref = np.column_stack([np.arange(n_unref) / 8.0, np.full(n_unref, -9.0), np.zeros(n_unref)])
    k = np.arange(n_pad, dtype=np.float64)
    a = np.column_stack([8.0 + k / 4.0, np.full(n_pad, 8.0), np.zeros(n_pad)])
    v = np.vstack([unref, np.stack([a, a + [0.125, 0.0, 0.0], a + [0.0, 0.125, 0.0]], 1).reshape(-1, 3)])
    t = (n_unref + np.arange(3 * n_pad)).reshape(-1, 3)
    return v, t


E_LANES = {255: 85, 0: 256}  # lane of the long run's head -> padding triangles in front of it (3 * 85 = 255, 3 * 256 = 768)


def case_e(kind, lane):
    """kind "fan": 300 flat triangles round one hub, a run of 300 corner records; kind "fin": 300 triangles on the edge (a, b), a run of
    300 edge records and two runs of 300 corner records.  The head of the long run stands at record 3 * E_LANES[lane]: lane 255 of
    block 0 or lane 0 of block 3; either way the run crosses into the next block.  The fin's third vertices all lie on the side x = 1,
    so its edge sum and vertex sums do not cancel."""
    pv, pt = _padding(E_LANES[lane], 5)
    base = len(pv)
    rng = np.random.default_rng(300 + lane)
    if kind == "fan":
        ring = _ring()
        v = np.vstack([pv, [[0.0, 0.0, 0.0]], np.column_stack([ring, np.zeros(E_RUN)])])
        i = np.arange(E_RUN)
        t = np.vstack([pt, np.column_stack([np.full(E_RUN, base), base + 1 + i, base + 1 + (i + 1) % E_RUN])]).astype(np.int32)
        q = np.column_stack([rng.integers(-96, 97, (E_RUN, 2)) / 64.0, rng.choice([-0.5, -0.25, -0.125, 0.125, 0.25, 0.5], E_RUN)])
        q[-6:] = v[[base, base + 1, base + 76, base + 151, base + 226, base + 40]]  # on the hub and on the rim
        q[-12:-6, :2], q[-12:-6, 2] = 0.0, [-0.5, -0.25, -0.125, 0.125, 0.25, 0.5]  # over the hub: the vertex pseudo-normal decides
    else:
        y = (np.arange(E_RUN) - 150) / 128.0
        v = np.vstack([pv, [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], np.column_stack([np.ones(E_RUN), y, np.full(E_RUN, 0.5)])])
        t = np.vstack([pt, np.column_stack([np.full(E_RUN, base), np.full(E_RUN, base + 1), base + 2 + np.arange(E_RUN)])]).astype(np.int32)
        q = np.column_stack([rng.integers(-32, 97, E_RUN), rng.integers(-96, 97, E_RUN), rng.integers(-32, 97, E_RUN)]) / 64.0
        q[:, 1] += 2.0 ** -14  # (a fin's plane is y = x (i - 150) / 128, a multiple of 2^-13 at these x: no query lies in one, where g == 0)
        q[-3:] = v[[base, base + 1, base + 2]]
    return {"v": v, "t": t, "q": np.ascontiguousarray(q), "head": 3 * E_LANES[lane], "first": base, "kind": kind}


# ---- F: the key packing at powers of two ----
F_NV = (7, 8, 9, 15, 16, 17, 255, 256, 257)


def case_f(nv):
    """The cube (the octahedron for nv = 7: the cube alone has 8 vertices) with unreferenced vertices up to nv, and three more triangles:
    (0, nv-2, nv-1) FIRST in the caller's order, (nv-1, nv-2, 1) and (nv-1, nv-1, 0) last.  The first two share the edge (nv-2, nv-1),
    the largest real key, in opposite directions, and their records of that edge and of the vertices nv-2 and nv-1 are emitted before
    and after all of the cube's: a sort that drops a key's top bit lets the cube's records in between.  The edges (0, nv-1) and
    (1, nv-1) are one key if `bits` is one too small.  The last triangle names a vertex twice and emits no_edge."""
    v, t = S.octahedron() if nv < 8 else S.cube()
    k = np.arange(nv - len(v))
    v = np.vstack([v, np.column_stack([2.0 + (k // 16) / 8.0, (k % 16) / 8.0, np.full(len(k), 3.0)])])
    nb = len(t)
    t = np.vstack([[[0, nv - 2, nv - 1]], t, [[nv - 1, nv - 2, 1], [nv - 1, nv - 1, 0]]]).astype(np.int32)
    return {"v": v, "t": t, "top_edge": ((0, 1), (nb + 1, 0)), "twice": nb + 2}


# ---- G: a degenerate triangle sharing an edge with a real one ----
def case_g(kind, degenerate_first):
    """kind "pair": the real triangle A B C and the collinear B A M (M on the line A B beyond B; it runs the shared edge against the
    real one, so the edge is consistent).  kind "cube": the cube with one cube edge split on one side only and the T-junction filled by
    the collinear triangle (S.with_degenerate).  The degenerate triangle is the first or the last in the caller's order: with equal
    distance to the shared edge it wins, or loses, by its index.  "shared": (triangle, local edge, the one real triangle) per side."""
    if kind == "pair":
        v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]])
        real, deg = [0, 1, 2], [1, 0, 3]
        t = np.array([deg, real] if degenerate_first else [real, deg], np.int32)
        i_deg, i_real = (0, 1) if degenerate_first else (1, 0)
        x = np.array([0.125, 0.5, 0.875])
        q = np.vstack([np.column_stack([x, np.full(3, -0.5), np.full(3, 0.25)]), np.column_stack([x, np.full(3, -0.5), np.full(3, -0.25)]),
                       [[0.25, 0.25, 0.5], [0.25, 0.25, -0.5], [1.5, -0.25, 0.25], [2.5, 0.0, 0.25], [0.5, 0.0, 0.0]]])
        return {"v": v, "t": t, "q": q, "deg": i_deg, "shared": ((i_real, 0), (i_deg, 0), i_real), "n_tie": 6}
    cv, ct = S.cube()
    ct = ct.copy()
    ct[0] = np.roll(ct[0], -1)  # (0, 2, 1) -> (2, 1, 0): its edge A B is now the cube edge x = 1, z = 0
    v, t = S.with_degenerate(cv, ct)
    assert (v[-1] == [1.0, 0.5, 0.0]).all() and list(t[-1]) == [2, 1, 8]
    nt = len(t)
    if degenerate_first:
        t = np.vstack([t[-1:], t[:-1]]).astype(np.int32)
    i_deg = 0 if degenerate_first else nt - 1
    i_nb = next(k for k in range(nt) if k != i_deg and any(t[k, e] == 1 and t[k, (e + 1) % 3] == 2 for e in range(3)))  # runs B -> A
    e_nb = next(e for e in range(3) if t[i_nb, e] == 1 and t[i_nb, (e + 1) % 3] == 2)
    y = np.array([0.125, 0.25, 0.5, 0.75, 0.875])
    q = np.vstack([np.column_stack([np.full(5, 1.25), y, np.full(5, -0.25)]), np.column_stack([np.full(5, 1.5), y, np.full(5, -0.125)]),
                   [[0.5, 0.5, 0.5], [0.25, 0.5, 0.25], [1.5, 0.5, 0.5], [0.5, 0.5, -1.0], [2.0, 2.0, -1.0], [1.0, 0.25, 0.0]]])
    return {"v": v, "t": t, "q": q, "deg": i_deg, "shared": ((i_nb, e_nb), (i_deg, 0), i_nb), "n_tie": 10}


# ---- H: the sampler around zero-area triangles ----
def case_h():
    """A 6 x 6 heightfield (heights k/8) with zero-area triangles at the caller's positions 0 (collinear), nt // 2 (a repeated index)
    and nt - 1 (collinear): cum[0] == 0, cum[nt // 2] == cum[nt // 2 - 1], cum[nt - 1] == cum[nt - 2] == the total."""
    v, t = sheet(5, 0.5)
    i = np.arange(36)
    v[:, 2] = ((3 * (i // 6) ** 2 + 5 * (i % 6) + (i // 6) * (i % 6)) % 7) / 8.0
    nv = len(v)
    v = np.vstack([v, [[0.0, 0.0, 1.0], [1.0, 0.5, 1.0], [3.0, 1.5, 1.0]]])  # three collinear points
    col = [nv, nv + 1, nv + 2]
    t = [list(x) for x in t]
    t = [col] + t[:25] + [[7, 7, 20]] + t[25:] + [[col[2], col[0], col[1]]]
    t = np.array(t, np.int32)
    assert len(t) == 53 and list(t[len(t) // 2]) == [7, 7, 20]
    return {"v": v, "t": t, "zero": (0, len(t) // 2, len(t) - 1), "n": 100003, "seeds": (77, 2 ** 40 + 5)}
