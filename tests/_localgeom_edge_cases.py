"""Hand-built clouds for me_local_geometry / me_radius_normals (csrc/me_localgeom.hip) at their exact edges, and the exact model.

Every cloud lies on a dyadic lattice (multiples of 2^-3 .. 2^-5 within a few units of the origin, or of a dyadic offset), so every
d = p_j - q, every product of two of them and all nine sums of a neighbourhood are exact in fp64 in whatever order the stream
delivers the candidates (test_localgeom_edges_cpu.py recomputes them in exact rational arithmetic).  From the exact sums the
kernel's epilogue is one fixed sequence of fp64 operations (the file is compiled with -ffp-contract=off; + - * / and sqrt are
correctly rounded), restated here in scalar Python: model() is the expectation for eig, k and valid BIT FOR BIT, model_normals()
for the normals of me_radius_normals.

A cloud is handed to the engine through shuffled(): a seeded permutation, so that cloud order and sorted order differ."""
import math

import numpy as np
from scipy.spatial import cKDTree

from _globreg_ref import jacobi_sym

FAR = np.array([2.0 ** 19, -(2.0 ** 18), 2.0 ** 6])  # a dyadic, survey-sized offset: differences of coordinates stay exact


# ---- the exact model -----------------------------------------------------------------------------------------------------------------
def moments(xyz, r):
    """-> (k[n] int64, s[n, 9] fp64): the neighbour count (d2 < r*r, the query itself removed, coincident copies kept) and
    sx sy sz sxx sxy sxz syy syz szz with d = p_j - q, the kernel's own expressions.  Exact on the clouds of this file."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    k = np.zeros(n, np.int64)
    s = np.zeros((n, 9))
    if n < 2:
        return k, s
    pairs = cKDTree(xyz).query_pairs(r * (1.0 + 1e-6), output_type="ndarray")  # a superset; the kernel's test decides
    i = np.concatenate([pairs[:, 0], pairs[:, 1]])
    j = np.concatenate([pairs[:, 1], pairs[:, 0]])
    d = xyz[j] - xyz[i]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    keep = (dx * dx + dy * dy) + dz * dz < r * r
    i, dx, dy, dz = i[keep], dx[keep], dy[keep], dz[keep]
    k = np.bincount(i, minlength=n).astype(np.int64)
    for c, w in enumerate((dx, dy, dz, dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz)):
        s[:, c] = np.bincount(i, weights=w, minlength=n)
    return k, s


def epilogue(k, s):
    """local_geom_body after the stream, operation for operation, for one point with k >= min_k.
    -> (ok, (l1, l2, l3), d, V): d and V as jacobi_sym left them (eigenvalues before the clamp, eigenvectors in the columns)."""
    sx, sy, sz, sxx, sxy, sxz, syy, syz, szz = s
    kd, km = float(k), float(k - 1)
    a0 = (sxx - sx * sx / kd) / km
    a4 = (syy - sy * sy / kd) / km
    a8 = (szz - sz * sz / kd) / km
    a1 = (sxy - sx * sy / kd) / km
    a2 = (sxz - sx * sz / kd) / km
    a5 = (syz - sy * sz / kd) / km
    d, V = jacobi_sym(3, [a0, a1, a2, a1, a4, a5, a2, a5, a8])
    # fmax(d, 0.0): a negative value and either zero give +0.0 here (the CPU test asserts that no d is -0.0 on these clouds, the
    # one input on which fmax may return either zero)
    e0, e1, e2 = (x if x > 0.0 else 0.0 for x in d)
    if e0 < e1:
        e0, e1 = e1, e0
    if e1 < e2:
        e1, e2 = e2, e1
    if e0 < e1:
        e0, e1 = e1, e0
    ok = e0 > 0.0
    return ok, ((e0, e1, e2) if ok else (0.0, 0.0, 0.0)), d, V


def _normal_of(d, V):
    """the column of the smallest eigenvalue before the clamp, the lowest index among equal ones, scaled to unit length"""
    b1 = d[1] < d[0]
    dm = d[1] if b1 else d[0]
    b2 = d[2] < dm
    c = 2 if b2 else (1 if b1 else 0)
    nx, ny, nz = V[c], V[3 + c], V[6 + c]
    ln = math.sqrt((nx * nx + ny * ny) + nz * nz)
    return nx / ln, ny / ln, nz / ln


def model(xyz, r, min_k, with_raw=False, mom=None):
    """-> (eig[n, 3], k[n] int32, valid[n] uint8) as me_local_geometry_fetch returns them; with_raw: also (d[n, 3], normal[n, 3]),
    the eigenvalues before the clamp and the unoriented unit normal (zeros where the point is invalid).  Points with the same k and
    sums share one epilogue (a lattice has few distinct neighbourhoods)."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    k, s = moments(xyz, r) if mom is None else mom
    n = len(xyz)
    eig = np.zeros((n, 3))
    valid = np.zeros(n, np.uint8)
    raw = np.zeros((n, 3))
    nrm = np.zeros((n, 3))
    memo = {}
    for i in np.flatnonzero(k >= min_k):
        key = (int(k[i]), *s[i].tolist())
        if key not in memo:
            ok, l, d, V = epilogue(key[0], key[1:])
            memo[key] = (ok, l, d, _normal_of(d, V) if ok else (0.0, 0.0, 0.0))
        ok, l, d, nv = memo[key]
        eig[i], valid[i], raw[i], nrm[i] = l, ok, d, nv
    out = (eig, k.astype(np.int32), valid)
    return out + (raw, nrm) if with_raw else out


def model_normals(xyz, r, min_k, viewpoint=None, invalid_z=False, mom=None):
    """the normals of me_radius_normals in cloud order: the unit column, flipped iff (n . (viewpoint - q)) < 0 (strict), and
    (0, 0, 0) or, with invalid_z, (0, 0, 1) where the point is invalid"""
    xyz = np.ascontiguousarray(xyz, np.float64)
    _, _, valid, _, nrm = model(xyz, r, min_k, with_raw=True, mom=mom)
    out = nrm.copy()
    if viewpoint is not None:
        v = np.asarray(viewpoint, np.float64)[None, :] - xyz
        dot = (out[:, 0] * v[:, 0] + out[:, 1] * v[:, 1]) + out[:, 2] * v[:, 2]
        flip = (dot < 0.0) & (valid != 0)
        out[flip] = -out[flip]
    if invalid_z:
        out[valid == 0, 2] = 1.0
    return out


def features(eig):
    """(l3, linearity, planarity, sphericity, surface variation) per row, the kernel's expressions; rows with l1 > 0"""
    l1, l2, l3 = eig[:, 0], eig[:, 1], eig[:, 2]
    return np.stack([l3, (l1 - l2) / l1, (l2 - l3) / l1, l3 / l1, l3 / ((l1 + l2) + l3)], 1)


SUM_FIELDS = ("sum_l3", "sum_linearity", "sum_planarity", "sum_sphericity", "sum_surface_variation")


def totals(eig, k, valid):
    """n_valid, sum_k and the five fp64 rows by math.fsum (the correctly rounded sum: THE sum wherever it is representable)"""
    v = valid.astype(bool)
    f = features(eig[v]) if v.any() else np.zeros((0, 5))
    out = {"n_valid": int(v.sum()), "sum_k": int(k[v].astype(np.int64).sum())}
    for c, name in enumerate(SUM_FIELDS):
        out[name] = math.fsum(f[:, c])
    return out


def shuffled(xyz, seed):
    """-> (cloud in a seeded random order, perm): cloud[i] = xyz[perm[i]], so a per-point result r of the cloud is r[inv] in the
    order of xyz, inv = argsort(perm)"""
    perm = np.random.default_rng(seed).permutation(len(xyz))
    return np.ascontiguousarray(xyz[perm]), perm


# ---- case 1 / 2: ties at the radius --------------------------------------------------------------------------------------------------
TIE_STEP = 1.0 / 8
TIE_HALF = 6
TIE_R = 5.0 / 8
TIE_R_IN = TIE_R * (1.0 + 2.0 ** -30)
TIE_MIN_K = 5


def tie_lattice():
    """A cubic lattice of step 1/8, 13 x 13 x 13 (the lattice of test_gpu_search.py with 13 layers instead of 7: a ball of 5 steps
    needs 5 layers on either side before any point has a whole one).  At r = 5/8 the offsets 3-4-0 and 5-0-0 have d2 == r*r."""
    g = np.arange(-TIE_HALF, TIE_HALF + 1)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return ijk * TIE_STEP, ijk


def tie_counts(ijk, inclusive):
    """k per lattice point in integers: offsets with i^2 + j^2 + k^2 < 25 (<= 25 when inclusive), clipped at the border"""
    h = TIE_HALF
    occ = np.zeros((2 * h + 11,) * 3, np.int64)
    occ[5:5 + 2 * h + 1, 5:5 + 2 * h + 1, 5:5 + 2 * h + 1] = 1
    k = np.zeros(len(ijk), np.int64)
    for a in range(-5, 6):
        for b in range(-5, 6):
            for c in range(-5, 6):
                q = a * a + b * b + c * c
                if q == 0 or q > 25 or (q == 25 and not inclusive):
                    continue
                k += occ[ijk[:, 0] + h + 5 + a, ijk[:, 1] + h + 5 + b, ijk[:, 2] + h + 5 + c]
    return k


def tie_interior(ijk):
    """the points whose whole ball of 5 steps lies in the lattice"""
    return np.all(np.abs(ijk) <= TIE_HALF - 5, axis=1)


# ---- case 3: sizes around a wave, a block and the reduction's chunk ------------------------------------------------------------------
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 513, 65537)
SHEET_R = 17.0 / 128  # r^2 = 4.52 steps^2: a middle-layer point of the interior has k = 30, an outer-layer one k = 22
SHEET_MIN_KS = (2, 23)  # 23: the outer layers are invalid, the middle layer valid, inside every wave


def sheet(n):
    """the first n points of a three-layer sheet of step 1/16, 16 columns wide: point t is layer t % 3, column (t / 3) % 16, row
    t / 48.  From 49 points on the cut is three-dimensional."""
    t = np.arange(n)
    return np.stack([((t // 3) % 16) / 16.0, (t // 48) / 16.0, (t % 3) / 16.0], 1)


# ---- case 4: the totals, exactly -----------------------------------------------------------------------------------------------------
CL_U = 2.0 ** -5
CL_R = 17 * CL_U
CL_MIN_K = 9
CL_SPACING = 2.0
CL_SIDE = 19
CL_COUNT = 6554  # x 10 points = 65540 >= 65537: 257 blocks
# (axis of the two-pair arm, axis of the 16-unit pair, axis of the last pair), lengths of the arm's pairs, length of the last pair:
# all in (r / 2, r) units of 2^-5, so that the centre sees all eight and an outer point never its mirror image
CL_SHAPES = (((0, 1, 2), (9, 12), 10), ((2, 0, 1), (9, 10), 13), ((1, 2, 0), (10, 11), 15), ((0, 2, 1), (9, 13), 9),
             ((1, 0, 2), (10, 12), 11), ((2, 1, 0), (9, 11), 14), ((0, 1, 2), (9, 10), 12))


def cluster(shape):
    """ten points about the origin: the centre twice, two mirror pairs along one axis, one pair of 16 units along a second, one
    along the third.  Each copy of the centre sees the other copy and the eight outer points: k = 9, sx = sy = sz = 0, a diagonal
    covariance sum(2 L^2) / 8, whose largest entry is 2 * 16^2 / 8 units^2 = 2^-4 on the second axis."""
    (arm, big, last), (p1, p2), s = shape
    pts = [np.zeros(3), np.zeros(3)]
    for axis, length in ((arm, p1), (arm, p2), (big, 16), (last, s)):
        for sign in (1.0, -1.0):
            p = np.zeros(3)
            p[axis] = sign * length * CL_U
            pts.append(p)
    return np.array(pts)


def clusters(count=CL_COUNT):
    """`count` isolated clusters on a grid of spacing 2 (> r + 2 * 16 units: no point sees another cluster), the shapes in turn"""
    c = np.arange(count)
    centres = np.stack([c % CL_SIDE, (c // CL_SIDE) % CL_SIDE, c // (CL_SIDE * CL_SIDE)], 1) * CL_SPACING
    return np.concatenate([cluster(CL_SHAPES[i % len(CL_SHAPES)]) + centres[i] for i in range(count)])


DYADIC_ROWS = SUM_FIELDS[:4]  # sum_surface_variation = sum l3 / (l1 + l2 + l3) is not dyadic: l1 + l2 + l3 is no power of two
# (with l1 = L^2 / 4 a power of two, l1 + l2 + l3 = (sum of four squares) / 4 is one only if the four lengths are equal)


# ---- case 5: the index reuse window --------------------------------------------------------------------------------------------------
REUSE_C = 3.0 / 16
REUSE_MIN_K = 5


def reuse_lattice():
    """15 x 15 x 13 points of step 1/16"""
    ijk = np.stack(np.meshgrid(np.arange(15), np.arange(15), np.arange(13), indexing="ij"), -1).reshape(-1, 3)
    return ijk / 16.0


def reuse_radii(c=REUSE_C):
    """(r, index builds the call must launch) on an index of cell_size c, cell_h = c (1 + 2^-20): kept iff
    r (1 + 2^-20) <= cell_h <= 1.5 r (1 + 2^-20)"""
    return ((c * (1.0 + 2.0 ** -10), 1),  # the cell is smaller than the radius
            (c, 0),  # cell_h == r (1 + 2^-20): the closed tight end
            (c * (1.0 - 2.0 ** -30), 0),  # just inside it
            (c / 1.25, 0),
            (c / 1.5 * (1.0 + 2.0 ** -10), 0),  # just inside the wide end
            (c / 1.5 * (1.0 - 2.0 ** -10), 1))  # just past it


# ---- case 6: frame borders and far coordinates ---------------------------------------------------------------------------------------
BORDER_R = 5.0 / 16
BORDER_MIN_K = 5


def border_lattice(isolated):
    """11 x 11 x 11 points of step 1/8 about the origin: alone, its faces are the cloud's bounding box and those queries sit in the
    border cells of the index frame.  isolated: six more points 4 r beyond the faces, one per axis direction, with k == 0."""
    g = np.arange(-5, 6) / 8.0
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    if isolated:
        far = 5.0 / 8 + 4 * BORDER_R
        xyz = np.concatenate([xyz, far * np.concatenate([np.eye(3), -np.eye(3)])])
    return xyz


# ---- case 7: the viewpoint flip ------------------------------------------------------------------------------------------------------
VIEW_R = 17.0 / 128
VIEW_MIN_K = 5


def view_sheet():
    """12 x 12 points of step 1/16 in the layers z = 0 and z = 1/16.  An interior point has a diagonal covariance with the
    smallest entry on z: its normal is exactly (0, 0, 1), and a viewpoint at its own height gives dot == 0."""
    ijk = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    return ijk / 16.0


def view_interior(xyz):
    """the points at least 2 steps from every edge of the sheet (r < 2.2 steps)"""
    ij = np.rint(xyz[:, :2] * 16).astype(int)
    return np.all((ij >= 2) & (ij <= 9), axis=1)
