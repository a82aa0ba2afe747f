"""The inputs of tests/test_m3c2_edges_cpu.py and tests/test_gpu_m3c2_edges.py: cloud pairs built to reach, exactly, the places of
csrc/me_m3c2.hip that random sheets do not: the strided loop of k_m3_final, the clamp of k_m3_stream<true> into the other cloud's
Morton frame at both ends of every axis, waves whose lanes sit in unrelated cells, runs longer than a wave tile, and the gates of
k_m3_final at equality.  Pure numpy.  Apart from case B every coordinate is a small multiple of 2^-8 and every normal an axis, so t,
S and Q are exact whatever the order of the sums (_m3c2_ref.order_free) and _m3c2_ref.m3c2_fp64 gives the device's bits.
Each generator returns a dict with "own", "other", "nrm", the parameters, the model and the facts the tests assert; the results are
cached, so the CPU test and the device test of one session share one model."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

import _m3c2_ref as R

BLOCKS = 1024  # kM3Blocks of csrc/me_m3c2.hip: above 256 * BLOCKS core points a block of k_m3_final strides over the array
MORTON_BITS = 21  # kMortonBits: cells per axis of the finest lattice, as a power of two
U = 2.0 ** -53

# one cylinder for the cases B to E: rp = 3/16 and L = 4/16 make R = sqrt(L*L + rp*rp) = 5/16 exactly
RP, L, RB = 3.0 / 16.0, 4.0 / 16.0, 5.0 / 16.0
assert math.sqrt(L * L + RP * RP) == RB


def frame(points, R):
    """cloud_build_index (csrc/me_index.hip) restated for a cloud uploaded with cell_size = R: the Morton frame me_m3c2 finds (its
    own test keeps an index whose cell edge is R (1 + 2^-20)).  `builds` is False where the library refuses the cell size (more than
    2^21 cells per axis).  cells(x) gives the cell of every row of x in this frame per axis, as a double and unclamped, the way
    k_m3_stream<true> places a core point: floor(floor((x - origin) / fine_h) * 2^-shift)."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    cell_h = R * (1.0 + 2.0 ** -20)
    lo, hi = points.min(axis=0), points.max(axis=0)
    origin = np.floor(lo / cell_h) * cell_h
    extent = float((hi - origin).max())  # (from the origin, not from bbox_lo)
    ncell = math.floor(extent / cell_h) + 1.0
    bits = 1
    while float(1 << bits) < ncell and bits <= MORTON_BITS:
        bits += 1
    f = SimpleNamespace(cell_h=cell_h, origin=origin, ncell=ncell, bits=bits, builds=bits <= MORTON_BITS, lo=lo, hi=hi)
    if f.builds:
        f.cell_lim = 1 << bits
        f.shift = MORTON_BITS - bits
        f.fine_h = math.ldexp(cell_h, -f.shift)
        f.cells = lambda x: np.floor(np.floor((np.asarray(x, np.float64).reshape(-1, 3) - origin) / f.fine_h) * 2.0 ** -f.shift)
    return f


def _axis(a, sign=1.0):
    v = np.zeros(3)
    v[a] = sign
    return v


# ---- A: more core points than one round of k_m3_final, and four equal maxima ----
A_RP, A_L = 2.0, 1.5  # R = 2.5
A_REG = 0.28  # lod lands between the sheet's smallest and largest |dist|: both outcomes of the significance test occur
A_MIN = 5


@functools.lru_cache(maxsize=None)
def case_a():
    """own: a flat lattice sheet (step 1/8, z = 0, 512 points to the row) and four islands of five points, n = 256 * BLOCKS + 257 in
    all; other: a lattice of step 1 over four fifths of the sheet, 52 x 65, at heights 8/16 .. 11/16, and five points one unit above or below every
    island.  Every own member has t = 0; an other member's t is a multiple of 1/16.  The islands' cores have dist = +1, -1, -1, +1
    (the other cloud above or below, the normal +z or -z) at the original indices n - 1, 0, 256 * 700 + 13 and 131072; on the sheet
    |dist| <= 11/16."""
    n = 256 * BLOCKS + 257
    n_sheet = n - 20
    k = np.arange(n_sheet)
    i, j = k % 512, k // 512
    sheet = np.stack([i / 8.0, j / 8.0, np.zeros(n_sheet)], -1)
    sheet_nrm = np.where(((i + j) % 3 != 0)[:, None], _axis(2), _axis(2, -1.0))
    gi, gj = np.meshgrid(np.arange(52), np.arange(65), indexing="ij")  # (x <= 51: the sheet's last fifth has no other cloud over it)
    gi, gj = gi.reshape(-1), gj.reshape(-1)
    grid = np.stack([gi.astype(np.float64), gj.astype(np.float64), 0.5 + ((3 * gi + 5 * gj) % 4) / 16.0], -1)
    star = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    own_is, nrm_is, other_is = [], [], []
    for m, (side, nz) in enumerate(((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0))):
        c = np.array([16.0 * m, -16.0, 0.0])
        own_is.append(star + c)
        nrm_is.append(np.tile(_axis(2, nz), (5, 1)))
        other_is.append(star + c + [0.0, 0.0, side])
    own = np.concatenate([sheet] + own_is)
    nrm = np.concatenate([sheet_nrm] + nrm_is)
    other = np.concatenate([grid] + other_is)
    slots = np.array([n - 1, 0, 256 * 700 + 13, 131072])  # the cores of the four islands go to these original indices
    for m, s in enumerate(slots):
        c = n_sheet + 5 * m
        own[[c, s]] = own[[s, c]]
        nrm[[c, s]] = nrm[[s, c]]
    mask = np.zeros(n, np.uint8)
    mask[7::175] = 1
    mask[slots] = 1
    model = R.m3c2_fp64(own, other, nrm, A_RP, A_L, A_MIN, A_REG, mask)
    return {"own": np.ascontiguousarray(own), "other": np.ascontiguousarray(other), "nrm": np.ascontiguousarray(nrm), "mask": mask,
            "slots": slots, "model": model, "n": n}


# ---- B: the other frame's border ----
B_MIN = 3
B_FAR = 2.0 ** 20  # cells


@functools.lru_cache(maxsize=None)
def case_b():
    """other: the lattice k R / 4, k = 0 .. 16 per axis: it starts at the lattice's origin and ends at 4 R, just below 4 cell edges, so
    the frame has exactly 4 = cell_lim cells per axis, the first and the last populated.  own: every combination, over the three
    axes, of the quarter and three-quarter positions of the cells -2, -1, 0, 3, 4, 5 and the middles of the cells 1 and 2; per axis
    three points at and one ulp either side of the -2 | -1 and the cell_lim | cell_lim + 1 boundaries; one point 2^20 cells away.
    Random tilted unit normals: sets only."""
    f = frame(np.array([[0.0, 0.0, 0.0], [4 * RB, 4 * RB, 4 * RB]]), RB)
    h = f.cell_h
    k = np.arange(17) * (RB / 4.0)
    other = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    pos = [(c + q) * h for c in (-2, -1, 0, 3, 4, 5) for q in (0.25, 0.75)] + [1.5 * h, 2.5 * h]
    pos = np.array(sorted(pos))
    product = np.stack(np.meshgrid(pos, pos, pos, indexing="ij"), -1).reshape(-1, 3)
    ulp = []
    for a in range(3):
        for b in (-h, 5.0 * h):
            for x in (np.nextafter(b, -math.inf), b, np.nextafter(b, math.inf)):
                p = np.full(3, 0.25 * h)
                p[a] = x
                ulp.append(p)
    far = np.array([[B_FAR * h + 0.3, 0.25 * h, 0.75 * h]])
    own = np.ascontiguousarray(np.concatenate([product, np.array(ulp), far]))
    rng = np.random.default_rng(5)
    v = np.array([0.0, 0.0, 1.0]) + 0.4 * rng.standard_normal((len(own), 3))
    nrm = np.ascontiguousarray(v / np.linalg.norm(v, axis=1)[:, None])
    model = R.m3c2(own, other, nrm, RP, L, B_MIN, exact=False)
    return {"own": own, "other": np.ascontiguousarray(other), "nrm": nrm, "model": model, "n_product": len(product), "n_ulp": len(ulp),
            "far": len(own) - 1}


# ---- C: one lane, one cell ----
C_MIN = 3


@functools.lru_cache(maxsize=None)
def case_c():
    """144 core points one unit (3.2 R) apart on a 6 x 6 x 4 lattice, each with two own companions 1/16 away (masked out: they are
    there for n_own = 3) and five points of the other cloud 1/16 around a spot up to 3/32 off the core point; the normals run through
    +-x, +-y, +-z.  One stray point of the other cloud moves its bbox_lo, and with it its frame's origin, off the own cloud's.
    "lone" is the own cloud without the companions: every lane of its waves is pending, each in a cell of its own."""
    base = np.array([1.0 / 8.0, 1.0 / 8.0, 1.0 / 8.0])
    cores, comps, nrm_c, other = [], [], [], [np.array([[-0.5, -0.9, -0.2]])]
    idx = 0
    for i in range(6):
        for j in range(6):
            for k in range(4):
                c = base + [float(i), float(j), float(k)]
                a, sign = idx % 3, 1.0 if (idx // 3) % 2 == 0 else -1.0
                b1, b2 = (a + 1) % 3, (a + 2) % 3
                d = ((idx % 7) - 3) / 32.0
                cores.append(c)
                nrm_c.append(_axis(a, sign))
                comps += [c + _axis(b1, 1.0 / 16.0), c - _axis(b1, 1.0 / 16.0)]
                spot = c + _axis(a, d)
                other.append(np.array([spot + _axis(b1, 1.0 / 16.0), spot - _axis(b1, 1.0 / 16.0), spot + _axis(b2, 1.0 / 16.0),
                                       spot - _axis(b2, 1.0 / 16.0), spot + _axis(a, 1.0 / 64.0)]))
                idx += 1
    cores, comps, nrm_c = np.array(cores), np.array(comps), np.array(nrm_c)
    own = np.concatenate([cores, comps])
    nrm = np.concatenate([nrm_c, np.repeat(nrm_c, 2, axis=0)])
    mask = np.concatenate([np.ones(len(cores), np.uint8), np.zeros(len(comps), np.uint8)])
    perm = np.random.default_rng(9).permutation(len(own))  # cores and companions interleaved in cloud order
    own, nrm, mask = np.ascontiguousarray(own[perm]), np.ascontiguousarray(nrm[perm]), np.ascontiguousarray(mask[perm])
    other = np.ascontiguousarray(np.concatenate(other))
    lone, lone_nrm = np.ascontiguousarray(cores), np.ascontiguousarray(nrm_c)
    return {"own": own, "other": other, "nrm": nrm, "mask": mask, "model": R.m3c2_fp64(own, other, nrm, RP, L, C_MIN, 0.0, mask),
            "lone": lone, "lone_nrm": lone_nrm, "lone_model": R.m3c2_fp64(lone, other, lone_nrm, RP, L, 2)}


# ---- D: long runs and duplicates ----
D_RUNS = (63, 64, 65, 128, 129, 1000)
D_MIN = 5
D_DUPLICATES = 200


@functools.lru_cache(maxsize=None)
def case_d():
    """other: one point at the origin (it pins the frame) and six clusters, each inside one cell, four cells apart along x: the first
    63, 64, 65, 128, 129 and 1000 points of a 10 x 10 x 10 lattice of step 1/128 around the cell's middle.  own: per cluster one core
    point 1/32 off the cluster's middle along its normal, five times (200 times at the 129-cluster): coincident duplicates, all of
    them core points with d2 == 0 and t == 0 among themselves."""
    h = RB * (1.0 + 2.0 ** -20)
    mid = round(0.5 * h * 64) / 64.0
    a = (np.arange(10) - 4.5) / 128.0
    cube = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)  # (z fastest: a partial cluster still has depth)
    other, own, nrm, centres = [np.zeros((1, 3))], [], [], []
    for m, run in enumerate(D_RUNS):
        c = np.array([round((4 * (m + 1) + 0.5) * h * 64) / 64.0, mid, mid])
        normal = (_axis(2), _axis(2, -1.0), _axis(0), _axis(1, -1.0), _axis(2), _axis(0, -1.0))[m]
        copies = D_DUPLICATES if run == 129 else 5
        other.append(cube[:run] + c)
        own.append(np.tile(c - normal / 32.0, (copies, 1)))
        nrm.append(np.tile(normal, (copies, 1)))
        centres.append(c)
    own, nrm, other = np.ascontiguousarray(np.concatenate(own)), np.ascontiguousarray(np.concatenate(nrm)), np.ascontiguousarray(np.concatenate(other))
    return {"own": own, "other": other, "nrm": nrm, "centres": np.array(centres), "model": R.m3c2_fp64(own, other, nrm, RP, L, D_MIN)}


# ---- E: the gates of k_m3_final ----
E_MINS = (2, 5)
E_DIST = 1.0 / 16.0


@functools.lru_cache(maxsize=None)
def case_e_counts():
    """Eight islands two units apart: for m in (2, 5) and (a, b) in {m - 1, m}^2, `a` coincident own points (all core points, normal
    +z) and `b` points of the other cloud 1/16 above them in a row of step 1/64.  Every t of the other cloud is 1/16 and every own t
    is 0: wherever an island is valid, dist = 1/16 and both variances are exactly 0."""
    own, other, combos = [], [], []
    x = 0.0
    for m in E_MINS:
        for a in (m - 1, m):
            for b in (m - 1, m):
                own.append(np.tile([x, 0.0, 0.0], (a, 1)))
                other.append(np.array([[x + j / 64.0, 0.0, E_DIST] for j in range(b)]))
                combos += [(m, a, b)] * a
                x += 2.0
    own, other = np.ascontiguousarray(np.concatenate(own)), np.ascontiguousarray(np.concatenate(other))
    nrm = np.tile(_axis(2), (len(own), 1))
    return {"own": own, "other": other, "nrm": nrm, "combos": np.array(combos),
            "models": {m: R.m3c2_fp64(own, other, nrm, RP, L, m) for m in E_MINS}}


def lod_of(reg):
    """lod on a core point whose two variances are 0, as k_m3_final forms it"""
    return 1.96 * (math.sqrt(0.0 / 2.0 + 0.0 / 2.0) + reg)


@functools.lru_cache(maxsize=None)
def lod_triple(dist=E_DIST):
    """reg_error values among the 64 neighbours of dist / 1.96 either side whose lod is the largest below dist, equal to dist (None
    where no neighbour gives it) and the smallest above dist"""
    r = dist / 1.96
    for _ in range(64):
        r = np.nextafter(r, 0.0)
    below = equal = above = None
    for _ in range(129):
        lod = lod_of(float(r))
        if lod < dist:
            below = float(r)
        elif lod == dist and equal is None:
            equal = float(r)
        elif lod > dist and above is None:
            above = float(r)
        r = np.nextafter(r, math.inf)
    return below, equal, above


def identical_t_raw(n, c):
    """the raw variance (before the clamp) of n members that all have t == c: S and Q as a lane adds them"""
    return R.raw_variance(n, R.sequential_sum([c] * n), R.sequential_sum([c * c] * n))


@functools.lru_cache(maxsize=None)
def variance_pairs(want=3):
    """(n, c) with a NEGATIVE raw variance and (n, c) with a POSITIVE one, `want` of each, found by search over n = 5 .. 40 and the
    non-dyadic offsets c = k / 1000: all members share one t, so the exact variance is 0 and the raw value is rounding alone"""
    neg, pos = [], []
    for n in range(5, 41):
        for k in range(7, 240, 13):
            raw = identical_t_raw(n, k / 1000.0)
            if raw < 0.0 and len(neg) < want and n not in [p[0] for p in neg]:
                neg.append((n, k / 1000.0))
            elif raw > 0.0 and len(pos) < want and n not in [p[0] for p in pos]:
                pos.append((n, k / 1000.0))
    return tuple(neg), tuple(pos)


@functools.lru_cache(maxsize=None)
def case_e_variance():
    """One island per pair of variance_pairs(), two units apart: five coincident own points at (x, 0, 0), normal +z, and n points of
    the other cloud in the plane z = c, in a row of step 1/1024.  The core point's z is 0, so t = c - 0 = c for every member."""
    neg, pos = variance_pairs()
    own, other, kind = [], [], []
    for m, (n, c) in enumerate(neg + pos):
        x = 2.0 * m
        own.append(np.tile([x, 0.0, 0.0], (5, 1)))
        other.append(np.array([[x + j / 1024.0, 0.0, c] for j in range(n)]))
        kind += [(n, c, m < len(neg))] * 5
    own, other = np.ascontiguousarray(np.concatenate(own)), np.ascontiguousarray(np.concatenate(other))
    nrm = np.tile(_axis(2), (len(own), 1))
    return {"own": own, "other": other, "nrm": nrm, "kind": kind, "model": R.m3c2_fp64(own, other, nrm, RP, L, 5)}


# ---- F: radii the index refuses ----
F_CELL = 0.05
F_RP, F_L = 0.06, 0.12
F_TINY = (1e-7, 1e-7)  # R = 1.4e-7: slot 0 (extent 1) would need 7e6 cells per axis
F_SMALL = (3e-4, 4e-4)  # R = 5e-4: slot 0 builds (2000 cells), slot 1 with its far point (extent 3000) would need 6e6


@functools.lru_cache(maxsize=None)
def case_f():
    """slot 0: a random sheet over the unit square; slot 1: another one 1 cm above it and one point 3000 units away"""
    rng = np.random.default_rng(77)

    def sheet(n, z):
        return np.stack([rng.random(n), rng.random(n), z + 0.008 * rng.standard_normal(n)], -1)

    def tilted(n):
        v = np.array([0.0, 0.0, 1.0]) + 0.1 * rng.standard_normal((n, 3))
        return np.ascontiguousarray(v / np.linalg.norm(v, axis=1)[:, None])

    a = np.ascontiguousarray(sheet(1200, 0.0))
    b = np.ascontiguousarray(np.concatenate([sheet(1000, 0.01), [[3000.0, 0.5, 0.0]]]))
    return {"clouds": (a, b), "normals": (tilted(len(a)), tilted(len(b)))}
