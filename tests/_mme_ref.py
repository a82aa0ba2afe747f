"""Brute-force model of me_mme (csrc/me_mme.hip) that is exact about the ACCEPTED SET, and the constructed inputs of
test_mme_ref_cpu.py / test_gpu_mme_edges.py.

The neighbour test is the library's own expression in fp64, `((dx*dx + dy*dy) + dz*dz) < r*r` with d = p - q and no FMA
(_localgeom_ref.d2_lib), over every pair (no tree: nothing approximates a radius).  The covariance is formed two-pass about the
neighbourhood mean in np.longdouble from those offsets, divisor k - 1, cofactor determinant, entropy 0.5 ln(2 pi e det), finite
gate (map_eval.cpp:1692).  The model's own rounding is k 2^-64 relative per covariance entry: nothing next to the project's bound
(rtol 1e-8, atol 1e-10) as long as the neighbourhood is not thin, which `thin_margin` measures and the tests assert.

Every constructor returns the cloud and a dict with the property it was built to have."""
import math

import numpy as np

from _localgeom_ref import d2_lib

_LD = np.longdouble
HAIR = 1.0 + 2.0 ** -20      # cloud_build_index: cell_h = cell_size * (1 + 2^-20)
BAND = 2.0 ** -12            # k_mme3: E = 2^-12 cell_h^2
REFINE_COND = 1.8e-6         # k_mme3 flags det < (tr / 2)^2 * 1.8e-6 cell_h^2 for k_mme_refine
MORTON_BITS = 21
RTOL, ATOL = 1e-8, 1e-10     # the bound of test_mme_parity_*


# ------------------------------------------------------------------------------------------------------------
# the accepted set
# ------------------------------------------------------------------------------------------------------------
def _row_chunks(xyz, r, pairs_per_chunk=1 << 21):
    """(rows, cols, acc[len(rows), len(cols)]) over all rows.  Rows are taken in x order and a chunk's columns are cut to the x
    slab that can hold a neighbour: |dx| > r (1 + 2^-20) gives dx*dx > r*r after rounding too, and the sum of non-negative terms
    is rounded monotonically, so nothing outside the slab passes the test.  Everything inside it is tested pair by pair."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    order = np.argsort(xyz[:, 0], kind="stable")
    xs = xyz[order, 0]
    reach = r * HAIR
    step = max(1, min(1024, pairs_per_chunk // max(n, 1)))
    for c0 in range(0, n, step):
        rows = order[c0:c0 + step]
        lo = np.searchsorted(xs, xs[c0] - reach, "left")
        hi = np.searchsorted(xs, xs[min(c0 + step, n) - 1] + reach, "right")
        cols = order[lo:hi]
        acc = d2_lib(xyz[rows][:, None, :], xyz[cols][None, :, :]) < r * r
        acc &= rows[:, None] != cols[None, :]  # the self pair (coincident duplicates have other indices and stay)
        yield rows, cols, acc


def accepted(xyz, r):
    """bool[n, n]: A[i, j] = point j is a neighbour of point i (strict radius, the self pair removed)."""
    n = len(xyz)
    out = np.zeros((n, n), bool)
    for rows, cols, acc in _row_chunks(xyz, r):
        out[np.ix_(rows, cols)] = acc
    return out


def moments(xyz, r):
    """-> (k[n], cov[n, 3, 3] float64 rounded from longdouble; zeros where k < 2)."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    k = np.zeros(n, np.int64)
    cov = np.zeros((n, 3, 3))
    for rows, cols, acc in _row_chunks(xyz, r):
        kk = acc.sum(1)
        k[rows] = kk
        ri, cj = np.nonzero(acc)  # row-major: the pairs of a row are contiguous
        if len(ri) == 0:
            continue
        d = (xyz[cols[cj]] - xyz[rows[ri]]).astype(_LD)  # p - q, the library's own subtraction
        has = kk > 0
        starts = np.concatenate([[0], np.cumsum(kk)[:-1]])[has]
        kl = kk[has].astype(_LD)
        mean = np.add.reduceat(d, starts, axis=0) / kl[:, None]
        e = d - np.repeat(mean, kk[has], axis=0)
        s = np.zeros((int(has.sum()), 3, 3), _LD)
        for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
            s[:, a, b] = s[:, b, a] = np.add.reduceat(e[:, a] * e[:, b], starts)
        s /= np.maximum(kl - 1, 1)[:, None, None]
        s[kk[has] < 2] = 0
        cov[rows[has]] = s.astype(np.float64)
    return k, cov


def _det(c):
    """Eigen's 3x3 determinant (cofactor expansion along row 0), in longdouble"""
    c = c.astype(_LD)
    return (c[:, 0, 0] * (c[:, 1, 1] * c[:, 2, 2] - c[:, 1, 2] * c[:, 1, 2]) - c[:, 0, 1] * (c[:, 0, 1] * c[:, 2, 2] - c[:, 1, 2] * c[:, 0, 2])
            + c[:, 0, 2] * (c[:, 0, 1] * c[:, 1, 2] - c[:, 1, 1] * c[:, 0, 2]))


def entropy_of(k, cov, min_k):
    """-> (entropy[n], valid[n], n_valid, sum) from moments()"""
    n = len(k)
    ent = np.zeros(n)
    have = k >= max(int(min_k), 2)
    with np.errstate(all="ignore"):
        h = (0.5 * np.log(2.0 * _LD(math.pi) * _LD(math.e) * _det(cov[have]))).astype(np.float64)
    ok = np.isfinite(h)  # (:1692) a non-finite value: ent = 0, valid = 0
    valid = np.zeros(n, bool)
    valid[np.nonzero(have)[0][ok]] = True
    ent[valid] = h[ok]
    return ent, valid, int(valid.sum()), math.fsum(ent[valid])


def mme(xyz, r, min_k):
    """-> (k[n], entropy[n], valid[n], n_valid, sum)"""
    k, cov = moments(xyz, r)
    return (k,) + entropy_of(k, cov, min_k)


def thin_margin(k, cov, cell_h, min_k=2):
    """min over the neighbourhoods with k >= min_k of det / ((tr / 2)^2 * 1.8e-6 cell_h^2): k_mme3 hands a neighbourhood to
    k_mme_refine when this is below 1.  inf when there is no such neighbourhood."""
    have = k >= max(int(min_k), 2)
    if not have.any():
        return math.inf
    c = cov[have]
    tr = (c[:, 0, 0] + c[:, 1, 1]) + c[:, 2, 2]
    with np.errstate(all="ignore"):
        m = _det(c).astype(np.float64) / (0.25 * tr * tr * REFINE_COND * cell_h * cell_h)
    return float(np.nanmin(m))


# ------------------------------------------------------------------------------------------------------------
# the grid of cloud_build_index, restated
# ------------------------------------------------------------------------------------------------------------
def grid(xyz, cell_size):
    """-> (cell_h, origin[3], shift) as cloud_build_index computes them; ValueError where it reports
    "cell size too small for the cloud extent"."""
    lo, hi = xyz.min(0), xyz.max(0)
    cell_h = cell_size * HAIR
    origin = np.floor(lo / cell_h) * cell_h
    extent = float((hi - origin).max())
    ncell = math.floor(extent / cell_h) + 1.0
    bits = 1
    while float(1 << bits) < ncell and bits <= MORTON_BITS:
        bits += 1
    if bits > MORTON_BITS:
        raise ValueError("cell size too small for the cloud extent")
    return cell_h, origin, MORTON_BITS - bits


def cells(xyz, cell_size):
    """integer cell coordinates [n, 3] on that grid"""
    cell_h, origin, _ = grid(xyz, cell_size)
    return np.floor((xyz - origin) / cell_h).astype(np.int64)


def _spread(v):
    out = np.zeros(len(v), np.uint64)
    for b in range(MORTON_BITS):
        out |= ((v.astype(np.uint64) >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton_order(xyz, cell_size):
    """Sorted order of the points along the Z curve of their cells (a stand-in for the index's Hilbert order: both keep a cell
    contiguous and neighbouring cells mostly close)."""
    c = cells(xyz, cell_size)
    code = _spread(c[:, 0]) | (_spread(c[:, 1]) << np.uint64(1)) | (_spread(c[:, 2]) << np.uint64(2))
    return np.argsort(code, kind="stable")


def clusters_per_wave(xyz, cell_size, label):
    """Distinct labels among every 64 consecutive points of morton_order -> array, one entry per wavefront."""
    lab = np.asarray(label)[morton_order(xyz, cell_size)]
    return np.array([len(np.unique(lab[i:i + 64])) for i in range(0, len(lab), 64)])


def band(xyz, r, cell_h):
    """The pairs the exact branch of k_mme3 is for: (i, j, accepted, tie) of every ordered pair i != j whose cells are adjacent (the 27-cell
    stencil of i on the grid of edge cell_h, origin snapped as the index does) and |d^2 - r^2| <= 2^-12 cell_h^2; tie: d^2 == r^2."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    origin = np.floor(xyz.min(0) / cell_h) * cell_h
    c = np.floor((xyz - origin) / cell_h).astype(np.int64)
    reach = math.sqrt(r * r + BAND * cell_h * cell_h) * HAIR
    E = BAND * cell_h * cell_h
    I, J, A, T = [], [], [], []
    for rows, cols, _ in _row_chunks(xyz, reach):
        d2 = d2_lib(xyz[rows][:, None, :], xyz[cols][None, :, :])
        m = np.abs(d2 - r * r) <= E
        m &= rows[:, None] != cols[None, :]
        ri, cj = np.nonzero(m)
        i, j = rows[ri], cols[cj]
        near = np.abs(c[i] - c[j]).max(1) <= 1
        I.append(i[near])
        J.append(j[near])
        A.append(d2[ri, cj][near] < r * r)
        T.append(d2[ri, cj][near] == r * r)
    return np.concatenate(I), np.concatenate(J), np.concatenate(A), np.concatenate(T)


# ------------------------------------------------------------------------------------------------------------
# constructed inputs
# ------------------------------------------------------------------------------------------------------------
LATTICE_S = 0.0625


def lattice(side=13, s=LATTICE_S, offset=(1024.0, -512.0, 64.0), seed=3, margin=3):
    """(a) Dyadic lattice, shuffled, shifted by a dyadic offset: every coordinate and every difference is exact, so d^2 == r^2
    holds exactly for the lattice vectors of that length.  info["interior"]: points at least `margin` steps from every face."""
    g = np.arange(side)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    ijk = ijk[np.random.default_rng(seed).permutation(len(ijk))]
    xyz = ijk * s + np.asarray(offset, np.float64)
    interior = np.all((ijk >= margin) & (ijk <= side - 1 - margin), 1)
    return np.ascontiguousarray(xyz), {"interior": interior, "s": s}


def lattice_counts(r_steps):
    """(inside, on): lattice vectors v != 0 with |v|^2 < r_steps^2, and with |v|^2 == r_steps^2"""
    m = int(r_steps) + 1
    g = np.arange(-m, m + 1)
    v2 = (g[:, None, None] ** 2 + g[None, :, None] ** 2) + g[None, None, :] ** 2
    return int((v2 < r_steps * r_steps).sum()) - 1, int((v2 == r_steps * r_steps).sum())


DELTAS = tuple(sg * 2.0 ** -e for e in (40, 30, 20, 16, 14, 13, 12) for sg in (1.0, -1.0))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _sites(rng, n, pitch, dims=(16, 16, 8)):
    """n distinct sites of a coarse lattice of the given pitch (dyadic multiples: cluster centres carry few mantissa bits)"""
    total = dims[0] * dims[1] * dims[2]
    pick = rng.choice(total, n, replace=False)
    ijk = np.stack(np.unravel_index(pick, dims), -1)
    return ijk * pitch


def probe_clusters(r=0.1, min_k=5, n_clusters=700, seed=11, extra=0):
    """(b) One cluster per site of a lattice of pitch 8 r (points of different clusters are >= 6 r apart): a query at the site,
    min_k - 1 neighbours in general position within 0.4 r of it, and one shell point at distance r (1 + delta) in a random
    direction, delta cycling through DELTAS; a draw whose cluster holds a neighbourhood of >= min_k points within 4x of
    k_mme_refine's threshold is drawn again.  The query has min_k neighbours exactly when its shell point is accepted.
    extra > 0 adds (c)'s second set: that many clusters of 3 - 12 points within 0.4 r of further sites.
    info: "query", "shell" (indices), "delta" per cluster, "label" per point (cluster number)."""
    rng = np.random.default_rng(seed)
    sites = _sites(rng, n_clusters + extra, 8.0 * r)
    pts, lab, qi, si, dl = [], [], [], [], []
    at = 0
    for c in range(n_clusters):
        o = sites[c]
        delta = DELTAS[c % len(DELTAS)]
        while True:  # "general position": no neighbourhood of the cluster within 4x of k_mme_refine's threshold
            inner = o + _unit(rng, min_k - 1) * (rng.uniform(0.1, 0.4, (min_k - 1, 1)) * r)
            shell = o + _unit(rng, 1) * (r * (1.0 + delta))
            if thin_margin(*moments(np.concatenate([o[None], inner, shell]), r), r * HAIR, min_k) > 4.0:
                break
        pts += [o[None], inner, shell]
        qi.append(at)
        si.append(at + min_k)
        dl.append(delta)
        lab += [c] * (min_k + 1)
        at += min_k + 1
    for c in range(n_clusters, n_clusters + extra):
        m = int(rng.integers(3, 13))
        pts.append(sites[c] + _unit(rng, m) * (rng.uniform(0.05, 0.4, (m, 1)) * r))
        lab += [c] * m
        at += m
    xyz = np.ascontiguousarray(np.concatenate(pts))
    perm = rng.permutation(len(xyz))  # index order unrelated to position
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return xyz[perm], {"query": inv[np.array(qi)], "shell": inv[np.array(si)], "delta": np.array(dl), "label": np.array(lab)[perm]}


def blob_between_sparse(r=0.1, n_sparse=300, n_blob=3000, seed=17):
    """(c) Sparse clusters of 3 - 12 points on a 16 x 16 x 8 lattice of pitch 8 r and ONE dense blob (a ball of radius 0.45 r) at a
    site in the middle of it: in the sorted order the blob's run lies between sparse points, so the waves that hold its ends mix a
    long run with many small groups.  info["label"]: cluster number, the blob's is n_sparse."""
    rng = np.random.default_rng(seed)
    sites = _sites(rng, n_sparse, 8.0 * r)
    centre = np.array([7, 8, 3]) * 8.0 * r + np.array([3.0, 3.0, 3.0]) * r  # off the sparse sites, in a cell of its own
    pts, lab = [], []
    for c in range(n_sparse):
        m = int(rng.integers(3, 13))
        pts.append(sites[c] + _unit(rng, m) * (rng.uniform(0.05, 0.4, (m, 1)) * r))
        lab += [c] * m
    pts.append(centre + _unit(rng, n_blob) * (0.45 * r * rng.uniform(0, 1, (n_blob, 1)) ** (1 / 3)))
    lab += [n_sparse] * n_blob
    xyz = np.ascontiguousarray(np.concatenate(pts))
    perm = rng.permutation(len(xyz))
    return xyz[perm], {"label": np.array(lab)[perm], "blob": n_sparse}


def ball(n, r=0.1, seed=23, centre=(2.03, -1.01, 0.52)):
    """(e) n points uniform in ONE ball of radius 0.45 r: every pair is a neighbour pair, k = n - 1 for every point."""
    rng = np.random.default_rng(seed + n)
    xyz = np.asarray(centre) + _unit(rng, n) * (0.45 * r * rng.uniform(0, 1, (n, 1)) ** (1 / 3))
    return np.ascontiguousarray(xyz), {"k": n - 1}


def scattered(n, r=0.1, seed=29):
    """(e) n points uniform over 5 x 5 x 4 = 100 cells"""
    rng = np.random.default_rng(seed + n)
    xyz = rng.uniform(0, 1, (n, 3)) * np.array([5, 5, 4]) * r * HAIR + np.array([-0.2, 0.3, 1.0])
    return np.ascontiguousarray(xyz), {}


def far_blobs(r, shift, n=500, seed=31):
    """(f) Two balls of radius 0.45 r so far apart that cloud_build_index(r) lands on `shift` (0, 1), or — shift = -1 — one notch
    past the largest grid (2^21 cells per axis), where it reports an error.  The separation is the middle of the bits_cell loop's
    bracket for that shift: ncell in (2^(20 - shift), 2^(21 - shift)]."""
    rng = np.random.default_rng(seed)
    span = 1.5 * 2.0 ** (20 - shift) * r * HAIR
    a = np.array([-3.0, 2.0, 1.0]) + _unit(rng, n) * (0.45 * r * rng.uniform(0, 1, (n, 1)) ** (1 / 3))
    b = np.array([-3.0, 2.0, 1.0]) + np.array([1.0, 0.37, -0.61]) * span + _unit(rng, n) * (0.45 * r * rng.uniform(0, 1, (n, 1)) ** (1 / 3))
    xyz = np.concatenate([a, b])
    return np.ascontiguousarray(xyz[rng.permutation(2 * n)]), {"k": n - 1}


def scan_slice(n=10_000, seed=100):
    """(d), (f) The middle n points in x of synth.scan_pair(4 n)'s estimated map: a slab of a campus scan at its full density"""
    from cloud_map_evaluation_amd import synth

    est = synth.scan_pair(4 * n, seed=seed)[0].numpy()
    o = np.argsort(est[:, 0], kind="stable")
    return np.ascontiguousarray(est[o[(len(o) - n) // 2:(len(o) - n) // 2 + n]]), {}


UTM = np.array([5.0e5, 4.5e6, 100.0])


def near_radius_share(xyz, r, rel=2.0 ** -20):
    """bool[n]: points with some pair within rel * r^2 of r^2 (their k may change when the cloud is shifted and re-rounded)"""
    out = np.zeros(len(xyz), bool)
    reach = r * math.sqrt(1.0 + rel) * HAIR
    for rows, cols, _ in _row_chunks(xyz, reach):
        d2 = d2_lib(xyz[rows][:, None, :], xyz[cols][None, :, :])
        out[rows] = (np.abs(d2 - r * r) <= rel * r * r).any(1)
    return out


def rounds_per_wave(xyz, cell_size):
    """Rounds a wavefront of 64 Morton-consecutive points needs when the first pending lane leads and takes every lane whose cell
    is within Chebyshev distance 2 of its own (k_mme3 picks the best of five candidate leaders: it needs this many or fewer).
    -> array, one entry per wavefront."""
    c = cells(xyz, cell_size)[morton_order(xyz, cell_size)]
    out = []
    for i in range(0, len(c), 64):
        w = c[i:i + 64]
        pending = np.ones(len(w), bool)
        n = 0
        while pending.any():
            lead = w[np.argmax(pending)]
            pending &= np.abs(w - lead).max(1) > 2
            n += 1
        out.append(n)
    return np.array(out)


# ------------------------------------------------------------------------------------------------------------
# the named cases both test files run: name -> (xyz, r, min_k, info), built once
# ------------------------------------------------------------------------------------------------------------
_S = LATTICE_S
TIE_UP = 1.0 + 2.0 ** -30  # a radius this much larger takes the exact ties in


def _lattice_case(r, strict):
    xyz, info = lattice()
    steps = round(r / _S)
    inside, on = lattice_counts(steps)
    info = dict(info, k_interior=inside if strict else inside + on, ties_interior=on)
    return xyz, (r if strict else r * TIE_UP), info["k_interior"], info


def _probe_case(min_k, extra):
    xyz, info = probe_clusters(0.1, min_k, 700, seed=11 + min_k, extra=extra)
    return xyz, 0.1, min_k, info


def _with(xyz_info, r, min_k):
    return xyz_info[0], r, min_k, xyz_info[1]


def _shifted(sign):
    xyz, info = scan_slice()
    return np.ascontiguousarray(xyz + sign * UTM), 0.1, 10, dict(info, base="scan")


CASES = {
    "lattice_r2": lambda: _lattice_case(2 * _S, True),
    "lattice_r3": lambda: _lattice_case(3 * _S, True),
    "lattice_r2_ties_in": lambda: _lattice_case(2 * _S, False),
    "lattice_r3_ties_in": lambda: _lattice_case(3 * _S, False),
    "probes_k5": lambda: _probe_case(5, 0),
    "probes_k10": lambda: _probe_case(10, 0),
    "rounds_k5": lambda: _probe_case(5, 600),
    "rounds_k10": lambda: _probe_case(10, 600),
    "blob_between_sparse": lambda: _with(blob_between_sparse(), 0.1, 5),
    "dense_4095": lambda: _with(ball(4095), 0.1, 10),
    "dense_4096": lambda: _with(ball(4096), 0.1, 10),
    "dense_4097": lambda: _with(ball(4097), 0.1, 10),
    "far_shift0": lambda: _with(far_blobs(0.01, 0), 0.01, 10),
    "far_shift1": lambda: _with(far_blobs(0.01, 1), 0.01, 10),
    "scan": lambda: _with(scan_slice(), 0.1, 10),
    "scan_utm": lambda: _shifted(1.0),
    "scan_utm_neg": lambda: _shifted(-1.0),
}
SIZES_MIN_K = 5
SIZES = (1, 2, 3, SIZES_MIN_K, SIZES_MIN_K + 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
for _n in SIZES:
    CASES[f"ball_{_n}"] = lambda n=_n: _with(ball(n), 0.1, SIZES_MIN_K)
    CASES[f"scattered_{_n}"] = lambda n=_n: _with(scattered(n), 0.1, SIZES_MIN_K)

# (d) index reuse: the clouds, their min_k and, per uploaded cell size c, the radii mme_run is asked for.  It rebuilds when
# cell_h > 1.5 want_h or cell_h < want_h (both carry the same 1 + 2^-20): the first four radii lie inside the window, the last outside.
REUSE_MIN_K = {"lattice_r2": 5, "scan": 10}
REUSE_CELLS = (0.1, 0.15)


def reuse_radii(c):
    return (c, 0.9 * c, 0.75 * c, c / 1.5 * (1.0 + 2.0 ** -10), c / 1.5 * (1.0 - 2.0 ** -10))


_cache = {}


def case(name):
    """-> (xyz, r, min_k, info) of a named case (built once per process; treat as read-only)"""
    if name not in _cache:
        xyz, r, min_k, info = CASES[name]()
        xyz.setflags(write=False)
        _cache[name] = (xyz, r, min_k, info)
    return _cache[name]


_mom = {}


def case_moments(name, r=None):
    """moments() of a named case at its own radius (or at r), computed once per process"""
    xyz, r0, _, _ = case(name)
    r = r0 if r is None else r
    if (name, r) not in _mom:
        _mom[(name, r)] = moments(xyz, r)
    return _mom[(name, r)]
