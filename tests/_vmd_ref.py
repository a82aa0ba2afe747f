"""The exact model of the voxel half of the suite (W2 of two voxel Gaussians, the est x gt join, AWD, SCS), restated from
include/mapeval_hip.h and DESIGN.md 4.4 in mpmath at 50 digits, the inputs shared by test_vmd_ref_cpu.py and the three
test_gpu_*_edges.py files that use it, the tolerances (each with the figure it comes from), and float64 restatements that take a
deliberate mistake (`mutant=`) so that the CPU test can show that every input family has teeth.

W.  D = W^2 = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr chol(L1 S2 L1^T), S_i = regularize(stored_i, n_i), L1 = chol(S1) (lower, unchecked:
the square root of a negative pivot is NaN, and W = sqrt(max(0, D)) with max(0, NaN) = 0, as std::max(0.0, NaN)).  The scale of the
cancellation is S = |mu1 - mu2|^2 + tr S1 + tr S2 + 2 tr chol(.), and a device value is judged by e = |W_dev^2 - D| / S in units of
u = 2^-53.  The tolerance of a family is max(64, 8 x the error of the project's own oracle.w2_gaussian on the SAME inputs) u: W2_TOL below,
measured on the CPU by test_vmd_ref_cpu.py (which fails if the oracle exceeds the figure written here), never against a device.

SCS.  Bound on |scs_dev - scs_model|, scs_bound(): (N_stencil + M / 256 + 16) u (1 + max_i scs_i), where
  * d = min(N - 1, ceil((2 r + 1)^3 / 64) + 6) is the depth of the device's sum over the N (the largest neighbour count of the table)
    neighbours of a voxel: each lane adds the stencil cells o = lane, lane + 64, ..., then a 6-level butterfly; W >= 0, so either sum
    (of w, of (w - mean)^2) is off by at most d u of itself;
  * the mean m' = m (1 + dm), |dm| <= (d + 1) u (the sum and one division);
  * sum (w - m')^2 = sum (w - m)^2 + n (m' - m)^2 exactly (the cross term vanishes), so the mean's error enters the variance only as
    its square: sqrt(v + dm^2 m^2) / m - sqrt(v) / m <= |dm|, an ABSOLUTE (d + 1) u on scs_i (all of the error when v = 0);
  * each term (w - m')^2 carries 3 u (a subtraction, a product), the sum d u, the division by n one u: (d + 4) u on the variance,
    half of it after the square root, plus 1 u for the root and 1 u + |dm| for the division by the mean:
    relative (d + 4) / 2 + 2 + (d + 1) = 1.5 d + 5;
  * so |d scs_i| <= (1.5 d + 5) u (1 + scs_i) and N_stencil = 1.5 d;
  * k_sum_masked adds the M values (>= 0) 256 apart per thread, then an 8-level tree, then one division: (M / 256 + 1 + 8 + 1) u;
  * 5 + 10 = 15, and 16 leaves one u for the second-order terms.
test_vmd_ref_cpu.py checks that a float64 restatement whose summation order is permuted at random 20 times stays within a quarter of it.

mu of a voxel: the device forms centre + (sum of offsets) / n; the offsets are below the voxel size vs, any order of n of them is off by
at most (n - 1) u vs after the division, the two roundings of the result cost 2 u |mu|: mu_bound() = (n + 8) u max(|mu|, vs).
"""
import functools
import math

import mpmath as mp
import numpy as np

from _tol import assert_sigma_close

mp.mp.dps = 50
U = 2.0 ** -53
CLAMP = mp.mpf(1e-6)  # the double nearest to 1e-6, as the kernel's literal
NAN = float("nan")

# family -> (largest e / u of oracle.w2_gaussian against this model on the family's inputs, as measured on the CPU and rounded up,
#            the tolerance max(64, 8 x that) in u)
W2_TOL = {
    "generic": (15.0, 120.0),
    "planar": (61000.0, 488000.0),
    "line": (5700.0, 45600.0),
    "straddle": (710.0, 5680.0),
    "clamped": (14.0, 112.0),
    "repeated": (6.0, 64.0),
    "diagonal": (4.0, 64.0),
    "asymmetric": (6.0, 64.0),
    "identical": (7200.0, 57600.0),
    "far": (29.0, 232.0),
    "small_n": (5.0, 64.0),
    "voxels": (4800.0, 38400.0),
}


def w2_tol(family):
    measured, tol = W2_TOL[family]
    assert tol == max(64.0, 8.0 * measured)
    return tol * U


# ------------------------------------------------------------------------------------------------------------------------------
# the model
def _mat(a):
    a = np.asarray(a, dtype=np.float64).reshape(3, 3)
    return mp.matrix([[mp.mpf(float(a[r, c])) for c in range(3)] for r in range(3)])


def stored_sigma(points):
    """-> (mu [3 mpf], sigma as stored (3x3 mp.matrix), n): M2 = sum (p - mu)(p - mu)^T, raw for n <= 10, M2 / (n - 1)^2 above."""
    p = [[mp.mpf(float(x)) for x in row] for row in np.asarray(points, dtype=np.float64).reshape(-1, 3)]
    n = len(p)
    mu = [mp.fsum(q[d] for q in p) / n for d in range(3)]
    m2 = mp.matrix(3, 3)
    for r in range(3):
        for c in range(3):
            m2[r, c] = mp.fsum((q[r] - mu[r]) * (q[c] - mu[c]) for q in p)
    if n > 10:
        m2 = m2 / ((n - 1) * (n - 1))
    return mu, m2, n


def regularize(sigma_stored, n):
    """identity for n <= 1; else / (n - 1), (A + A^T) / 2, eigenvalues max(., 1e-6), rebuilt."""
    if n <= 1:
        return mp.eye(3)
    a = (sigma_stored if isinstance(sigma_stored, mp.matrix) else _mat(sigma_stored)) / (n - 1)
    a = (a + a.T) / 2
    ev, q = mp.eigsy(a)
    return q * mp.diag([max(e, CLAMP) for e in ev]) * q.T


def _chol_trace(a):
    """tr of the unchecked lower Cholesky factor and the factor, or (None, None) where IEEE arithmetic gives NaN: a negative pivot,
    or a zero first or second pivot (x / 0 is inf or NaN, and the pivot after it sqrt(. - inf) or sqrt(NaN))."""
    if a[0, 0] <= 0:
        return None, None
    l00 = mp.sqrt(a[0, 0])
    l10, l20 = a[1, 0] / l00, a[2, 0] / l00
    p1 = a[1, 1] - l10 * l10
    if p1 <= 0:
        return None, None
    l11 = mp.sqrt(p1)
    l21 = (a[2, 1] - l20 * l10) / l11
    p2 = a[2, 2] - l20 * l20 - l21 * l21
    if p2 < 0:
        return None, None
    l22 = mp.sqrt(p2)
    return l00 + l11 + l22, mp.matrix([[l00, 0, 0], [l10, l11, 0], [l20, l21, l22]])


def w2_squared(mu1, s1, n1, mu2, s2, n2):
    """-> (D, S, W): D and S mpf (NaN floats where IEEE gives NaN), W a float = sqrt(max(0, D)), NaN -> 0."""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64).reshape(3), np.asarray(mu2, dtype=np.float64).reshape(3)
    used = [mu1, mu2] + ([np.asarray(s1, dtype=np.float64)] if n1 > 1 else []) + ([np.asarray(s2, dtype=np.float64)] if n2 > 1 else [])
    if not all(np.isfinite(x).all() for x in used):
        assert not any(np.isinf(x).any() for x in used), "the model does not define infinite inputs"
        return NAN, NAN, 0.0
    a, b = regularize(_mat(s1), n1), regularize(_mat(s2), n2)
    md = mp.fsum((mp.mpf(float(mu1[d])) - mp.mpf(float(mu2[d]))) ** 2 for d in range(3))
    tr = a[0, 0] + a[1, 1] + a[2, 2] + b[0, 0] + b[1, 1] + b[2, 2]
    _, l1 = _chol_trace(a)
    t = None if l1 is None else _chol_trace(l1 * b * l1.T)[0]
    if t is None:
        return NAN, NAN, 0.0
    d, s = md + tr - 2 * t, md + tr + 2 * t
    return d, s, float(mp.sqrt(d)) if d > 0 else 0.0


def w2_error_units(w_dev, d, s):
    """e / u of a device (or oracle) W against the model's (D, S)."""
    w = mp.mpf(float(w_dev))
    return float(abs(w * w - d) / s / U)


def neighbours(keys, radius):
    """[M, M] bool: j is a neighbour of i = inside the Chebyshev cube of that radius round i, centre excluded."""
    k = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    cheb = np.abs(k[:, None, :] - k[None, :, :]).max(axis=2)
    return (cheb <= radius) & ~np.eye(len(k), dtype=bool)


def scs(keys, w, radius):
    """-> (scs, per-voxel values [M] (NaN where a voxel has no neighbour), the largest neighbour count).  map_eval.cpp:347-389 as the
    header cites it: per voxel with neighbours, population std / mean of the neighbours' W; the mean of those, NaN if there are none;
    0 / 0 = NaN and x / 0 = inf propagate."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    nb = neighbours(keys, radius) if len(w) else np.zeros((0, 0), bool)
    per, vals = np.full(len(w), NAN), []
    for i in range(len(w)):
        idx = np.flatnonzero(nb[i])
        if len(idx) == 0:
            continue
        ws = [mp.mpf(float(w[j])) for j in idx]
        mean = mp.fsum(ws) / len(ws)
        var = mp.fsum((x - mean) ** 2 for x in ws) / len(ws)
        v = (mp.nan if var == 0 else mp.inf) if mean == 0 else mp.sqrt(var) / mean
        vals.append(v)
        per[i] = float(v)
    n_max = int(nb.sum(axis=1).max()) if len(w) else 0
    if not vals:
        return NAN, per, n_max
    if any(mp.isnan(v) for v in vals):
        return NAN, per, n_max
    return float(mp.fsum(vals) / len(vals)), per, n_max


def scs_bound(n_max, m, radius, per):
    """The derivation is in the module's docstring."""
    depth = min(max(n_max - 1, 0), math.ceil((2 * radius + 1) ** 3 / 64) + 6)
    fin = per[np.isfinite(per)]
    return (1.5 * depth + m / 256 + 16) * U * (1.0 + (float(fin.max()) if len(fin) else 0.0))


def _lex(keys):
    k = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    return np.lexsort((k[:, 2], k[:, 1], k[:, 0]))


def join(ekeys, en, gkeys, gn, min_pts):
    """-> ([(est row, gt row)] in ascending est-key order, (active, old, new)): active = est voxels whose key the ground truth has,
    old = ground-truth voxels without an est voxel, new = est voxels without one; matched = active and both populations >= min_pts."""
    g_at = {tuple(int(x) for x in k): j for j, k in enumerate(np.asarray(gkeys).reshape(-1, 3))}
    ek = np.asarray(ekeys).reshape(-1, 3)
    pairs, active = [], 0
    for i in _lex(ek):
        j = g_at.get(tuple(int(x) for x in ek[i]))
        if j is None:
            continue
        active += 1
        if en[i] >= min_pts and gn[j] >= min_pts:
            pairs.append((int(i), j))
    return pairs, (active, len(g_at) - active, len(ek) - active)


def voxels(points, vs):
    """-> keys [V, 3] ascending, [(mu, sigma stored, n)] per voxel: the lattice floor(p / vs) (IEEE division, as getVoxelIndex)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    k = np.floor(p / vs).astype(np.int64)
    uk, inv = np.unique(k, axis=0, return_inverse=True)
    inv = inv.ravel()
    return uk, [stored_sigma(p[inv == v]) for v in range(len(uk))]


def _f(m):
    return np.array([[float(m[r, c]) for c in range(3)] for r in range(3)])


def awd_scs(est_points, gt_points, vs, min_pts, radius):
    """-> dict(rows [M, 27], w_sorted, awd, scs, counts, n_rows, per (the SCS per-voxel values), n_max)."""
    ek, ev = voxels(est_points, vs)
    gk, gv = voxels(gt_points, vs)
    pairs, counts = join(ek, [v[2] for v in ev], gk, [v[2] for v in gv], min_pts)
    rows = np.zeros((len(pairs), 27))
    for m, (i, j) in enumerate(pairs):
        (emu, es, en), (gmu, gs, gn) = ev[i], gv[j]
        es_f, gs_f = _f(es), _f(gs)
        key = ek[i].astype(np.float64)
        rows[m, 0:3], rows[m, 3:6] = key * vs, (key + 1.0) * vs
        rows[m, 6:9] = [float(x) for x in emu]
        # W of the Gaussians as a double holds them (what any implementation is handed), ground truth first
        rows[m, 9] = w2_squared([float(x) for x in gmu], gs_f, gn, [float(x) for x in emu], es_f, en)[2]
        rows[m, 10], rows[m, 11] = gn, en
        rows[m, 12:18] = es_f[np.triu_indices(3)]
        rows[m, 18:21] = [float(x) for x in gmu]
        rows[m, 21:27] = gs_f[np.triu_indices(3)]
    w = rows[:, 9]
    keys = ek[[i for i, _ in pairs]] if pairs else np.zeros((0, 3), np.int64)
    s, per, n_max = scs(keys, w, radius)
    awd = float(mp.fsum(mp.mpf(float(x)) for x in w) / len(w)) if len(w) else NAN
    return dict(rows=rows, w_sorted=np.sort(w), awd=awd, scs=s, counts=counts, n_rows=len(pairs), per=per, n_max=n_max, keys=keys)


def mu_bound(n, mu, vs):
    return (np.asarray(n, dtype=np.float64) + 8.0) * U * np.maximum(np.abs(mu).max(axis=-1), vs)


def full9(r6):
    """[k, 6] upper triangles (the rows' sigma columns) -> [k, 9]."""
    r6 = np.asarray(r6, dtype=np.float64).reshape(-1, 6)
    return r6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]


# ------------------------------------------------------------------------------------------------------------------------------
# float64 restatements that take a deliberate mistake
def stored_sigma_f64(points, mutant=None):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    mu = p.mean(axis=0)
    m2 = (p - mu).T @ (p - mu)
    if n > 10 or (mutant == "no_quirk" and n > 1):
        m2 = m2 / (n - 1) / (n - 1)
    return mu, m2, n


def _chol_f64(a, upper=False):
    with np.errstate(all="ignore"):
        if upper:  # a = R^T R with R upper = the lower factor of the matrix reversed in both axes, reversed back
            return _chol_f64(a[::-1, ::-1])[::-1, ::-1]
        l = np.zeros((3, 3))
        l[0, 0] = np.sqrt(a[0, 0])
        l[1, 0], l[2, 0] = a[1, 0] / l[0, 0], a[2, 0] / l[0, 0]
        l[1, 1] = np.sqrt(a[1, 1] - l[1, 0] * l[1, 0])
        l[2, 1] = (a[2, 1] - l[2, 0] * l[1, 0]) / l[1, 1]
        l[2, 2] = np.sqrt(a[2, 2] - l[2, 0] * l[2, 0] - l[2, 1] * l[2, 1])
        return l


def _regularize_f64(s, n, mutant):
    if n <= 1:
        return np.zeros((3, 3)) if mutant == "zeros_for_n1" else np.eye(3)
    s = np.asarray(s, dtype=np.float64).reshape(3, 3)
    div = {"div_n": float(n), "no_third_division": 1.0, "clamp_before_division": 1.0}.get(mutant, float(n - 1))
    a = s / div
    a = np.tril(a) + np.tril(a, -1).T if mutant == "no_symmetrisation" else (a + a.T) / 2  # (a self-adjoint solver reads one triangle)
    if not np.isfinite(a).all():
        return np.full((3, 3), np.nan)  # (numpy's solver raises; IEEE arithmetic carries the NaN through to D)
    ev, q = np.linalg.eigh(a)
    if mutant == "clamp_before_division":
        ev = np.maximum(ev, 1e-6) / (n - 1)
    elif mutant != "no_clamp":
        ev = np.maximum(ev, 1e-6)
    return (q * ev) @ q.T


def w2_f64(mu1, s1, n1, mu2, s2, n2, mutant=None):
    """W in float64, with one of W2_MUTANTS applied."""
    if mutant == "swapped":
        mu1, s1, n1, mu2, s2, n2 = mu2, s2, n2, mu1, s1, n1
    with np.errstate(all="ignore"):
        a, b = _regularize_f64(s1, n1, mutant), _regularize_f64(s2, n2, mutant)
        dm = np.asarray(mu1, dtype=np.float64) - np.asarray(mu2, dtype=np.float64)
        if mutant == "upper_cholesky":
            r = _chol_f64(a, upper=True)
            t = np.trace(_chol_f64(r @ b @ r.T, upper=True))
        elif mutant == "matrix_sqrt":
            l1 = _chol_f64(a)
            m = l1 @ b @ l1.T
            t = np.sqrt(np.maximum(np.linalg.eigvalsh((m + m.T) / 2), 0.0)).sum()
        else:
            l1 = _chol_f64(a)
            t = np.trace(_chol_f64(l1 @ b @ l1.T))
        d = dm @ dm + np.trace(a) + np.trace(b) - 2 * t
        return float(np.sqrt(d)) if d > 0 else 0.0  # max(0, NaN) = 0


W2_MUTANTS = ("swapped", "div_n", "no_third_division", "no_quirk", "no_symmetrisation", "no_clamp", "clamp_before_division",
              "zeros_for_n1", "matrix_sqrt", "upper_cholesky")
SCS_MUTANTS = ("centre_included", "sample_variance", "euclidean_ball", "radius_plus_1", "radius_minus_1", "neighbourless_as_zero",
               "ratio_of_means")
JOIN_MUTANTS = ("gt_instead_of_ge", "est_gate_only", "gt_gate_only")


def scs_f64(keys, w, radius, mutant=None, rng=None):
    """SCS in float64, sequential sums; rng: every sum in a random order."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    k = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    if len(w) == 0:
        return NAN
    r = radius + {"radius_plus_1": 1, "radius_minus_1": -1}.get(mutant, 0)
    d = k[:, None, :] - k[None, :, :]
    nb = (d * d).sum(axis=2) <= r * r if mutant == "euclidean_ball" else np.abs(d).max(axis=2) <= r
    if mutant != "centre_included":
        nb &= ~np.eye(len(k), dtype=bool)

    def total(x):
        x = np.asarray(x, dtype=np.float64)
        if rng is not None:
            x = x[rng.permutation(len(x))]
        s = 0.0
        for v in x:
            s += v
        return s

    vals, stds, means = [], [], []
    with np.errstate(all="ignore"):
        for i in range(len(w)):
            ws = w[nb[i]]
            if len(ws) == 0:
                if mutant == "neighbourless_as_zero":
                    vals.append(0.0)
                continue
            mean = total(ws) / len(ws)
            var = np.float64(total((ws - mean) * (ws - mean))) / np.float64(len(ws) - 1 if mutant == "sample_variance" else len(ws))
            stds.append(np.sqrt(var))
            means.append(mean)
            vals.append(np.sqrt(var) / np.float64(mean))
        if mutant == "ratio_of_means":
            return float(np.float64(total(stds)) / np.float64(total(means))) if stds else NAN
        return float(np.float64(total(vals)) / np.float64(len(vals))) if vals else NAN


def join_f64(ekeys, en, gkeys, gn, min_pts, mutant=None):
    g_at = {tuple(int(x) for x in k): j for j, k in enumerate(np.asarray(gkeys).reshape(-1, 3))}
    ek = np.asarray(ekeys).reshape(-1, 3)
    ok = (lambda a: a > min_pts) if mutant == "gt_instead_of_ge" else (lambda a: a >= min_pts)
    pairs = []
    for i in _lex(ek):
        j = g_at.get(tuple(int(x) for x in ek[i]))
        if j is not None and (mutant == "gt_gate_only" or ok(en[i])) and (mutant == "est_gate_only" or ok(gn[j])):
            pairs.append((int(i), j))
    return pairs


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs of the W tests: family -> dict(mu1 [k, 3], s1 [k, 9], n1 [k], mu2, s2, n2)
def _rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _spd(rng, ev, rot=True):
    q = _rot(rng) if rot else np.eye(3)
    return (q * np.asarray(ev, dtype=np.float64)) @ q.T


class _Fam:
    def __init__(self):
        self.c = []

    def add(self, mu1, cov1, n1, mu2, cov2, n2, raw=False):
        """cov: the matrix regularize() is to see after its division; raw: s is handed over as it is"""
        f1, f2 = (1.0, 1.0) if raw else (max(n1 - 1, 1), max(n2 - 1, 1))
        self.c.append((np.asarray(mu1, float), np.asarray(cov1, float).reshape(9) * f1, int(n1), np.asarray(mu2, float),
                       np.asarray(cov2, float).reshape(9) * f2, int(n2)))

    def done(self):
        return dict(mu1=np.array([c[0] for c in self.c]), s1=np.array([c[1] for c in self.c]), n1=np.array([c[2] for c in self.c], np.int32),
                    mu2=np.array([c[3] for c in self.c]), s2=np.array([c[4] for c in self.c]), n2=np.array([c[5] for c in self.c], np.int32))


@functools.lru_cache(maxsize=None)
def w2_families():
    rng = np.random.default_rng(20240611)
    out = {}

    def ev_generic():
        return 10.0 ** rng.uniform(-3, 0, 3)

    def n_generic():
        return int(rng.integers(100, 5001))

    def mu():
        return rng.uniform(-1, 1, 3)

    f = _Fam()
    for _ in range(40):
        f.add(mu(), _spd(rng, ev_generic()), n_generic(), mu(), _spd(rng, ev_generic()), n_generic())
    out["generic"] = f.done()

    f = _Fam()
    for _ in range(40):  # one eigenvalue below the clamp, on either side or on both
        a = _spd(rng, [*ev_generic()[:2], 10.0 ** rng.uniform(-12, -7)])
        b = _spd(rng, [*ev_generic()[:2], 10.0 ** rng.uniform(-12, -7)])
        g = _spd(rng, ev_generic())
        pick = [(a, b), (a, g), (g, b)][_ % 3]
        f.add(mu(), pick[0], n_generic(), mu(), pick[1], n_generic())
    out["planar"] = f.done()

    f = _Fam()
    for _ in range(40):  # two eigenvalues below the clamp; every third case has an exactly rank-1 matrix
        lo = [0.0, 0.0] if _ % 3 == 0 else list(10.0 ** rng.uniform(-12, -7, 2))
        a = _spd(rng, [ev_generic()[0], *lo])
        b = _spd(rng, [ev_generic()[0], *list(10.0 ** rng.uniform(-12, -7, 2))])
        f.add(mu(), a, n_generic(), mu(), b if _ % 2 else _spd(rng, ev_generic()), n_generic())
    out["line"] = f.done()

    f = _Fam()
    for k in range(10, 51):  # an eigenvalue at (1e-6)(1 +- 2^-k): already diagonal for odd k, rotated for even k
        for sign in (1.0, -1.0):
            a = _spd(rng, [0.3, 0.01, 1e-6 * (1.0 + sign * 2.0 ** -k)], rot=k % 2 == 0)
            f.add(mu(), a, n_generic(), mu(), _spd(rng, ev_generic()), n_generic())
    out["straddle"] = f.done()

    f = _Fam()
    z = np.zeros((3, 3))
    for _ in range(40):  # all three eigenvalues clamped: zero and tiny matrices
        tiny = _spd(rng, 10.0 ** rng.uniform(-14, -7, 3))
        a, b = [(z, z), (z, tiny), (tiny, z), (tiny, _spd(rng, ev_generic())), (z, _spd(rng, ev_generic()))][_ % 5]
        f.add(mu() * (_ % 2), a, n_generic(), mu() * (_ % 2), b, n_generic())
    out["clamped"] = f.done()

    f = _Fam()
    for _ in range(42):  # repeated eigenvalues: isotropic, isotropic plus one off-diagonal entry, two equal under a rotation
        c = float(10.0 ** rng.uniform(-3, 0))
        iso = c * np.eye(3)
        off = iso.copy()
        off[0, 1] = off[1, 0] = c * 10.0 ** rng.uniform(-12, -1)
        two = _spd(rng, [c, c, float(10.0 ** rng.uniform(-3, 0))])
        a = [iso, off, two][_ % 3]
        f.add(mu(), a, n_generic(), mu(), [_spd(rng, ev_generic()), iso, two][(_ // 3) % 3], n_generic())
    out["repeated"] = f.done()

    f = _Fam()
    for _ in range(40):  # already diagonal: ascending, descending, any order; every fourth pair diagonal on both sides
        e = np.sort(ev_generic())
        a = np.diag([e, e[::-1], rng.permutation(e), e[::-1]][_ % 4])
        b = np.diag(np.sort(ev_generic())[::-1]) if _ % 4 == 3 else _spd(rng, ev_generic())
        f.add(mu(), a, n_generic(), mu(), b, n_generic())
    out["diagonal"] = f.done()

    f = _Fam()
    for _ in range(40):  # the stored matrix is not symmetric: its symmetric part is what counts
        a, b = _spd(rng, ev_generic()), _spd(rng, ev_generic())
        k = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, 0)
        f.add(mu(), a + (k - k.T), n_generic(), mu(), b + (k - k.T).T * (_ % 2), n_generic())
    out["asymmetric"] = f.done()

    f = _Fam()
    for _ in range(40):  # the same Gaussian on both sides: D = 0 by cancellation
        a = [_spd(rng, ev_generic()), _spd(rng, [*ev_generic()[:2], 1e-9]), z, _spd(rng, ev_generic() * 1e3)][_ % 4]
        n, m = n_generic(), mu() * 10.0 ** rng.uniform(0, 5)
        f.add(m, a, n, m, a, n)
    out["identical"] = f.done()

    f = _Fam()
    for _ in range(40):  # |mu1 - mu2| = 1e4, and survey coordinates of 4e5 a voxel apart
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        m = mu() if _ % 2 == 0 else np.array([4.0e5, -4.0e5, 4.0e5]) + mu()
        m2 = m + d * 1e4 if _ % 2 == 0 else m + mu() * 0.5
        f.add(m, _spd(rng, ev_generic()), n_generic(), m2, _spd(rng, ev_generic()), n_generic())
    out["far"] = f.done()

    f = _Fam()
    for n1 in (0, 1, 2, 10, 11, 12):  # the identity branch (n <= 1) and the first divisors, crossed; the matrix is handed over as it is
        for n2 in (0, 1, 2, 10, 11, 12):
            f.add(mu(), _spd(rng, ev_generic()), n1, mu(), _spd(rng, ev_generic()), n2, raw=True)
    out["small_n"] = f.done()
    return out


@functools.lru_cache(maxsize=None)
def w2_model(family):
    """-> (D [k] mpf or NaN, S [k], W [k] float array) of the family, computed once."""
    f = w2_families()[family] if family != "voxels" else voxel_family()
    res = [w2_squared(f["mu1"][i], f["s1"][i], int(f["n1"][i]), f["mu2"][i], f["s2"][i], int(f["n2"][i])) for i in range(len(f["n1"]))]
    return [r[0] for r in res], [r[1] for r in res], np.array([r[2] for r in res])


def w2_all():
    """Every family one after the other: (arrays, [(family, index in the family)])."""
    fam = w2_families()
    cat = {k: np.concatenate([fam[n][k] for n in fam]) for k in ("mu1", "s1", "n1", "mu2", "s2", "n2")}
    return cat, [(n, i) for n in fam for i in range(len(fam[n]["n1"]))]


def w2_batch(count):
    """A batch of `count` elements: element j is element j mod K of w2_all()."""
    cat, tags = w2_all()
    at = np.arange(count) % len(tags)
    return {k: np.ascontiguousarray(v[at]) for k, v in cat.items()}, [tags[j] for j in at]


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs of the SCS tests: name -> (keys [M, 3] int32, w [M])
@functools.lru_cache(maxsize=None)
def scs_tables():
    rng = np.random.default_rng(77)
    t = {}
    g = np.arange(-2, 3)
    t["dense5"] = np.array([(x, y, z) for x in g for y in g for z in g], np.int32)
    g = np.arange(-4, 5)
    t["slab9"] = np.array([(x, y, -7) for x in g for y in g], np.int32)
    cells = rng.choice(30 ** 3, 700, replace=False)
    t["sparse700"] = (np.stack([cells // 900, (cells // 30) % 30, cells % 30], axis=1) - 15).astype(np.int32)
    out = {}
    for name, keys in t.items():
        keys = keys[rng.permutation(len(keys))]
        out[name] = (keys, rng.uniform(0.05, 1.0, len(keys)))
    for m in (1, 2, 32, 33, 255, 256, 257):  # hash sizes 64 and 128 on either side of 32, the block edge of the final sum
        cells = rng.choice(8 ** 3, m, replace=False)
        keys = (np.stack([cells // 64, (cells // 8) % 8, cells % 8], axis=1) - 4).astype(np.int32)
        out[f"size{m}"] = (keys, rng.uniform(0.05, 1.0, m))
    return out


@functools.lru_cache(maxsize=None)
def scs_model(name, radius):
    keys, w = scs_tables()[name]
    return scs(keys, w, radius)


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs of the AWD / join tests: clouds built voxel by voxel
def cloud(cells, vs, rng):
    """cells: [((ix, iy, iz), n)] -> n points uniform in the interior of each cell (5 % off its faces), in a random order."""
    pts = [(np.asarray(k, dtype=np.float64) + 0.05 + 0.9 * rng.random((n, 3))) * vs for k, n in cells if n > 0]
    p = np.concatenate(pts) if pts else np.zeros((0, 3))
    assert all((np.floor(q / vs) == np.asarray(k)).all() for q, (k, n) in zip(pts, [c for c in cells if c[1] > 0]))
    return p[rng.permutation(len(p))]


@functools.lru_cache(maxsize=None)
def awd_cases():
    """name -> (est points, gt points, vs, min_pts, radius)"""
    rng = np.random.default_rng(5150)
    out = {}
    for vs in (1.0, 0.37):
        tag = f"vs{vs}"
        # populations at the gate, (est, gt) per cell; negative cells included; the cells are neighbours at radius 2
        gate = [(99, 100), (100, 99), (100, 100), (99, 99), (101, 250)]
        cells = [(-2, 0, 1), (-1, 0, 1), (0, 0, 1), (0, -1, 1), (1, -1, 0)]
        out[f"gate_{tag}"] = (cloud([(c, e) for c, (e, g) in zip(cells, gate)], vs, rng),
                              cloud([(c, g) for c, (e, g) in zip(cells, gate)], vs, rng), vs, 100, 2)
        # small gates: every (n_est, n_gt) of {1, 2, 3, 10, 11, 12}^2, one cell each on a 6 x 6 sheet that spans negative indices
        ns = (1, 2, 3, 10, 11, 12)
        ce = [((a - 3, b - 3, -1), ns[a]) for a in range(6) for b in range(6)]
        cg = [((a - 3, b - 3, -1), ns[b]) for a in range(6) for b in range(6)]
        pe, pg = cloud(ce, vs, rng), cloud(cg, vs, rng)
        out[f"small_min2_{tag}"] = (pe, pg, vs, 2, 1)
        out[f"small_min1_{tag}"] = (pe, pg, vs, 1, 2)
    vs = 1.0
    # est-only and gt-only voxels, an est voxel above every gt key and one below every gt key
    e = [((0, 0, 0), 120), ((1, 0, 0), 130), ((5, 5, 5), 110), ((-9, 0, 0), 140), ((9, 9, 9), 105), ((2, 0, 0), 50)]
    g = [((0, 0, 0), 100), ((1, 0, 0), 160), ((2, 0, 0), 170), ((-3, 1, 1), 200), ((3, -1, 2), 111)]
    out["only_and_extreme"] = (cloud(e, vs, rng), cloud(g, vs, rng), vs, 100, 5)
    # one ground-truth voxel; est keys below it, at it and above it
    out["vg1"] = (cloud([((-1, 2, 2), 100), ((0, 2, 2), 101), ((1, 2, 2), 102)], vs, rng), cloud([((0, 2, 2), 100)], vs, rng), vs, 100, 1)
    # 257 est voxels (more than one block of the join) of which 3 match
    e = [((x - 128, 0, 0), 100 if x in (0, 128, 256) else 3) for x in range(257)]
    g = [((-128, 0, 0), 100), ((0, 0, 0), 150), ((128, 0, 0), 100), ((-5, 0, 0), 99), ((300, 1, 1), 100)]
    out["est257"] = (cloud(e, vs, rng), cloud(g, vs, rng), vs, 100, 10)
    out["m0"] = (cloud([((0, 0, 0), 100), ((1, 0, 0), 99)], vs, rng), cloud([((1, 0, 0), 100), ((2, 0, 0), 100)], vs, rng), vs, 100, 5)
    out["m1"] = (cloud([((0, 0, 0), 100), ((1, 0, 0), 99)], vs, rng), cloud([((0, 0, 0), 100), ((1, 0, 0), 100)], vs, rng), vs, 100, 5)
    out["m2_adjacent"] = (cloud([((0, 0, 0), 100), ((1, 0, 0), 100)], vs, rng), cloud([((0, 0, 0), 100), ((1, 0, 0), 100)], vs, rng),
                          vs, 100, 1)
    return out


@functools.lru_cache(maxsize=None)
def awd_model(name):
    return awd_scs(*awd_cases()[name])


@functools.lru_cache(maxsize=None)
def voxel_family():
    """The W inputs of every AWD case's rows (the model's Gaussians rounded to double), ground truth first: the family 'voxels'."""
    rows = np.concatenate([awd_model(n)["rows"] for n in awd_cases()])
    return dict(mu1=rows[:, 18:21].copy(), s1=full9(rows[:, 21:27]), n1=rows[:, 10].astype(np.int32),
                mu2=rows[:, 6:9].copy(), s2=full9(rows[:, 12:18]), n2=rows[:, 11].astype(np.int32))


def check_awd(got, m, vs, radius):
    """A result dict (rows, w_sorted, awd, scs, counts) against the model's: what test_gpu_awd_join_edges.py asserts of the device."""
    rows = got["rows"]
    assert tuple(got["counts"]) == tuple(m["counts"]) and len(rows) == m["n_rows"]
    if m["n_rows"] == 0:
        assert np.isnan(got["awd"]) and np.isnan(got["scs"])
        return
    assert np.array_equal(rows[:, 0:6], m["rows"][:, 0:6]) and np.array_equal(rows[:, 10:12], m["rows"][:, 10:12])
    for c, n in ((6, rows[:, 11]), (18, rows[:, 10])):
        assert (np.abs(rows[:, c:c + 3] - m["rows"][:, c:c + 3]).max(axis=1) <= mu_bound(n, m["rows"][:, c:c + 3], vs)).all()
    assert_sigma_close(rows[:, 12:18], m["rows"][:, 12:18])
    assert_sigma_close(rows[:, 21:27], m["rows"][:, 21:27])
    # W of each row against the model ON THE ROW'S OWN Gaussians (the voxel build has its own bars above), ground truth first
    e = []
    for r in rows:
        d, s, w = w2_squared(r[18:21], full9(r[21:27])[0], int(r[10]), r[6:9], full9(r[12:18])[0], int(r[11]))
        e.append(w2_error_units(r[9], d, s))
    print(f"\nrows={len(rows)} max e(W)={max(e):.1f} u of {W2_TOL['voxels'][1]:g} u")
    assert max(e) <= W2_TOL["voxels"][1]
    assert np.array_equal(got["w_sorted"], np.sort(rows[:, 9]))
    mean = float(mp.fsum(mp.mpf(float(x)) for x in rows[:, 9]) / len(rows))
    assert abs(got["awd"] - mean) <= (len(rows) + 8) * U * abs(mean)
    keys = np.rint(rows[:, 0:3] / vs).astype(np.int64)
    assert np.array_equal(keys, m["keys"])
    s, per, n_max = scs(keys, rows[:, 9], radius)  # of the W the rows hold
    if np.isnan(s):
        assert np.isnan(got["scs"])
    else:
        assert abs(got["scs"] - s) <= scs_bound(n_max, len(rows), radius, per)
