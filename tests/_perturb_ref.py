"""numpy model of me_perturb_cloud (csrc/me_perturb.hip): the reference's four simulation-mode generators (map_eval.cpp:1745-1829)
with the counter-based randomness the library uses in place of the reference's unseeded mt19937.

Philox4x64-10 (Random123) is written out vectorised, the 64 x 64 -> 128-bit multiply split into 32-bit halves; the word assignment is
the one include/mapeval_hip.h documents:
    density  of source point i   counter (i, 1, 0, 0)   w0 -> u
    noise    of source point i   counter (i, 2, 0, 0)   Box-Muller (w0, w1) -> x, y;  (w2, w3) -> z
    outlier j                    counter (j, 3, 0, 0)   w0 -> base;  Box-Muller (w1, w2) -> x, y
                                 counter (j, 3, 1, 0)   Box-Muller (w0, w1) -> z
"""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
PHILOX_M = (0xD2E7470EE14C6C93, 0xCA5A826395121157)
PHILOX_W = (0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B)


def mulhilo64(a: int, b: np.ndarray):
    """(hi, lo) of the 128-bit product of the constant a and every word of b, from 32-bit halves."""
    b = b.astype(np.uint64)
    a_lo, a_hi = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    b_lo, b_hi = b & _M32, b >> _S32
    p0 = a_lo * b_lo
    p1 = a_lo * b_hi
    p2 = a_hi * b_lo
    p3 = a_hi * b_hi
    mid = (p0 >> _S32) + (p1 & _M32) + (p2 & _M32)
    hi = p3 + (p1 >> _S32) + (p2 >> _S32) + (mid >> _S32)
    lo = (mid << _S32) | (p0 & _M32)
    return hi, lo


def philox4x64_10(c0, c1, c2, c3, k0: int, k1: int = 0):
    """Random123 philox4x64_R(10, ctr, key) for arrays of counter words; returns the four output words."""
    n = max(np.size(c) for c in (c0, c1, c2, c3))
    c = [np.broadcast_to(np.asarray(w, dtype=np.uint64), (n,)).copy() for w in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & M64, int(k1) & M64
    for r in range(10):
        if r > 0:
            k0 = (k0 + PHILOX_W[0]) & M64
            k1 = (k1 + PHILOX_W[1]) & M64
        hi0, lo0 = mulhilo64(PHILOX_M[0], c[0])
        hi1, lo1 = mulhilo64(PHILOX_M[1], c[2])
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return c


def u01(w):  # [0, 1)
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def u01_open0(w):  # (0, 1]
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def box_muller(a, b):
    r = np.sqrt(-2.0 * np.log(u01_open0(a)))
    t = (2.0 * np.pi) * u01(b)
    return r * np.cos(t), r * np.sin(t)


def _block(seed: int, idx, c1: int, c2: int = 0):
    return philox4x64_10(np.asarray(idx, dtype=np.uint64), c1, c2, 0, seed, 0)


# ---- the four stages ---------------------------------------------------------------------------------------------------------------
def deform(pts: np.ndarray, radius: float, strength: float, center) -> np.ndarray:
    """addLocalDeformation (:1808-1825): d = (p - c).norm() = sqrt((dx^2 + dy^2) + dz^2); d < R strictly; w = 0.5 (1 + cos(pi d / R));
    p += (p - c) / d * s * w; a point at d == 0 stays (Eigen 3.3's normalize() leaves a zero vector)."""
    out = np.array(pts, dtype=np.float64, copy=True)
    if not (radius > 0) or strength == 0:
        return out
    dv = out - np.asarray(center, dtype=np.float64)
    d = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
    m = (d < radius) & (d > 0)
    dm = d[m]
    w = 0.5 * (1.0 + np.cos(np.pi * dm / radius))
    for a in range(3):
        out[m, a] += dv[m, a] / dm * strength * w
    return out


def density_keep(pts: np.ndarray, sparse_ratio: float, dense_ratio: float, region_size: float, seed: int) -> np.ndarray:
    """addNonUniformDensity (:1766-1780): keep mask of the (deformed) points, in source order."""
    n = len(pts)
    if not (region_size > 0):
        return np.ones(n, bool)
    xn = np.sin(pts[:, 0] / region_size * np.pi)
    yn = np.sin(pts[:, 1] / region_size * np.pi)
    keep = np.where(xn * yn > 0, sparse_ratio, dense_ratio)
    u = u01(_block(seed, np.arange(n, dtype=np.uint64), 1)[0])
    return u < keep


def gaussian_noise(n_src: int, src_idx: np.ndarray, sigma: float, seed: int) -> np.ndarray:
    """addGaussianNoise (:1750-1754): the N(0, sigma^2) offsets of the source points src_idx, (len, 3)."""
    w = _block(seed, np.asarray(src_idx, dtype=np.uint64), 2)
    nx, ny = box_muller(w[0], w[1])
    nz, _ = box_muller(w[2], w[3])
    return sigma * np.stack([nx, ny, nz], axis=1)


def outlier_bases(n_kept: int, m: int, seed: int) -> np.ndarray:
    """b_j = min(n_kept - 1, (int64)(u n_kept)) (:1797; the clamp replaces the reference's read one past the end)."""
    u = u01(_block(seed, np.arange(m, dtype=np.uint64), 3)[0])
    return np.minimum(n_kept - 1, (u * float(n_kept)).astype(np.int64))


def outlier_offsets(m: int, range_: float, seed: int) -> np.ndarray:
    j = np.arange(m, dtype=np.uint64)
    w = _block(seed, j, 3, 0)
    v = _block(seed, j, 3, 1)
    nx, ny = box_muller(w[1], w[2])
    nz, _ = box_muller(v[0], v[1])
    return range_ * np.stack([nx, ny, nz], axis=1)


# ---- the bounds of the device tests (test_gpu_perturb.py, test_gpu_perturb_edges.py): one place, so that the two cannot drift -------
def survivor_bound(sigma: float, deformed: np.ndarray, strength: float) -> np.ndarray:
    """|(device survivor - model's deformed point) - model's noise| stays below this: 1e-12 sigma (a log, sqrt, sin or cos that differs
    by an ulp) plus the rounding of the subtraction and of a deform cos that may differ by an ulp."""
    return 1e-12 * sigma + (2 * np.spacing(np.abs(deformed)) + 4 * np.spacing(abs(strength)))


def outlier_bound(range_: float, outliers: np.ndarray) -> np.ndarray:
    """|(device outlier - its base point as downloaded) - model's N(0, range^2) offset| stays below this."""
    return 1e-12 * range_ + 2 * np.spacing(np.abs(outliers))


def perturb(src: np.ndarray, *, noise_std=0.0, sparse_ratio=1.0, dense_ratio=1.0, region_size=0.0, outlier_ratio=0.0,
            outlier_range=0.0, deform_radius=0.0, deform_strength=0.0, deform_center=(0.0, 0.0, 0.0), seed=0) -> dict:
    """The whole pipeline: deform -> density -> noise -> outliers.  Returns the points and what the tests compare: the survivors'
    source indices, the deformed survivors (before the noise), the noise offsets and the outliers' base indices."""
    src = np.asarray(src, dtype=np.float64)
    n = len(src)
    p = deform(src, deform_radius, deform_strength, deform_center)
    keep = density_keep(p, sparse_ratio, dense_ratio, region_size, seed)
    idx = np.nonzero(keep)[0]
    deformed = p[idx]
    noise = gaussian_noise(n, idx, noise_std, seed) if noise_std != 0 else np.zeros((len(idx), 3))
    kept = deformed + noise
    n_kept = len(idx)
    m = int(np.int64(float(n_kept) * outlier_ratio)) if outlier_ratio > 0 else 0
    bases = outlier_bases(n_kept, m, seed) if m else np.zeros(0, np.int64)
    outl = kept[bases] + outlier_offsets(m, outlier_range, seed) if m else np.zeros((0, 3))
    return {"points": np.concatenate([kept, outl]), "src_index": idx, "deformed": deformed, "noise": noise, "n_kept": n_kept,
            "bases": bases}
