"""Numpy model of the cloud preparation and output steps (csrc/me_index.hip k_transform / k_ingest / k_bbox, csrc/me_voxel.hip
k_vds_keys .. k_vds_mean, csrc/me_render.hip), restated operation by operation in the order of the source comments.  numpy's ufuncs
round every product and every sum on its own (no FMA), which is what the library is compiled to do (-ffp-contract=off), so every
function here is meant to be compared with the device BIT FOR BIT; the one exception is the two `log` calls of render_entropy, which
run the host's libm here (math.log) and the device's `log` there.  No GPU and no oracle import."""
import math

import numpy as np

KEY_LIMIT = 2097151  # 2^21 - 1: the largest voxel index per axis of the 63-bit key
REFUSED = None       # downsample()'s error marker (the library: ME_ERR_ARG, slot untouched)
JET_BREAKS = (-0.75, -0.25, 0.25, 0.75)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ---- transform and bounding box ---------------------------------------------------------------------------------------------------------
def transform(xyz, T):
    """Open3D PointCloud::Transform: h_r = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3], p = h[:3] / h[3]."""
    xyz, T = _f64(xyz), _f64(T).reshape(4, 4)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        h = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(4)]
        return np.stack([h[0] / h[3], h[1] / h[3], h[2] / h[3]], axis=1)


def homogeneous_w(xyz, T):
    xyz, T = _f64(xyz), _f64(T).reshape(4, 4)
    return ((T[3, 0] * xyz[:, 0] + T[3, 1] * xyz[:, 1]) + T[3, 2] * xyz[:, 2]) + T[3, 3]


def bbox(xyz):
    xyz = _f64(xyz)
    return xyz.min(axis=0), xyz.max(axis=0)


# ---- VoxelDownSample ----------------------------------------------------------------------------------------------------------------------
def voxel_index(xyz, vs):
    """floor((p - (min - vs * 0.5)) / vs) per component, as float64 (the division is kept: no multiplication by 1 / vs)."""
    xyz = _f64(xyz)
    origin = bbox(xyz)[0] - vs * 0.5
    with np.errstate(all="ignore"):
        return np.floor((xyz - origin) / vs)


def downsample(xyz, vs, normals=None):
    """-> REFUSED, or dict(points (V,3), normals (V,3) or None, keys (V,) uint64 ascending, counts (V,), index (n,3) int64, voxel_of (n,)).
    A voxel's sum starts at 0.0 and adds its points one by one in ORIGINAL index order, then divides by the count; the normals go
    through the same permutation and segments and are not re-normalised."""
    xyz = _f64(xyz)
    if not (vs > 0):
        return REFUSED
    f = voxel_index(xyz, vs)
    if not ((f >= 0) & (f <= KEY_LIMIT)).all():  # (NaN fails both comparisons: vs = inf gives inf / inf)
        return REFUSED
    idx = f.astype(np.int64)
    key = ((idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]).astype(np.uint64)
    keys, voxel_of, counts = np.unique(key, return_inverse=True, return_counts=True)  # ascending key order
    voxel_of = voxel_of.reshape(-1)

    def mean(a):
        acc = np.zeros((len(keys), 3), np.float64)
        np.add.at(acc, voxel_of, a)  # unbuffered: one addition per point, in index order
        return acc / counts[:, None].astype(np.float64)

    return dict(points=mean(xyz), normals=None if normals is None else mean(_f64(normals)), keys=keys, counts=counts, index=idx,
                voxel_of=voxel_of)


# ---- ColorMapJet -----------------------------------------------------------------------------------------------------------------------------
def _interpolate(v, y0, x0, y1, x1):
    with np.errstate(all="ignore"):
        mid = (v - x0) * (y1 - y0) / (x1 - x0) + y0
    return np.where(v < x0, y0, np.where(v > x1, y1, mid))


def jet_base(v):
    """Five `<=` comparisons in order; NaN fails every one of them and falls through to 0.0."""
    v = _f64(v)
    with np.errstate(invalid="ignore"):
        return np.select([v <= -0.75, v <= -0.25, v <= 0.25, v <= 0.75],
                         [0.0, _interpolate(v, 0.0, -0.75, 1.0, -0.25), 1.0, _interpolate(v, 1.0, 0.25, 0.0, 0.75)], default=0.0)


def jet_args(value):
    value = _f64(value)
    with np.errstate(invalid="ignore"):
        return np.stack([value * 2.0 - 1.5, value * 2.0 - 1.0, value * 2.0 - 0.5], axis=-1)


def jet_color(value):
    return jet_base(jet_args(value))


# ---- renderDistanceOnPointCloud --------------------------------------------------------------------------------------------------------------
def render_distance(d2, dis):
    """e = min(d2, dis): the SQUARED distance against the UNSQUARED threshold (sic, map_eval.cpp:591-595); colour = Jet(e / dis)."""
    d2 = _f64(d2)
    e = np.where(d2 > dis, dis, d2)
    return jet_color(e / dis)


def inliers(d2, gate, mode):
    """gate < 0: everybody.  mode 0: d2 <= gate.  mode 1: d2 < gate * gate, the product formed once in fp64."""
    d2 = _f64(d2)
    if gate < 0:
        return np.ones(len(d2), bool)
    if mode == 1:
        g2 = np.float64(gate) * np.float64(gate)
        return d2 < g2
    return d2 <= gate


# ---- ColorPointCloudByMME -------------------------------------------------------------------------------------------------------------------
def _log(x):
    """C's log on the host's libm, with its special values (math.log raises where C returns NaN or -inf)."""
    if x != x or x < 0.0:
        return math.nan
    if x == 0.0:
        return -math.inf
    return math.log(x)


def render_entropy(xyz, ent, valid):
    """-> dict(xyz (m,3), rgb (m,3), n_valid, min_abs, max_abs, ne (m,): the mapped value that went into Jet).
    The range runs over ALL non-zero entries, valid or not; max_abs = |min|, min_abs = |max| (map_eval.cpp:698-699, swapped on
    purpose); an empty range leaves min = +inf, max = -inf, so both are inf.  Only valid points come out, in cloud order."""
    xyz, ent = _f64(xyz), _f64(ent)
    valid = np.asarray(valid).astype(bool)
    nz = ent[ent != 0.0]
    mn = nz.min() if len(nz) else math.inf
    mx = nz.max() if len(nz) else -math.inf
    max_abs, min_abs = abs(float(mn)), abs(float(mx))
    eps = 1e-1
    keep = np.nonzero(valid)[0]
    with np.errstate(all="ignore"):
        ne0 = (np.abs(ent[keep]) - min_abs) / np.float64(max_abs - min_abs)
    lo, hi = _log(eps), _log(1.0 + eps)
    with np.errstate(all="ignore"):
        ne = np.array([(_log(float(v + eps)) - lo) for v in ne0], np.float64).reshape(-1) / np.float64(hi - lo)
    return dict(xyz=xyz[keep].copy(), rgb=jet_color(ne).reshape(-1, 3), n_valid=len(keep), min_abs=min_abs, max_abs=max_abs, ne=ne)


def jet_exact_mask(ne):
    """(m,3) bool: the channels of Jet(ne) that a last-place difference in `log` cannot move: NaN (every comparison fails: 0.0), or an
    argument more than 1e-6 inside a plateau of jet_base (the channel is exactly 0.0 or 1.0 there)."""
    a = jet_args(ne)
    with np.errstate(invalid="ignore"):
        far = np.ones(a.shape, bool)
        for b in JET_BREAKS:
            far &= np.abs(a - b) > 1e-6
        plateau = (a <= -0.75) | ((a > -0.25) & (a <= 0.25)) | (a > 0.75)
    return np.isnan(a) | (far & plateau)
