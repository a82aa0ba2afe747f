"""Hand-built clouds for me_perturb_cloud (csrc/me_perturb.hip) at its exact edges, each with the numpy model's result.

A case is a dict: "name", "src" (the source cloud, read-only), "kw" (the keyword arguments of Engine.perturb, seed included),
"ref" (R.perturb(src, **kw)), "hits" (what the case is built to hit) and, per family, what the builder knows beyond the model
(the keep pattern, the listed outlier count, the mpmath flags); "cell" is the cell size to upload the source with (the index
admits 2^21 cells per axis, so the survey-sized clouds ask for a coarser one).  Needs numpy, mpmath and _perturb_ref only; shared by
test_perturb_edges_cpu.py (every case hits its edge under the model alone) and test_gpu_perturb_edges.py (the device against it).

Coordinates are dyadic wherever exactness is claimed, and no coordinate is -0.0 (the kernel's x + 0 n turns one into +0.0)."""
import math

import mpmath
import numpy as np

import _perturb_ref as R

mpmath.mp.dps = 50

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 20_001)  # around a wave, a block, the scan's tile; > 1 tile
SEEDS = (0, 1, 7, (1 << 32) + 7, 1 << 63, (1 << 64) - 1)
OUTLIER_COUNTS = ((100, 0.29, 28), (100, 0.57, 56), (10, 0.7, 7), (3, 1.0 / 3.0, 1), (1, 1.0, 1), (1, 0.999, 0), (257, 1.0, 257),
                  (4097, 0.05, 204))  # (n, ratio, m): 100 * 0.29 = 28.999999999999996, 100 * 0.57 = 56.99999999999999
BIG_REGION = 2.0 ** 20  # every lattice point of this file lies in (0, BIG_REGION)^2: one region, so u alone decides


def _case(name, src, kw, hits, **extra):
    src = np.ascontiguousarray(src, np.float64)
    src.setflags(write=False)
    return {"name": name, "src": src, "kw": kw, "ref": R.perturb(src, **kw), "hits": hits, "cell": 0.2, **extra}


def lattice(n, y_sign=None):
    """n distinct dyadic points with x in (0, 1): x = (i % 128 + 1) / 256, y = +-0.5 (y_sign[i]; +0.5 without), z = (i // 128) / 8"""
    i = np.arange(n)
    y = np.full(n, 0.5) if y_sign is None else np.where(y_sign, 0.5, -0.5)
    return np.stack([(i % 128 + 1) / 256.0, y, (i // 128) / 8.0], axis=1)


# ---- geometry-decided keep patterns ---------------------------------------------------------------------------------------------------
def keep_patterns(n):
    """name -> bool[n], deduplicated by content (at n = 1 "first", "last" and "all" are one pattern)"""
    i = np.arange(n)
    pats = {"all": np.ones(n, bool), "first": i == 0, "last": i == n - 1, "all_but_first": i != 0, "all_but_last": i != n - 1,
            "alternating": i % 2 == 0, "alternating_from_1": i % 2 == 1, "runs_64": (i // 64) % 2 == 0, "runs_64_from_1": (i // 64) % 2 == 1,
            "runs_256": (i // 256) % 2 == 0, "runs_256_from_1": (i // 256) % 2 == 1}
    for lone in (255, 256, 257):
        if lone < n:
            pats[f"lone_{lone}"] = i == lone
    out, seen = {}, set()
    for name, p in pats.items():
        if p.tobytes() not in seen:
            seen.add(p.tobytes())
            out[name] = p
    return out


def pattern_cases(n):
    """With sparse_ratio = 1, dense_ratio = 0 the keep flag is the point's alone (u < 1 always, u < 0 never): a point in (0, 1)^2 is
    kept, one in (0, 1) x (-1, 0) dropped (region_size = 1).  With the ratios swapped the survivors are the complement.  A pattern
    without a survivor is a refused call ("expect" is None then)."""
    cases = []
    for name, pat in keep_patterns(n).items():
        src = lattice(n, pat)
        for swapped in (False, True):
            kw = dict(sparse_ratio=0.0 if swapped else 1.0, dense_ratio=1.0 if swapped else 0.0, region_size=1.0, seed=7)
            want = ~pat if swapped else pat
            c = _case(f"pattern/{n}/{name}/{'swapped' if swapped else 'plain'}", src, kw, "compaction: keep flags -> scan -> scatter",
                      pattern=want, expect=src[want] if want.any() else None)
            cases.append(c)
    return cases


# ---- region borders ---------------------------------------------------------------------------------------------------------------------
def _arg(v, region):
    return np.float64(v) / np.float64(region) * np.float64(np.pi)  # fl(fl(v / region) pi), the kernel's own expression


def sine_sign(v, region):
    """the sign of sin at the fp64 argument fl(v / region pi), from mpmath at 50 digits: -1, 0 or 1"""
    return int(mpmath.sign(mpmath.sin(mpmath.mpf(float(_arg(v, region))))))


def border_points(region):
    """-> (xyz, what): one point per border value and partner.  x on a border with y = +-region / 2 (a kept and a dropped partner
    under sparse = 1, dense = 0), y on a border with x = +-region / 2, and both at survey offsets at once."""
    h = region / 2.0
    xs = [0.0] + [s * m * region for m in (1.0, 2.0, 3.0) for s in (1.0, -1.0)] + [4e5 + k for k in range(-3, 4)]
    ys = [0.0] + [s * m * region for m in (1.0, 2.0, 3.0) for s in (1.0, -1.0)] + [3e6 + k for k in range(-3, 4)]
    # fl(k region), k = 1 .. 2000: for a region that is no power of two x / region lands on, just below or just above the integer, and
    # x (pi / region) rounds differently from x / region pi (the reciprocal-multiply the kernel must not use)
    xs += [k * region for k in range(4, 2001)]
    pts, what = [], []
    for x in xs:
        for y in (h, -h):
            pts.append((x, y))
            what.append("x")
    for y in ys:
        for x in (h, -h):
            pts.append((x, y))
            what.append("y")
    for k in range(-3, 4):
        pts.append((4e5 + k, 3e6 + k))
        what.append("xy")
    xy = np.array(pts)
    return np.column_stack([xy, np.arange(len(xy)) / 8.0]), what


def border_cases():
    """One cloud per region size and ratio assignment.  "mp_product_sign" is the sign of sin sin from mpmath; the builder asserts that
    the model's flag agrees with it, so the expected survivors rest on the high-precision value and not on the libm in use.
    "left_out" counts the points dropped because an mpmath sine is exactly 0 away from argument 0 (there are none)."""
    cases = []
    for region in (1.0, 0.3):
        xyz, what = border_points(region)
        sx = np.array([sine_sign(v, region) for v in xyz[:, 0]])
        sy = np.array([sine_sign(v, region) for v in xyz[:, 1]])
        zero_off_origin = ((sx == 0) & (xyz[:, 0] != 0)) | ((sy == 0) & (xyz[:, 1] != 0))
        left_out = int(zero_off_origin.sum())
        xyz, sx, sy = xyz[~zero_off_origin], sx[~zero_off_origin], sy[~zero_off_origin]
        positive = sx * sy > 0
        for swapped in (False, True):
            kw = dict(sparse_ratio=0.0 if swapped else 1.0, dense_ratio=1.0 if swapped else 0.0, region_size=region, seed=7)
            c = _case(f"border/{region}/{'swapped' if swapped else 'plain'}", xyz, kw, "the region rule at products of 0, at +-k region "
                      "and at survey offsets", mp_positive=positive, left_out=left_out, what=what, cell=4.0)
            want = ~positive if swapped else positive
            assert np.array_equal(c["ref"]["src_index"], np.nonzero(want)[0]), "the numpy model's flags differ from the mpmath signs"
            cases.append(c)
    return cases


def reciprocal_multiply_flips(c):
    """how many points of a border case would change sides under sin(x (pi / region)) in place of sin(x / region pi)"""
    region = np.float64(c["kw"]["region_size"])
    x, y = c["src"][:, 0], c["src"][:, 1]
    alt = np.sin(x * (np.pi / region)) * np.sin(y * (np.pi / region)) > 0
    return int((alt != c["mp_positive"]).sum())


# ---- deformation ------------------------------------------------------------------------------------------------------------------------
DC = (1.5, -2.25, 0.5)  # dyadic centre
DR = 2.5                # dyadic radius; (1.5, 2, 0) has length exactly 2.5
D_BELOW = math.nextafter(DR, 0.0)  # = fl(R (1 - 2^-52)), one ulp inside


def deform_points():
    c = np.array(DC)
    rows = {"at_R_x": c + [DR, 0, 0], "at_R_minus_y": c + [0, -DR, 0], "at_R_z": c + [0, 0, DR], "at_R_345": c + [1.5, 2.0, 0],
            "at_R_345_b": c + [0, -2.0, 1.5], "below_R_x": c + [D_BELOW, 0, 0], "centre": c, "half_R_x": c + [DR / 2, 0, 0],
            "half_R_minus_z": c + [0, 0, -DR / 2], "inside": c + [0.375, -0.5, 1.0], "outside": c + [3.0, 1.0, 0]}
    names = list(rows)
    return names, np.array([rows[k] for k in names])


def w_exact(d, radius):
    """0.5 (1 + cos(pi d / R)) at 50 digits"""
    return mpmath.mpf("0.5") * (1 + mpmath.cos(mpmath.pi * mpmath.mpf(d) / mpmath.mpf(radius)))


def deform_cases():
    names, pts = deform_points()
    cases = []
    for tag, radius, strength in (("plain", DR, 0.3), ("negative", DR, -0.3), ("inf_R", math.inf, 0.3), ("nan_R", math.nan, 0.3),
                                  ("big_strength", DR, 2.0 ** 20)):
        kw = dict(deform_radius=radius, deform_strength=strength, deform_center=DC, seed=7)
        copies = list(range(len(names))) if tag == "nan_R" else [i for i, k in enumerate(names) if k == "centre" or (
            radius == DR and (k.startswith("at_R") or k == "outside"))]
        cases.append(_case(f"deform/{tag}", pts, kw, "strict d < R, d == 0, R (1 - 2^-52), R / 2, -strength, R = inf, R = NaN",
                           names=names, copies=copies, cell=4.0 if tag == "big_strength" else 0.2))
    # a point the deformation carries across a region border, density on (region 1, sparse 1, dense 0): the keep decision is the
    # deformed point's.  (0.875, 0.5) is pushed from c = (0.5, 0.5) to x ~ 1.08: kept -> dropped; (1.125, 0.5) from c = (1.5, 0.5)
    # to x ~ 0.92: dropped -> kept.  The bystanders lie outside the radius and keep every call alive.
    for tag, cx, px in (("kept_to_dropped", 0.5, 0.875), ("dropped_to_kept", 1.5, 1.125)):
        pts2 = np.array([[8.25, -0.5, 0.25], [px, 0.5, 0.25], [8.25, 0.5, 0.25]])  # (a dropped and a kept bystander around it)
        kw = dict(deform_radius=1.0, deform_strength=0.3, deform_center=(cx, 0.5, 0.25), sparse_ratio=1.0, dense_ratio=0.0,
                  region_size=1.0, seed=7)
        cases.append(_case(f"deform/flip/{tag}", pts2, kw, "the keep pass deforms before it decides", flips=tag))
    return cases


# ---- outlier counts and bases -----------------------------------------------------------------------------------------------------------
def outlier_cases():
    cases = []
    for n, ratio, m in OUTLIER_COUNTS:
        kw = dict(outlier_ratio=ratio, outlier_range=0.0, seed=7)
        cases.append(_case(f"outliers/{n}/{ratio:.3f}", lattice(n), kw, "m = (int64)(n_kept ratio); bases bit for bit at range 0", m=m))
    n = 4097
    kw = dict(outlier_ratio=0.3, outlier_range=0.0, sparse_ratio=0.5, dense_ratio=0.5, region_size=BIG_REGION, seed=7)
    cases.append(_case("outliers/density_on", lattice(n), kw, "the bases index the compacted cloud", m=None))
    kw = dict(outlier_ratio=0.5, outlier_range=0.0, noise_std=0.05, seed=7)
    cases.append(_case("outliers/noised_base", lattice(257), kw, "an outlier at range 0 is a copy of the noised base", m=128))
    kw = dict(outlier_ratio=0.25, outlier_range=1.5, noise_std=0.05, sparse_ratio=0.3, dense_ratio=0.9, region_size=0.25,
              deform_radius=1.0, deform_strength=0.3, deform_center=(0.5, 0.5, 2.0), seed=(1 << 32) + 7)
    i = np.arange(n)
    src = lattice(n, i % 3 != 0)
    cases.append(_case("outliers/all_stages", src, kw, "noise counter = the source index, all four stages together", m=None))
    return cases


# ---- seeds ------------------------------------------------------------------------------------------------------------------------------
def seed_cases():
    src = lattice(4097)
    cases = [_case(f"seed/{s}", src, dict(sparse_ratio=0.5, dense_ratio=0.5, region_size=BIG_REGION, seed=s), "the 64-bit Philox key")
             for s in SEEDS]
    by_seed = {c["kw"]["seed"]: c["ref"]["src_index"] for c in cases}
    assert not np.array_equal(by_seed[7], by_seed[(1 << 32) + 7]), "seeds 7 and 2^32 + 7 keep the same points under the model"
    return cases


def all_cases():
    out = []
    for n in SIZES:
        out += pattern_cases(n)
    return out + border_cases() + deform_cases() + outlier_cases() + seed_cases()
