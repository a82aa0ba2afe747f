"""numpy model of MOM (csrc/me_mom.hip; include/mapeval_hip.h): the choice of mutually orthogonal axes among plane records — vectorised
and once more as scalar pure Python — the grouped order statistics by numpy.sort, and the metric from per-point arrays."""
from __future__ import annotations

import itertools
import math

import numpy as np

EPS = 2.0 ** -53
TILE = 2048       # entries of one block of k_gs_stat (256 lanes x 8 entries): the unit of the block-order sum
STAGE = 256       # chunks of the first reduction level: above TILE * STAGE entries a chunk holds more than one block partial
SLICE = 16        # groups per launch of k_gs_hist
DIGIT_BITS = 8    # radix-select digit: eight passes over the 64-bit key
HIST_BLOCKS = 2048  # blocks of k_gs_hist: above 256 * HIST_BLOCKS entries a block strides over the array


# ---- axis choice ------------------------------------------------------------------------------------------------------------
def dot_scalar(u, v) -> float:
    return (float(u[0]) * float(v[0]) + float(u[1]) * float(v[1])) + float(u[2]) * float(v[2])


def _choose(nd, W, eligible, orth):
    """Step 4 on nd directions: the ascending tuple chosen (possibly empty)."""
    for s in (3, 2, 1):
        best, key = None, None
        for tup in itertools.combinations(range(nd), s):  # (lexicographic order: only a strictly better key replaces the first)
            if not all(eligible[g] for g in tup):
                continue
            if not all(orth[a][b] for a, b in itertools.combinations(tup, 2)):
                continue
            k = (min(W[g] for g in tup), sum(W[g] for g in tup))
            if key is None or k > key:
                best, key = tup, k
        if best is not None:
            return best
    return ()


def select_axes_scalar(normals, counts, cos_parallel: float, cos_orthogonal: float, min_axis_points: int):
    """me_mom_select_axes one Python float operation at a time: (dir_of_plane, axes dict)."""
    normals = [tuple(map(float, n[:3])) for n in normals]
    founder, members, W, dirs = [], [], [], []
    for r, n in enumerate(normals):
        g = 0
        while g < len(founder) and not abs(dot_scalar(n, normals[founder[g]])) >= cos_parallel:
            g += 1
        if g == len(founder):
            founder.append(r)
            members.append(0)
            W.append(0)
        dirs.append(g)
        members[g] += 1
        W[g] += int(counts[r])
    nd = len(founder)
    eligible = [W[g] >= min_axis_points for g in range(nd)]
    orth = [[abs(dot_scalar(normals[founder[g]], normals[founder[h]])) <= cos_orthogonal for h in range(nd)] for g in range(nd)]
    tup = _choose(nd, W, eligible, orth)
    axes = [{"direction": g, "n_planes": members[g], "weight": W[g], "rep": np.array(normals[founder[g]])} for g in tup]
    return np.array(dirs, np.int32), {"n_axes": len(tup), "n_directions": nd, "axes": axes}


def select_axes(normals, counts, cos_parallel: float, cos_orthogonal: float, min_axis_points: int):
    """The same with the dot products of all pairs formed at once (the same association, element by element)."""
    P = len(normals)
    if P == 0:
        return np.zeros(0, np.int32), {"n_axes": 0, "n_directions": 0, "axes": []}
    N = np.array([list(n)[:3] for n in normals], np.float64)
    counts = np.asarray(counts, np.int64)
    D = np.abs((N[:, None, 0] * N[None, :, 0] + N[:, None, 1] * N[None, :, 1]) + N[:, None, 2] * N[None, :, 2])
    founder, dirs = [], np.zeros(P, np.int32)
    for r in range(P):
        hit = np.flatnonzero(D[r, founder] >= cos_parallel) if founder else np.zeros(0, np.int64)
        if len(hit):
            dirs[r] = hit[0]
        else:
            dirs[r] = len(founder)
            founder.append(r)
    nd = len(founder)
    W = np.array([int(counts[dirs == g].sum()) for g in range(nd)], np.int64)
    members = np.bincount(dirs, minlength=nd)
    orth = D[np.ix_(founder, founder)] <= cos_orthogonal
    tup = _choose(nd, W.tolist(), (W >= min_axis_points).tolist(), orth.tolist())
    axes = [{"direction": g, "n_planes": int(members[g]), "weight": int(W[g]), "rep": N[founder[g]].copy()} for g in tup]
    return dirs, {"n_axes": len(tup), "n_directions": nd, "axes": axes}


def same_axes(a, b) -> bool:
    return (a["n_axes"], a["n_directions"]) == (b["n_axes"], b["n_directions"]) and all(
        (x["direction"], x["n_planes"], x["weight"]) == (y["direction"], y["n_planes"], y["weight"]) and np.array_equal(x["rep"], y["rep"])
        for x, y in zip(a["axes"], b["axes"]))


def cosines(parallel_deg: float, orthogonal_deg: float):
    """Engine's and the host's conversion: cos(parallel), cos(90 - orthogonal) = sin(orthogonal)."""
    return math.cos(parallel_deg * (math.pi / 180.0)), math.sin(orthogonal_deg * (math.pi / 180.0))


# ---- grouped order statistics --------------------------------------------------------------------------------------------------
def keys_of(values) -> np.ndarray:
    """The selection keys: the bits of v + 0.0 (a negative zero becomes positive)."""
    return (np.asarray(values, np.float64) + 0.0).view(np.uint64)


def order_stats(values, groups, n_groups: int) -> dict:
    """me_group_order_stats by numpy.sort on the keys; the sum by math.fsum (correctly rounded)."""
    keys = keys_of(values)
    groups = np.asarray(groups, np.int64)
    out = {"count": np.zeros(n_groups, np.int64)}
    for f in ("sum", "min", "max", "lower", "upper"):
        out[f] = np.zeros(n_groups, np.float64)
    for g in range(n_groups):
        k = np.sort(keys[groups == g])
        c = len(k)
        if c == 0:
            continue
        v = k.view(np.float64)
        out["count"][g] = c
        out["sum"][g] = math.fsum(v)
        out["min"][g], out["max"][g] = v[0], v[-1]
        out["lower"][g], out["upper"][g] = v[(c - 1) // 2], v[c // 2]
    out["median"] = (out["lower"] + out["upper"]) / 2
    return out


def group_sums_in_order(values, groups, n_groups: int) -> np.ndarray:
    """me_group_order_stats' per-group sums in the order of the device: a block holds TILE entries, thread t adds its eight entries
    t, t + 256, ... in order (an entry of another group adds nothing but keeps its place) and the block tree follows; STAGE chunk
    blocks add the block partials of their chunk by the same rule, then one block adds the STAGE results."""
    from _errdist_ref import block_order_sum

    v = np.asarray(values, np.float64) + 0.0
    g = np.asarray(groups, np.int64)
    n = len(v)
    nb = max(1, -(-n // TILE))
    chunk = -(-nb // STAGE)
    vp, gp = np.zeros(nb * TILE), np.full(nb * TILE, -1, np.int64)
    vp[:n], gp[:n] = v, g
    out = np.zeros(n_groups, np.float64)
    for k in range(n_groups):
        part = np.zeros(STAGE * chunk)
        part[:nb] = block_order_sum(np.where(gp == k, vp, 0.0).reshape(nb, TILE))
        out[k] = block_order_sum(block_order_sum(part.reshape(STAGE, chunk)))
    return out


def sum_bound(count, total):
    """|sum_device - sum_exact| <= (count - 1) 2^-53 sum: count - 1 additions of non-negative terms, each partial sum <= the total, in
    any order."""
    return np.maximum(np.asarray(count, np.float64) - 1, 0) * EPS * np.asarray(total, np.float64)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the metric ------------------------------------------------------------------------------------------------------------------
def mom(l3, valid, labels, planes, cos_parallel: float, cos_orthogonal: float, min_axis_points: int):
    """me_mom from per-point arrays in cloud order (l3 and the validity byte of me_local_geometry, the labels of me_segment_planes)
    and the plane records (dicts with "plane" and "count"): (result dict as Engine.mom's, axis byte per point)."""
    l3 = np.asarray(l3, np.float64)
    labels = np.asarray(labels, np.int64)
    dirs, ax = select_axes([p["plane"][:3] for p in planes], [p["count"] for p in planes], cos_parallel, cos_orthogonal, min_axis_points)
    axis_of_dir = {a["direction"]: k for k, a in enumerate(ax["axes"])}
    axis_of_plane = np.array([axis_of_dir.get(int(d), -1) for d in dirs] + [-1], np.int8)  # (the last entry: label -1)
    axis = np.where(np.asarray(valid).astype(bool), axis_of_plane[labels], -1).astype(np.int8)
    st = order_stats(l3, axis, max(1, ax["n_axes"]))
    axes, med, mean = [], 0.0, 0.0
    for k, a in enumerate(ax["axes"]):
        d = {"direction": a["direction"], "n_planes": a["n_planes"], "rep": a["rep"], "n_points": a["weight"], "n_valid": int(st["count"][k])}
        for f, name in (("sum", "sum_l3"), ("min", "min"), ("max", "max"), ("lower", "lower"), ("upper", "upper"), ("median", "median")):
            d[name] = float(st[f][k])
        axes.append(d)
        med += d["median"]
        if d["n_valid"] > 0:
            mean += d["sum_l3"] / d["n_valid"]
    return {"n_axes": ax["n_axes"], "n_directions": ax["n_directions"], "mom_median": med, "mom_mean": mean, "axes": axes}, axis


def box_room(n_per: int = 600, side: float = 8.0, seed: int = 3, noise: float = 0.01, oblique: bool = True) -> np.ndarray:
    """The six faces of a cube of edge `side` and, optionally, one oblique plane through it (x = z), n_per noisy points each, shuffled;
    coordinates rounded to 2^-8."""
    rng = np.random.default_rng(seed)
    parts = []
    for axis in range(3):
        for at in (0.0, side):
            p = rng.uniform(0.0, side, (n_per, 3))
            p[:, axis] = at + rng.normal(scale=noise, size=n_per)
            parts.append(p)
    if oblique:
        p = rng.uniform(0.0, side, (n_per, 3))
        off = rng.normal(scale=noise, size=n_per) / math.sqrt(2.0)
        p[:, 2] = p[:, 0] + off
        p[:, 0] -= off
        parts.append(p)
    xyz = np.round(np.concatenate(parts) * 256.0) / 256.0
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))])
