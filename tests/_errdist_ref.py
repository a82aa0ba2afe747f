"""numpy model of the error-distribution metrics (csrc/me_errdist.hip; include/mapeval_hip.h): the multi-rank select by numpy.sort, the
nearest-rank formula, the threshold rule t2max by numpy.nextafter, the histogram by numpy.searchsorted, the sums by math.fsum, the
worst query as the smallest index among the largest d2, and the F-score."""
from __future__ import annotations

import functools
import math

import numpy as np

EPS = 2.0 ** -53
RANK_MAX = 16
MAX_THRESHOLDS = 8
MAX_BINS = 4096
STAT_BLOCKS = 1024     # blocks of k_ed_stat: up to 256 * STAT_BLOCKS entries one per thread, above it a block strides over the array
FINAL_THREADS = 256    # the one-block total: above 256 * FINAL_THREADS entries a thread of the final block adds more than one block partial
IN_FLIGHT = 4          # loads in flight of k_ed_stat's strided walk: taken above IN_FLIGHT * 256 * STAT_BLOCKS entries
DIGIT_BITS = 8         # radix-select digit: eight passes over the 64-bit key
HIST_BLOCKS = 2048     # pieces of the list in k_rs_hist / k_rs_scatter
COMPACT_MIN = 32768    # a list of fewer entries is never compacted
COMPACT_DIV = 8        # a list is compacted when at most 1 / COMPACT_DIV of its entries carried a live prefix in a pass
GATE_LE_UNSQUARED, GATE_LT_SQUARED = 0, 1


def keys_of(values) -> np.ndarray:
    """The selection keys: the bits of v + 0.0 (a negative zero becomes positive)."""
    return (np.asarray(values, np.float64) + 0.0).view(np.uint64)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def rank_select(values, ranks, use=None) -> dict:
    """me_rank_select: count, sum (math.fsum), min, max, value[j] = sorted_used[ranks[j]]."""
    k = keys_of(values)
    if use is not None:
        k = k[np.asarray(use) != 0]
    k = np.sort(k)
    v = k.view(np.float64)
    ranks = np.asarray(ranks, np.int64).reshape(-1)
    if len(v) == 0:
        return {"count": 0, "sum": 0.0, "min": 0.0, "max": 0.0, "value": np.zeros(len(ranks))}
    return {"count": len(v), "sum": math.fsum(v), "min": float(v[0]), "max": float(v[-1]), "value": v[ranks].copy()}


def tree_256(x) -> np.ndarray:
    """block_sum_256 over the last axis (256 threads): every wave of 64 folds its halves, 64 -> 32 -> ... -> 1, then
    (w0 + w1) + (w2 + w3)."""
    w = np.asarray(x, np.float64)
    w = w.reshape(w.shape[:-1] + (4, 64))
    for o in (32, 16, 8, 4, 2, 1):
        w = w[..., :o] + w[..., o:2 * o]
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def block_order_sum(x) -> np.ndarray:
    """One block over the last axis: thread t adds the entries t, t + 256, ... in order, starting from 0.0, then tree_256.  (A missing
    entry is a +0.0: adding it to a sum of non-negative terms changes no bit.)"""
    x = np.asarray(x, np.float64)
    m = x.shape[-1]
    rounds = max(1, -(-m // 256))
    p = np.zeros(x.shape[:-1] + (rounds * 256,))
    p[..., :m] = x
    p = p.reshape(x.shape[:-1] + (rounds, 256))
    acc = np.zeros(x.shape[:-1] + (256,))
    for k in range(rounds):
        acc = acc + p[..., k, :]
    return tree_256(acc)


def rank_select_sum_in_order(values, use=None) -> float:
    """me_rank_select's sum in the order of the device: thread (b, t) of min(STAT_BLOCKS, ceil(n / 256)) blocks adds v[i] for
    i = 256 b + t, stepping by the grid size (an unused entry adds nothing but keeps its place); a block folds by tree_256; one block
    adds the block partials by the same rule.  0.0 without a used entry."""
    v = np.asarray(values, np.float64)
    n = len(v)
    if use is not None:
        v = np.where(np.asarray(use) != 0, v, 0.0)
    nb = min(STAT_BLOCKS, max(1, -(-n // 256)))
    grid = 256 * nb
    rounds = max(1, -(-n // grid))
    p = np.zeros(rounds * grid)
    p[:n] = v
    per_block = p.reshape(rounds, nb, 256).transpose(1, 0, 2).reshape(nb, rounds * 256)  # (b, k, t) = v[k grid + 256 b + t]
    return float(block_order_sum(block_order_sum(per_block)))


def sum_bound(count, total) -> float:
    """|sum_device - sum_exact| <= (count - 1) 2^-53 sum: count - 1 additions of non-negative terms, in any order."""
    return max(float(count) - 1, 0.0) * EPS * float(total)


def nearest_rank(prob: float, n_used: int) -> int:
    """min(n - 1, max(0, ceil(p n) - 1)), one fp64 multiplication; -1 without a used entry."""
    if n_used <= 0:
        return -1
    return min(n_used - 1, max(0, int(math.ceil(float(prob) * float(n_used))) - 1))


def t2max(t: float) -> float:
    """The largest double whose correctly rounded sqrt is <= t (make_params' rule)."""
    t = float(t)
    if not t >= 0:
        return -1.0
    x = np.float64(t) * np.float64(t)
    while np.sqrt(np.nextafter(x, np.inf)) <= t:
        x = np.nextafter(x, np.inf)
    while x > 0 and np.sqrt(x) > t:
        x = np.nextafter(x, -np.inf)
    return float(x)


@functools.lru_cache(maxsize=16)
def edges(n_bins: int, bin_width: float) -> np.ndarray:
    """E_j = t2max(j * bin_width), j = 1 .. n_bins."""
    return np.array([t2max(float(j) * float(bin_width)) for j in range(1, n_bins + 1)], np.float64)


def gate_mask(d2, gate: float, gate_mode: int) -> np.ndarray:
    d2 = np.asarray(d2, np.float64)
    m = d2 >= 0
    if gate < 0:
        return m
    if gate_mode == GATE_LT_SQUARED:
        return m & (d2 < gate * gate)
    return m & (d2 <= gate)


def fscore(n_within_est: int, n_est: int, n_within_gt: int, n_gt: int):
    P = n_within_est / n_est if n_est > 0 else 0.0
    R = n_within_gt / n_gt if n_gt > 0 else 0.0
    return P, R, (2 * P * R / (P + R) if P + R > 0 else 0.0)


def error_distribution(d2, quantiles=(), thresholds=(), bins: int = 0, bin_width: float = 0.0, gate: float = -1.0,
                       gate_mode: int = GATE_LE_UNSQUARED) -> dict:
    """me_nn_error_distribution on the squared distances in cloud order."""
    d2 = np.asarray(d2, np.float64)
    m = gate_mask(d2, gate, gate_mode)
    u = d2[m] + 0.0
    n_used = len(u)
    s = np.sort(u.view(np.uint64)).view(np.float64)
    out = {"n_query": int((d2 >= 0).sum()), "n_used": n_used, "sum_d": math.fsum(np.sqrt(u)), "sum_d2": math.fsum(u),
           "min_d2": float(s[0]) if n_used else 0.0, "max_d2": float(s[-1]) if n_used else 0.0}
    out["min_d"], out["max_d"] = math.sqrt(out["min_d2"]), math.sqrt(out["max_d2"])
    out["argmax"] = int(np.flatnonzero(m & (d2 == out["max_d2"]))[0]) if n_used else -1
    out["rank"] = np.array([nearest_rank(p, n_used) for p in quantiles], np.int64)
    out["quantile_d2"] = np.array([s[r] if r >= 0 else 0.0 for r in out["rank"]], np.float64)
    out["quantile_d"] = np.sqrt(out["quantile_d2"])
    out["n_within"] = np.array([int((u <= t2max(t)).sum()) for t in thresholds], np.int64)
    if bins > 0:
        E = edges(bins, bin_width)
        c = np.bincount(np.searchsorted(E, u, side="left"), minlength=bins + 1)
        out["hist"], out["n_overflow"] = c[:bins].astype(np.int64), int(c[bins])
    else:
        out["hist"], out["n_overflow"] = np.zeros(0, np.int64), 0
    return out
