"""Brute-force numpy model of the neighbour-list searches (me_knn_search, me_hybrid_search, me_radius_search; DESIGN.md section
4.16): the full distance matrix with d2 = (dx*dx + dy*dy) + dz*dz in float64 (numpy evaluates the three products and the two sums one
after the other: no fused multiply-add), every row ordered by np.lexsort((index, d2)) — ascending distance, equal distances by the
smaller index — and strict `<` for the radius.  Nothing here carries a tolerance: the device must reproduce indices and the bit
patterns of d2."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def dist2(q, ref):
    """[nq, nr] squared distances, the library's expression"""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    dx = q[:, None, 0] - ref[None, :, 0]
    dy = q[:, None, 1] - ref[None, :, 1]
    dz = q[:, None, 2] - ref[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def ordered(q, ref):
    """(idx[nq, nr] int32, d2[nq, nr]): every row of the distance matrix in the order of the lists"""
    d2 = dist2(q, ref)
    index = np.broadcast_to(np.arange(d2.shape[1]), d2.shape)
    o = np.lexsort((index, d2), axis=1)
    return o.astype(np.int32), np.take_along_axis(d2, o, axis=1)


def knn_from(order, k):
    """SearchKNN from ordered(): idx / d2 [nq, k], padded with -1 / inf where the reference has fewer than k points"""
    oi, od = order
    nq, nr = oi.shape
    idx = np.full((nq, k), -1, np.int32)
    d2 = np.full((nq, k), np.inf, np.float64)
    m = min(k, nr)
    idx[:, :m] = oi[:, :m]
    d2[:, :m] = od[:, :m]
    return idx, d2


def radius_from(order, radius):
    """SearchRadius from ordered(), as CSR: offsets int64[nq + 1], idx int32[total], d2[total]; membership d2 < radius * radius"""
    oi, od = order
    r2 = float(radius) * float(radius)
    inside = od < r2  # (a prefix of every row: the rows ascend)
    cnt = inside.sum(axis=1)
    off = np.zeros(len(cnt) + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    return off, oi[inside].astype(np.int32), od[inside]


def hybrid_from(order, radius, max_nn):
    """SearchHybrid from ordered(): counts int32[nq], idx / d2 [nq, max_nn] padded with -1 / inf"""
    oi, od = order
    r2 = float(radius) * float(radius)
    cnt = np.minimum((od < r2).sum(axis=1), max_nn).astype(np.int32)
    idx, d2 = knn_from(order, max_nn)
    pad = np.arange(max_nn)[None, :] >= cnt[:, None]
    idx[pad] = -1
    d2[pad] = np.inf
    return cnt, idx, d2


def knn(q, ref, k):
    return knn_from(ordered(q, ref), k)


def radius(q, ref, r):
    return radius_from(ordered(q, ref), r)


def hybrid(q, ref, r, max_nn):
    return hybrid_from(ordered(q, ref), r, max_nn)


def mask_rows_knn(idx, d2, mask):
    """what a masked search returns, from the unmasked lists: padding in the masked-out rows"""
    idx, d2 = idx.copy(), d2.copy()
    out = np.asarray(mask) == 0
    idx[out] = -1
    d2[out] = np.inf
    return idx, d2


def mask_rows_csr(off, idx, d2, mask):
    """... and empty rows in the CSR lists"""
    keep = np.asarray(mask) != 0
    cnt = np.diff(off) * keep
    new = np.zeros(len(off), np.int64)
    np.cumsum(cnt, out=new[1:])
    sel = np.repeat(keep, np.diff(off))
    return new, idx[sel], d2[sel]


def rows_bruteforce(q, ref, k, r, threads=8):
    """For a few queries against a LARGE reference: per query one pass over the whole reference (no matrix).  Returns
    (knn_idx[nq, k], knn_d2[nq, k], radius_rows) with radius_rows a list of (idx, d2) per query.  The k nearest are taken from all
    points at or below the k-th smallest distance (np.partition), so ties at the k-th place are resolved by the index rule too."""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    rx, ry, rz = (np.ascontiguousarray(ref[:, a]) for a in range(3))
    nr = len(ref)
    r2 = float(r) * float(r)
    kk = min(k, nr)
    out_i = np.full((len(q), k), -1, np.int32)
    out_d = np.full((len(q), k), np.inf, np.float64)
    rows = [None] * len(q)

    def work(chunk):
        a, b = np.empty(nr), np.empty(nr)
        for i in chunk:
            np.subtract(q[i, 0], rx, out=a)
            np.multiply(a, a, out=a)
            np.subtract(q[i, 1], ry, out=b)
            np.multiply(b, b, out=b)
            np.add(a, b, out=a)
            np.subtract(q[i, 2], rz, out=b)
            np.multiply(b, b, out=b)
            np.add(a, b, out=a)  # a = (dx*dx + dy*dy) + dz*dz
            kth = np.partition(a, kk - 1)[kk - 1]
            cand = np.flatnonzero(a <= kth)
            o = cand[np.lexsort((cand, a[cand]))][:kk]
            out_i[i, :kk] = o
            out_d[i, :kk] = a[o]
            ins = np.flatnonzero(a < r2)
            o = ins[np.lexsort((ins, a[ins]))]
            rows[i] = (o.astype(np.int32), a[o].copy())

    chunks = [range(t, len(q), threads) for t in range(threads)]
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, chunks))
    return out_i, out_d, rows
