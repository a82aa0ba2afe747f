"""The brute-force model of the neighbour-list searches (tests/_search_ref.py) pinned on something it did not write: scipy's cKDTree
on random clouds without ties, and counted expectations on a dyadic lattice for the tie rule and the strict radius.  Also the surface:
the three entry points are bound and the engine offers them.  No GPU needed."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import _search_ref as S


def _cloud(n, seed, scale=1.0):
    return np.ascontiguousarray(np.random.default_rng(seed).random((n, 3)) * scale)


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("nq,nr,k", [(200, 300, 1), (257, 500, 20), (64, 41, 40)])
def test_knn_matches_ckdtree(nq, nr, k):
    q, ref = _cloud(nq, 1), _cloud(nr, 2)
    idx, d2 = S.knn(q, ref, k)
    dist, ti = cKDTree(ref).query(q, k=k)
    dist, ti = dist.reshape(nq, k), ti.reshape(nq, k)
    assert len(np.unique(S.dist2(q, ref))) == nq * nr  # no ties: the order is decided by the distances alone
    assert np.array_equal(idx, ti.astype(np.int32))    # the same neighbours in the same order
    assert (_ulps(d2, dist * dist) <= 4).all()         # scipy returns distances: sqrt and the square cost up to 4 ulp, not bit-equal


def test_knn_pads_when_the_reference_is_short():
    q, ref = _cloud(10, 3), _cloud(7, 4)
    idx, d2 = S.knn(q, ref, 9)
    assert (idx[:, 7:] == -1).all() and np.isinf(d2[:, 7:]).all()
    assert (np.sort(idx[:, :7], axis=1) == np.arange(7)).all() and (np.diff(d2[:, :7], axis=1) >= 0).all()


@pytest.mark.parametrize("r", [0.05, 0.2])
def test_radius_matches_ckdtree(r):
    q, ref = _cloud(300, 5), _cloud(800, 6)
    off, idx, d2 = S.radius(q, ref, r)
    # no distance within 8 ulp of r^2: scipy's <= r and the model's strict < r^2 then describe the same sets
    assert (_ulps(S.dist2(q, ref), np.full((), r * r)) > 8).all()
    ball = cKDTree(ref).query_ball_point(q, r)
    assert off[0] == 0 and off[-1] == len(idx) == len(d2) == sum(len(b) for b in ball) > 0
    for i, b in enumerate(ball):
        row = idx[off[i]:off[i + 1]]
        assert sorted(b) == sorted(row.tolist())
        assert (np.diff(d2[off[i]:off[i + 1]]) > 0).all()
        dd = np.linalg.norm(ref[row] - q[i], axis=1)
        assert (_ulps(d2[off[i]:off[i + 1]], dd * dd) <= 4).all()
    c, hi, hd = S.hybrid(q, ref, r, 5)
    assert np.array_equal(c, np.minimum(np.diff(off), 5))
    for i in range(len(q)):
        assert np.array_equal(hi[i, :c[i]], idx[off[i]:off[i] + c[i]]) and (hi[i, c[i]:] == -1).all() and np.isinf(hd[i, c[i]:]).all()


def _lattice():
    return np.array([(i / 8, j / 8, k / 8) for i in range(-6, 7) for j in range(-6, 7) for k in range(-3, 4)], np.float64)


def test_lattice_ties_and_the_strict_radius_by_hand():
    """step 1/8: every d2 is an exact multiple of 1/64.  Around the centre there are 6 points at one step, 12 at sqrt(2) steps, 8 at
    sqrt(3): inside each shell only the index decides.  Radius 5/8: the points at exactly 25/64 (3-4-0, 5-0-0 and their like) are out."""
    pts = _lattice()
    centre = int(np.flatnonzero((pts == 0).all(axis=1))[0])
    idx, d2 = S.knn(pts[centre:centre + 1], pts, 27)
    assert idx[0, 0] == centre and d2[0, 0] == 0.0
    assert np.array_equal(d2[0] * 64, [0] + [1] * 6 + [2] * 12 + [3] * 8)
    for a, b in ((1, 7), (7, 19), (19, 27)):
        assert (np.diff(idx[0, a:b]) > 0).all()  # equal distances: ascending index
    cells = [(i, j, k) for i in range(-6, 7) for j in range(-6, 7) for k in range(-3, 4)]
    strict = sum(1 for i, j, k in cells if i * i + j * j + k * k < 25)
    closed = sum(1 for i, j, k in cells if i * i + j * j + k * k <= 25)
    # on the sphere, inside the slab |k| <= 3: (+-5,0,0), (0,+-5,0) = 4; (+-3,+-4,0), (+-4,+-3,0) = 8; (+-4,0,+-3), (0,+-4,+-3) = 8
    on_sphere = [(i, j, k) for i, j, k in cells if i * i + j * j + k * k == 25]
    assert closed - strict == len(on_sphere) == 20 and (3, 4, 0) in on_sphere and (5, 0, 0) in on_sphere
    off, ridx, rd2 = S.radius(pts[centre:centre + 1], pts, 5 / 8)
    assert off[1] == strict and (rd2 < 25 / 64).all() and rd2.max() == 24 / 64


def test_duplicates_resolve_to_the_smaller_index():
    p = _cloud(50, 9)
    both = np.concatenate([p, p])
    idx, d2 = S.knn(both, both, 2)
    assert np.array_equal(idx[:, 0], np.tile(np.arange(50), 2)) and np.array_equal(idx[:, 1], np.tile(np.arange(50), 2) + 50)
    assert (d2 == 0).all()


def test_rows_bruteforce_agrees_with_the_matrix_model():
    q, ref = _cloud(40, 11), np.concatenate([_cloud(900, 12), _cloud(40, 11)[:5]])  # (five exact hits: d2 = 0)
    ki, kd, rows = S.rows_bruteforce(q, ref, 20, 0.15, threads=3)
    mi, md = S.knn(q, ref, 20)
    assert np.array_equal(ki, mi) and np.array_equal(kd.view(np.uint64), md.view(np.uint64))
    off, ri, rd = S.radius(q, ref, 0.15)
    for i, (a, b) in enumerate(rows):
        assert np.array_equal(a, ri[off[i]:off[i + 1]]) and np.array_equal(b.view(np.uint64), rd[off[i]:off[i + 1]].view(np.uint64))


def test_mask_helpers():
    q, ref = _cloud(30, 13), _cloud(60, 14)
    mask = (np.arange(30) % 3 != 0).astype(np.uint8)
    off, idx, d2 = S.radius(q, ref, 0.3)
    moff, midx, md2 = S.mask_rows_csr(off, idx, d2, mask)
    o2, i2, d22 = S.radius(q[mask != 0], ref, 0.3)
    assert np.array_equal(np.diff(moff)[mask != 0], np.diff(o2)) and (np.diff(moff)[mask == 0] == 0).all()
    assert np.array_equal(midx, i2) and np.array_equal(md2, d22)


def test_the_searches_are_exported_bound_and_offered():
    from cloud_map_evaluation_amd import _lib
    from cloud_map_evaluation_amd.engine import Engine

    L = _lib.load()
    for name in ("me_knn_search", "me_hybrid_search", "me_radius_search", "me_search_sort_tile"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.me_search_sort_tile() >= 64  # at least a wavefront's worth: the GPU tests cross it with a 3000-point blob
    for name in ("knn_search", "hybrid_search", "radius_search"):
        assert callable(getattr(Engine, name))
