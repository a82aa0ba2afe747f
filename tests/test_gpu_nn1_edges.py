"""The 1-NN cascade (k_nn_grid -> k_nn1 -> k_nn_far) on EXACT ties between non-coincident reference points, and at its hand-overs.
DESIGN 4.2: "exact minimum, ties -> smallest index".  The reference cloud is a shuffled dyadic lattice, so the squared distances of
a cell centre to its 8 corners, of a face centre to its 4, of an edge midpoint to its 2 are bit-equal, and the index order says
nothing about position: "first found" and "smallest index" differ.  The model is a full scan with the library's expression
(_reg_ref.d2_exact, fp64, no FMA), argmin = the smallest index of the tied set.

Which kernel served a query is read from the library's own counters (timers on): "nn_fallback_queries" / "nn_queries" (what the grid
pass left to the octree walk) and "nn1_far" (walks k_nn1 handed to k_nn_far).  me_nn_unresolved counts something else — the owned
queries of a slab whose neighbour may lie on another rank — and is 0 here by definition; it is asserted to be."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _reg_ref import d2_exact  # noqa: E402

gpu = pytest.mark.gpu
S = 0.25
SIDE = 17
ORIGIN = np.array([8.0, -4.0, 2.0])


def brute_nn1(ref, q, chunk=2048):
    """-> (idx, d2, n_tied, lex_first): smallest index of the exactly tied minimum, the minimum, the size of the tied set, and the
    index a scan in lexicographic (x, y, z) order of the reference would have found first"""
    lex = np.lexsort((ref[:, 2], ref[:, 1], ref[:, 0]))
    idx = np.empty(len(q), np.int32)
    d2 = np.empty(len(q))
    tied = np.empty(len(q), np.int64)
    first = np.empty(len(q), np.int32)
    for c0 in range(0, len(q), chunk):
        D = d2_exact(q[c0:c0 + chunk, None, :], ref[None, :, :])
        i = np.argmin(D, axis=1)  # (argmin: the first, i.e. smallest, index of the minimum)
        m = D[np.arange(len(i)), i]
        idx[c0:c0 + chunk], d2[c0:c0 + chunk] = i, m
        tied[c0:c0 + chunk] = (D == m[:, None]).sum(1)
        first[c0:c0 + chunk] = lex[np.argmin(D[:, lex], axis=1)]
    return idx, d2, tied, first


def lattice_ref(seed=5):
    g = np.arange(SIDE)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    ijk = ijk[np.random.default_rng(seed).permutation(len(ijk))]  # index order unrelated to position
    return np.ascontiguousarray(ijk * S + ORIGIN)


def _half_points(kind, rng, n):
    """points of the lattice with `kind` half-integer coordinates: 3 cell centres (8-way tie), 2 face centres (4), 1 edge midpoints (2),
    0 the lattice points themselves (d^2 = 0); n of them at random (all when n is None)"""
    out = []
    axes = {3: [(0, 1, 2)], 2: [(0, 1), (0, 2), (1, 2)], 1: [(0,), (1,), (2,)], 0: [()]}[kind]
    for half in axes:
        rng_ax = [np.arange(SIDE - 1) + 0.5 if a in half else np.arange(SIDE) for a in range(3)]
        out.append(np.stack(np.meshgrid(*rng_ax, indexing="ij"), -1).reshape(-1, 3))
    p = np.concatenate(out)
    if n is not None and n < len(p):
        p = p[rng.choice(len(p), n, replace=False)]
    return p * S + ORIGIN


def _outside(rng, steps):
    """points `steps` lattice spacings outside the cloud, on the axes through a face centre (4-way tie among the corners of the outer
    face's cell), through an edge midpoint (2-way) and through a lattice point (a corner of the cloud among them: unique)"""
    out = []
    for axis in range(3):
        for side in (-1, 1):
            for kind in ("face", "edge", "corner"):
                for _ in range(8):
                    uv = rng.integers(0, SIDE - 1, 2).astype(np.float64)
                    if kind == "face":
                        uv += 0.5
                    elif kind == "edge":
                        uv[0] += 0.5
                    p = np.insert(uv, axis, (SIDE - 1 + steps) if side > 0 else -float(steps))
                    out.append(p)
            for cu in (0.0, SIDE - 1.0):
                for cv in (0.0, SIDE - 1.0):
                    out.append(np.insert(np.array([cu, cv]), axis, (SIDE - 1 + steps) if side > 0 else -float(steps)))
    return np.array(out) * S + ORIGIN


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(9)
    ref = lattice_ref()
    parts = {"cell": _half_points(3, rng, None), "face": _half_points(2, rng, 4000), "edge": _half_points(1, rng, 4000),
             "self": _half_points(0, rng, None), "out50": _outside(rng, 50), "out5000": _outside(rng, 5000)}
    q = np.ascontiguousarray(np.concatenate(list(parts.values())))
    part = np.concatenate([[k] * len(v) for k, v in parts.items()])
    perm = rng.permutation(len(q))
    q, part = q[perm], part[perm]
    assert len(q) <= 20_000 and len(ref) == SIDE ** 3
    return ref, q, part, brute_nn1(ref, q)


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _nn(eng, q, ref, cell):
    eng.upload(0, q, cell_size=cell)
    eng.upload(1, ref, cell_size=cell)
    eng.timers_enable(True)
    try:
        eng.timers_reset()
        idx, d2 = eng.nn1(0, 1)
        fb, tot, far = eng.timer("nn_fallback_queries")[1], eng.timer("nn_queries")[1], eng.timer("nn1_far")[1]
    finally:
        eng.timers_enable(False)
    assert tot == len(q) and eng.nn_unresolved_count(0) == 0
    return idx, d2, fb, far


def _points(eng, q):
    import torch

    return eng.nn_points(1, torch.from_numpy(q)).cpu().numpy()


def test_the_tied_sets_are_what_they_were_built_to_be(scene):
    """conditions of the case, on the model: 8 / 4 / 2-way ties, d^2 = 0 on the lattice points, and "first found" (a lexicographic
    scan) differs from "smallest index" for at least half of the tied queries"""
    ref, q, part, (idx, d2, tied, first) = scene
    assert np.all(tied[part == "cell"] == 8) and np.all(tied[part == "face"] == 4) and np.all(tied[part == "edge"] == 2)
    assert np.all(tied[part == "self"] == 1) and np.all(d2[part == "self"] == 0.0)
    for steps in ("out50", "out5000"):
        t = tied[part == steps]
        assert (t == 4).sum() >= 40 and (t == 2).sum() >= 40 and (t == 1).sum() >= 40
    t = tied > 1
    assert t.sum() > 12_000 and (first[t] != idx[t]).mean() >= 0.5, (first[t] != idx[t]).mean()


@gpu
@pytest.mark.parametrize("cell", [0.25, 0.1])
def test_ties_go_to_the_smallest_index_in_every_kernel(eng, scene, cell):
    ref, q, part, (ridx, rd2, tied, _) = scene
    idx, d2, fb, far = _nn(eng, q, ref, cell)
    assert np.array_equal(d2.view(np.uint64), rd2.view(np.uint64))                 # d^2 bit-exact
    bad = np.nonzero(idx != ridx)[0]
    assert len(bad) == 0, (len(bad), {p: int((part[bad] == p).sum()) for p in np.unique(part[bad])}, idx[bad][:8], ridx[bad][:8], tied[bad][:8])
    assert np.array_equal(_points(eng, q).view(np.uint64), rd2.view(np.uint64))    # the same queries through nn_points
    # On this lattice k_nn1 settles the outside queries within its step cap (nn1_far is printed, 0 when measured): its ties are theirs.
    # k_nn_far's own tie-breaking is put to the test where a walk must outlive the cap: the shell and the leaf-threshold tests below.
    out = np.isin(part, ("out50", "out5000"))
    oidx, od2, ofb, ofar = _nn(eng, np.ascontiguousarray(q[out]), ref, cell)
    assert np.array_equal(oidx, ridx[out]) and np.array_equal(od2.view(np.uint64), rd2[out].view(np.uint64)) and ofb == out.sum()
    print(f"\n[nn1-edges] cell={cell}: all queries: octree walk {fb} of {len(q)}, handed to k_nn_far {far}; "
          f"outside queries: octree walk {ofb} of {int(out.sum())}, handed to k_nn_far {ofar}")
    # the tied queries alone: both the grid pass and the octree walk served at least 100 of them
    t = tied > 1
    tidx, td2, tfb, _ = _nn(eng, np.ascontiguousarray(q[t]), ref, cell)
    assert np.array_equal(tidx, ridx[t]) and np.array_equal(td2.view(np.uint64), rd2[t].view(np.uint64))
    assert tfb >= 100 and t.sum() - tfb >= 100, (cell, int(t.sum()), tfb)


def sphere_shell(n2=1454, scale=1.0 / 64.0):
    """every integer vector with |v|^2 == n2, scaled by a power of two: all exactly equidistant from the origin"""
    m = int(np.sqrt(n2)) + 1
    g = np.arange(-m, m + 1)
    v2 = (g[:, None, None] ** 2 + g[None, :, None] ** 2) + g[None, None, :] ** 2
    return np.stack(np.nonzero(v2 == n2), -1).astype(np.float64) * scale - m * scale


@gpu
def test_a_query_equidistant_from_a_whole_shell_reaches_k_nn_far(eng):
    """Hundreds of reference points at ONE exact distance from the query (the integer vectors of one norm): no bound prunes any of
    them, the walk outlives k_nn1's step cap and k_nn_far has to return the smallest index of the whole shell."""
    rng = np.random.default_rng(77)
    shell = sphere_shell()
    ref = np.ascontiguousarray(shell[rng.permutation(len(shell))] + np.array([4.0, -2.0, 1.0]))
    q = np.ascontiguousarray(np.array([4.0, -2.0, 1.0]) + np.concatenate([np.zeros((1, 3)), rng.integers(-2, 3, (63, 3)) / 1024.0]))
    ridx, rd2, tied, first = brute_nn1(ref, q)
    assert tied[0] == len(ref) >= 200 and first[0] != ridx[0]
    idx, d2, fb, far = _nn(eng, q, ref, 0.0)
    assert np.array_equal(d2.view(np.uint64), rd2.view(np.uint64)) and np.array_equal(idx, ridx), (idx[:4], ridx[:4])
    assert far > 0, (fb, far)
    assert np.array_equal(_points(eng, q).view(np.uint64), rd2.view(np.uint64))


@gpu
@pytest.mark.parametrize("n_blob", [1023, 1024, 1025])
def test_far_leaf_scan_at_its_threshold(eng, n_blob):
    """k_nn_far scans a node whole when it holds <= ME_TUNE_NN_FAR_LEAF = 1024 points: a reference of one blob of 1023 / 1024 / 1025
    dyadic points — all on one sphere about the blob's centre, so that the query there is tied with every one of them and its walk
    outlives k_nn1's step cap — and a distant second blob; far queries and midpoints of blob points (exact 2-way ties)."""
    rng = np.random.default_rng(100 + n_blob)
    shell = sphere_shell(3506, 1.0 / 1024.0)  # 1248 integer vectors of one norm, |v| = 0.058: the centre is tied with all of them
    blob = shell[rng.permutation(len(shell))[:n_blob]] + np.array([3.0, 1.0, -2.0])
    other = rng.integers(-48, 49, (40, 3)) / 1024.0 + np.array([203.0, 1.0, -2.0])
    ref = np.concatenate([blob, other])
    ref = np.ascontiguousarray(ref[rng.permutation(len(ref))])
    a = rng.choice(len(ref), 600, replace=False)
    D = d2_exact(ref[a][:, None, :], ref[None, :, :])
    D[np.arange(len(a)), a] = np.inf
    mid = 0.5 * (ref[a] + ref[np.argmin(D, axis=1)])  # a point and its nearest other point; exact: the coordinates are multiples of 2^-10
    far = np.array([3.0, 1.0, -2.0]) + rng.normal(size=(200, 3)) * np.array([2000.0, 2000.0, 300.0])
    sym = np.array([3.0, 1.0, -2.0]) + np.array([[0.0, 0, 0], [5000.0, 0, 0], [0, -5000.0, 0], [0, 0, 700.0], [-64.0, 64.0, 0]])
    q = np.ascontiguousarray(np.concatenate([mid, far, sym, ref[:50]]))
    ridx, rd2, tied, _ = brute_nn1(ref, q)
    assert (tied > 1).sum() >= 20 and tied.max() == n_blob
    idx, d2, fb, nfar = _nn(eng, q, ref, 0.05)
    assert np.array_equal(d2.view(np.uint64), rd2.view(np.uint64)) and np.array_equal(idx, ridx), np.nonzero(idx != ridx)[0][:10]
    assert nfar > 0
    assert np.array_equal(_points(eng, q).view(np.uint64), rd2.view(np.uint64))


@gpu
@pytest.mark.parametrize("n_ref", [1, 17, 2049])
@pytest.mark.parametrize("n_q", [1, 63, 64, 65, 257])
def test_query_and_reference_counts(eng, n_q, n_ref):
    rng = np.random.default_rng(1000 * n_ref + n_q)
    ref = np.ascontiguousarray(rng.integers(-256, 257, (n_ref, 3)) / 64.0)
    mids = 0.5 * (ref[rng.integers(0, n_ref, n_q)] + ref[rng.integers(0, n_ref, n_q)])
    q = np.where(rng.random((n_q, 1)) < 0.5, mids, rng.uniform(-6, 6, (n_q, 3)))
    q = np.ascontiguousarray(q)
    ridx, rd2, _, _ = brute_nn1(ref, q)
    idx, d2, _, _ = _nn(eng, q, ref, 0.5)
    assert np.array_equal(d2.view(np.uint64), rd2.view(np.uint64)) and np.array_equal(idx, ridx)
    assert np.array_equal(_points(eng, q).view(np.uint64), rd2.view(np.uint64))
