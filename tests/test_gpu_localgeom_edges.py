"""me_local_geometry and me_radius_normals on the MI355X (csrc/me_localgeom.hip: local_geom_body<NORMALS>) at their exact edges,
against the exact model of tests/_localgeom_edge_cases.py.

Every cloud lies on a dyadic lattice, so the nine sums of a neighbourhood are exact in any order and the kernel's epilogue is one
fixed sequence of correctly rounded fp64 operations: eig, k, valid and the normals are compared BIT FOR BIT on every point, with no
tolerance and nobody left out.  Every cloud is uploaded in a seeded shuffled order, every call is made twice and the two results
must be byte-identical.

(1) exact ties d2 == r*r are excluded, and included at r (1 + 2^-30);  (2) min_k met exactly and missed by one;  (3) 1 .. 65537
points: around a wave, a block and the chunk of the two-level reduction (257 blocks: chunk 2, a ragged last one);  (4) the
totals: the integer rows equal the model's in every case; the fp64 rows are EXACT on a cloud of isolated clusters whose per-point
values are dyadic (sum_l3, sum_linearity, sum_planarity, sum_sphericity), and within n_valid 2^-53 sum|x| of math.fsum of the
fetched values, the worst case of any summation order, where they are not (sum_surface_variation there, all five rows elsewhere);
(5) the index reuse window r (1 + 2^-20) <= cell_h <= 1.5 r (1 + 2^-20) from both sides of both ends;  (6) queries in the border
cells of the frame, isolated points, survey-sized coordinates;  (7) me_radius_normals leaves the bytes of me_local_geometry, the
lowest-index column on equal eigenvalues, the strict viewpoint flip at dot == 0."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _localgeom_edge_cases as E  # noqa: E402
import _mme_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


_clouds, _moments, _models = {}, {}, {}


def _cloud(name):
    """a named cloud of the case file, built once (read-only)"""
    if name not in _clouds:
        kind, _, arg = name.partition(":")
        xyz = {"tie": lambda: E.tie_lattice()[0], "sheet": lambda: E.sheet(int(arg)), "clusters": E.clusters,
               "reuse": E.reuse_lattice, "border": lambda: E.border_lattice(arg.startswith("iso")), "view": E.view_sheet}[kind]()
        if arg.endswith("far"):
            xyz = xyz + E.FAR
        xyz = np.ascontiguousarray(xyz, np.float64)
        xyz.setflags(write=False)
        _clouds[name] = xyz
    return _clouds[name]


def _mom(name, r):
    if (name, r) not in _moments:
        _moments[(name, r)] = E.moments(_cloud(name), r)
    return _moments[(name, r)]


def _model(name, r, min_k):
    """(eig, k, valid) of the named cloud in ITS order, computed once and shared"""
    if (name, r, min_k) not in _models:
        _models[(name, r, min_k)] = E.model(_cloud(name), r, min_k, mom=_mom(name, r))
    return _models[(name, r, min_k)]


def _assert_bits(tag, dev, ref):
    dev, ref = np.ascontiguousarray(dev), np.ascontiguousarray(ref)
    assert dev.shape == ref.shape and dev.dtype == ref.dtype, (tag, dev.shape, ref.shape, dev.dtype, ref.dtype)
    if dev.tobytes() != ref.tobytes():
        bad = np.flatnonzero((dev.view(np.uint8).reshape(len(dev), -1) != ref.view(np.uint8).reshape(len(ref), -1)).any(1))
        pytest.fail(f"{tag}: {len(bad)} of {len(dev)} rows differ; first {bad[0]}: device {dev[bad[0]]!r} model {ref[bad[0]]!r}")


def _raw(eng, r, min_k):
    """me_local_geometry itself: the totals as the library returns them"""
    from cloud_map_evaluation_amd import _lib

    o = _lib.LocalGeomOut()
    eng._ck(eng._L.me_local_geometry(eng._ctx, 0, float(r), int(min_k), C.byref(o)))
    return {f: getattr(o, f) for f in ("n", "n_valid", "sum_k") + E.SUM_FIELDS}


def _check_totals(tag, tot, eig, k, valid, ref_tot, exact_rows=()):
    """the integer rows against the model; an fp64 row exactly where the case makes it dyadic, else against math.fsum of the
    device's own per-point values within n_valid 2^-53 sum|x|"""
    assert tot["n"] == len(k) and tot["n_valid"] == ref_tot["n_valid"] and tot["sum_k"] == ref_tot["sum_k"], (tag, tot, ref_tot)
    v = valid.astype(bool)
    f = E.features(eig[v]) if v.any() else np.zeros((0, 5))
    for c, name in enumerate(E.SUM_FIELDS):
        if name in exact_rows:
            assert tot[name] == ref_tot[name], (tag, name, tot[name], ref_tot[name])
        else:
            bound = ref_tot["n_valid"] * EPS * math.fsum(np.abs(f[:, c]))
            assert abs(tot[name] - math.fsum(f[:, c])) <= bound, (tag, name, tot[name], math.fsum(f[:, c]), bound)


def _upload(eng, name, seed, cell):
    cloud, perm = E.shuffled(_cloud(name), seed)
    eng.upload(0, cloud, cell_size=cell)
    return perm


def _geometry(eng, tag, name, perm, r, min_k, exact_rows=()):
    """local_geometry twice on the uploaded shuffle of the named cloud, against the model -> (totals, eig, k, valid), cloud order"""
    tot = _raw(eng, r, min_k)
    dev = eng.local_geometry_fetch(0)
    tot2 = _raw(eng, r, min_k)
    dev2 = eng.local_geometry_fetch(0)
    assert tot == tot2 and all(a.tobytes() == b.tobytes() for a, b in zip(dev, dev2)), f"{tag}: two runs differ"
    ref = _model(name, r, min_k)
    _assert_bits(f"{tag} k", dev[1], ref[1][perm])
    _assert_bits(f"{tag} valid", dev[2], ref[2][perm])
    _assert_bits(f"{tag} eig", dev[0], ref[0][perm])
    _check_totals(tag, tot, *dev, E.totals(*ref), exact_rows)
    return (tot, *dev)


def _normals(eng, tag, name, perm, r, min_k, before=None, viewpoint=None, invalid_z=False):
    """radius_normals twice: the per-point result it stores (against `before`, what local_geometry returned, and the model), its
    two totals, and the normals per original index against the model -> normals in the order of the named cloud"""
    info, nrm = eng.radius_normals(0, r, min_k, viewpoint=viewpoint, invalid_z=invalid_z, fetch=True)
    dev = eng.local_geometry_fetch(0)
    info2, nrm2 = eng.radius_normals(0, r, min_k, viewpoint=viewpoint, invalid_z=invalid_z, fetch=True)
    dev2 = eng.local_geometry_fetch(0)
    assert info == info2 and nrm.tobytes() == nrm2.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(dev, dev2)), tag
    ref = _model(name, r, min_k)
    for what, a, b in zip(("eig", "k", "valid"), dev, ref):
        _assert_bits(f"{tag} normals' {what}", a, b[perm])
        if before is not None:
            assert a.tobytes() == before[what].tobytes(), f"{tag}: radius_normals leaves another {what} than local_geometry"
    t = E.totals(*ref)
    assert info["n"] == len(perm) and info["n_valid"] == t["n_valid"] and info["sum_k"] == t["sum_k"], (tag, info, t)
    want = E.model_normals(_cloud(name), r, min_k, viewpoint=viewpoint, invalid_z=invalid_z, mom=_mom(name, r))
    back = np.empty_like(nrm)
    back[perm] = nrm  # cloud[i] = xyz[perm[i]]
    _assert_bits(f"{tag} normals", back, want)
    return back


# ---- (1) ties at the radius, (7) the same bytes from me_radius_normals and the lowest-index column ----------------------------------
@pytest.mark.parametrize("r", [E.TIE_R, E.TIE_R_IN], ids=["r", "r(1+2^-30)"])
def test_ties_at_the_radius(eng, r):
    """13^3 lattice of step 1/8, r = 5/8: the offsets 3-4-0 and 5-0-0 (d2 == r*r exactly) are out, at r (1 + 2^-30) they are in; k
    is the integer count of lattice offsets, clipped at the border.  The 27 interior points have three equal eigenvalues:
    linearity == planarity == 0, sphericity == 1, and the normal is (1, 0, 0), the lowest-index column of V = I."""
    xyz, ijk = E.tie_lattice()
    perm = _upload(eng, "tie", 101, r)
    tot, eig, k, valid = _geometry(eng, f"tie {r!r}", "tie", perm, r, E.TIE_MIN_K)
    assert np.array_equal(k, E.tie_counts(ijk, r > E.TIE_R)[perm])
    inner = E.tie_interior(ijk)[perm]
    e = eig[inner]
    assert inner.sum() == 27 and valid[inner].all() and np.all(e[:, 0] == e[:, 1]) and np.all(e[:, 1] == e[:, 2])
    f = E.features(e)
    assert np.all(f[:, 1] == 0.0) and np.all(f[:, 2] == 0.0) and np.all(f[:, 3] == 1.0)
    nrm = _normals(eng, f"tie {r!r}", "tie", perm, r, E.TIE_MIN_K, before={"eig": eig, "k": k, "valid": valid})
    assert np.all(nrm[E.tie_interior(ijk)] == [1.0, 0.0, 0.0])


# ---- (2) min_k met exactly and missed by one ------------------------------------------------------------------------------------------
def test_min_k_met_exactly_and_missed_by_one(eng):
    """K = the median k of the tie lattice (its border gives a spread): at min_k = K the points with k == K are valid, at K + 1 the
    same points are invalid and their rows zero.  min_k = 1 is refused."""
    from cloud_map_evaluation_amd.engine import MapEvalError

    r = E.TIE_R
    perm = _upload(eng, "tie", 102, r)
    k_ref = _model("tie", r, E.TIE_MIN_K)[1][perm]
    K = int(np.median(k_ref))
    at = k_ref == K
    assert at.any() and (k_ref < K).any() and (k_ref > K).any()
    _, eig, k, valid = _geometry(eng, "min_k = K", "tie", perm, r, K)
    assert np.array_equal(k, k_ref) and valid[at].all() and np.all(eig[at, 0] > 0.0) and not valid[k_ref < K].any()
    _, eig, k, valid = _geometry(eng, "min_k = K + 1", "tie", perm, r, K + 1)
    assert np.array_equal(k, k_ref) and not valid[at].any() and not eig[at].any() and valid[k_ref > K].all()
    with pytest.raises(MapEvalError):
        eng.local_geometry(0, r, 1)
    with pytest.raises(MapEvalError):
        eng.radius_normals(0, r, 1)


# ---- (3) sizes around a wave, a block and the reduction's chunk -----------------------------------------------------------------------
@pytest.mark.parametrize("n", E.SIZES)
def test_sizes_around_a_wave_a_block_and_the_reduction_chunk(eng, n):
    """the first n points of a three-layer sheet of step 1/16 (interior k = 30 / 22), at min_k = 2 and at min_k = 23, where the
    outer layers are invalid inside every wave.  65537 points are 257 blocks: k_row_sum runs with chunk == 2 and a ragged last
    chunk.  me_radius_normals must leave the same bytes."""
    name = f"sheet:{n}"
    perm = _upload(eng, name, 300 + n, E.SHEET_R)
    for min_k in E.SHEET_MIN_KS:
        tot, eig, k, valid = _geometry(eng, f"{name} min_k {min_k}", name, perm, E.SHEET_R, min_k)
        _normals(eng, f"{name} min_k {min_k}", name, perm, E.SHEET_R, min_k, before={"eig": eig, "k": k, "valid": valid},
                 invalid_z=min_k == 23)
    if n >= 513:
        assert 0 < tot["n_valid"] < n  # (min_k = 23: a mixture)


# ---- (4) the totals, exactly ----------------------------------------------------------------------------------------------------------
def test_totals_are_exact_on_dyadic_clusters(eng):
    """6554 isolated clusters of ten points (65540 points, 257 blocks): the two copies of each centre are valid with k = 9,
    sx = sy = sz = 0 and dyadic l1 = 2^-4 >= l2 >= l3, the outer points stay below min_k.  sum_l3, sum_linearity, sum_planarity and
    sum_sphericity are sums of multiples of 2^-12 below 1: exact in any order, so a dropped, doubled or misplaced block partial
    changes them, and they must EQUAL the model's.  sum_surface_variation (l1 + l2 + l3 is no power of two) is held to math.fsum of
    the fetched values within n_valid 2^-53 sum|x|.  The engine's means are sum / n_valid."""
    perm = _upload(eng, "clusters", 104, E.CL_R)
    tot, eig, k, valid = _geometry(eng, "clusters", "clusters", perm, E.CL_R, E.CL_MIN_K, exact_rows=E.DYADIC_ROWS)
    assert tot["n_valid"] == 2 * E.CL_COUNT and tot["sum_k"] == 18 * E.CL_COUNT
    info = eng.local_geometry(0, E.CL_R, E.CL_MIN_K)
    nv = tot["n_valid"]
    assert info["n_valid"] == nv and info["sum_k"] == tot["sum_k"] and info["mean_k"] == tot["sum_k"] / nv == 9.0
    for key, field in zip(("mpv", "linearity", "planarity", "sphericity", "surface_variation"), E.SUM_FIELDS):
        assert info[key] == tot[field] / nv, key
    _normals(eng, "clusters", "clusters", perm, E.CL_R, E.CL_MIN_K, before={"eig": eig, "k": k, "valid": valid})


# ---- (5) the index reuse window -------------------------------------------------------------------------------------------------------
def test_index_reuse_window_from_both_sides_of_both_ends(eng):
    """an index of cell_size c is kept iff r (1 + 2^-20) <= cell_h <= 1.5 r (1 + 2^-20) ("morton" timer count, as
    test_gpu_mme_edges.py counts the builds): rebuilt just above r = c, kept at r = c (cell_h == r (1 + 2^-20): the end is closed),
    just below it, at c / 1.25 and just above c / 1.5, rebuilt just below c / 1.5.  Either way the result is the model's at that r,
    and the MME at c afterwards is what it was before: the rebuild leaves the slot's requested cell size alone."""
    # (before the tight end the MME at c keeps the rebuilt, coarser grid: the same flags there, the entropies to the MME's own bound)
    c = E.REUSE_C
    eng.timers_enable(True)
    try:
        for i, (r, builds) in enumerate(E.reuse_radii(c)):
            perm = _upload(eng, "reuse", 500 + i, c)
            m0 = eng.mme(0, c, E.REUSE_MIN_K)
            eng.timers_reset()
            eng.local_geometry(0, r, E.REUSE_MIN_K)
            assert eng.timer("morton")[1] == builds, (r, builds)
            m1 = eng.mme(0, c, E.REUSE_MIN_K)
            assert m1[3] == m0[3] and m1[2].tobytes() == m0[2].tobytes()
            if r <= c:  # the MME ran on the grid of cell c again (kept, or rebuilt at c): the same bytes
                assert m1[0] == m0[0] and m1[4] == m0[4] and m1[1].tobytes() == m0[1].tobytes()
            else:  # it kept the coarser grid of cell r: other round leaders, so its leader-origin moments round differently
                np.testing.assert_allclose(m1[1], m0[1], rtol=M.RTOL, atol=M.ATOL)
            eng.upload(0, np.ascontiguousarray(_cloud("reuse")[perm]), cell_size=c)  # (the window again, from cell c)
            _geometry(eng, f"reuse r = {r!r}", "reuse", perm, r, E.REUSE_MIN_K)
            _normals(eng, f"reuse r = {r!r}", "reuse", perm, r, E.REUSE_MIN_K)
    finally:
        eng.timers_enable(False)


# ---- (6) frame borders and far coordinates --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("isolated", [False, True], ids=["lattice", "lattice+isolated"])
def test_frame_borders_isolated_points_and_far_coordinates(eng, isolated):
    """an 11^3 lattice whose faces are the cloud's bounding box: those queries sit in the border cells of the frame; with six
    isolated points 4 r beyond the faces (k == 0, invalid, zero rows), the frame's border cells hold those.  The same cloud moved by
    (2^19, -2^18, 2^6) gives the same bytes."""
    name = "border:iso" if isolated else "border:"
    out = {}
    for nm in (name, name + "far"):
        perm = _upload(eng, nm, 106, E.BORDER_R)  # the same permutation for both
        _, eig, k, valid = _geometry(eng, nm, nm, perm, E.BORDER_R, E.BORDER_MIN_K)
        nrm = _normals(eng, nm, nm, perm, E.BORDER_R, E.BORDER_MIN_K, before={"eig": eig, "k": k, "valid": valid}, invalid_z=True)
        out[nm] = (eig, k, valid, nrm)
    for a, b in zip(out[name], out[name + "far"]):
        assert a.tobytes() == b.tobytes()
    eig, k, valid, nrm = out[name]
    lone = perm >= 11 ** 3
    assert lone.sum() == (6 if isolated else 0)
    assert not k[lone].any() and not valid[lone].any() and not eig[lone].any() and valid[~lone].all()
    assert np.all(nrm[11 ** 3:] == [0.0, 0.0, 1.0])


# ---- (7) the viewpoint flip -----------------------------------------------------------------------------------------------------------
def test_viewpoint_flip_is_strict_at_dot_zero(eng):
    """a two-layer sheet z = 0, 1/16: the interior normals are exactly (0, 0, 1).  A viewpoint at the height of a layer has
    dot == 0 on that layer's interior: the normal stays; 1/16 above it points up, 1/16 below it down.  Invalid points give
    (0, 0, 0), and (0, 0, 1) with invalid_z.  Every point is compared with the model, per original index."""
    xyz = _cloud("view")
    perm = _upload(eng, "view", 107, E.VIEW_R)
    inner = E.view_interior(xyz)
    plain = _normals(eng, "view", "view", perm, E.VIEW_R, E.VIEW_MIN_K)
    assert np.all(plain[inner] == [0.0, 0.0, 1.0])
    for z0 in (0.0, 1.0 / 16):
        level = inner & (xyz[:, 2] == z0)
        for dz, want in ((0.0, 1.0), (1.0 / 16, 1.0), (-1.0 / 16, -1.0)):
            vp = (0.40625, 0.28125, z0 + dz)
            nrm = _normals(eng, f"view {vp}", "view", perm, E.VIEW_R, E.VIEW_MIN_K, viewpoint=vp)
            assert level.sum() == 64 and np.all(nrm[level] == [0.0, 0.0, want]), (vp, want)
    none = _normals(eng, "view min_k 22", "view", perm, E.VIEW_R, 22, viewpoint=(0.0, 0.0, -1.0))
    assert not none.any()
    up = _normals(eng, "view min_k 22 invalid_z", "view", perm, E.VIEW_R, 22, viewpoint=(0.0, 0.0, -1.0), invalid_z=True)
    assert np.all(up == [0.0, 0.0, 1.0])
