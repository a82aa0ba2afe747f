"""The per-round cell table of k_mme3 and k_nn_grid (wave_group_table with the 16-byte cell records, GridView::hent) at the edges of
its probe: MME validity / entropies and 1-NN index / squared distance against the oracle, compared exactly as test_gpu_parity.py
compares them (validity, index and d^2 bit-exact, entropies rtol 1e-8 / atol 1e-10), on clouds built to reach one edge each.

Every case is both the MME's cloud (radius R, cells of edge R) and the 1-NN reference of a jittered copy of itself and of a query
cloud that also lies outside it.  Clouds have at most a few thousand points: the oracle is brute force."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
R = 0.1
MIN_K = 5


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _rng(seed):
    return np.random.default_rng(seed)


def _box(n, lo, hi, seed):
    return _rng(seed).uniform(lo, hi, size=(n, 3))


def _spread21(x):
    x = x.astype(np.uint64) & np.uint64(0x1FFFFF)
    for sh, m in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(sh))) & np.uint64(m)
    return x


def _cell_key(ijk):
    """key of a cell in the hash table: its Morton code (me_internal.hpp, wave_group_table)"""
    return _spread21(ijk[:, 0]) | (_spread21(ijk[:, 1]) << np.uint64(1)) | (_spread21(ijk[:, 2]) << np.uint64(2))


def _hash_u64(k):
    """hash_u64 of me_internal.hpp on uint64 arrays (wrapping multiplies)"""
    k = k.astype(np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xFF51AFD7ED558CCD)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xC4CEB9FE1A85EC53)
        k ^= k >> np.uint64(33)
    return k


WRAP_CELLS, WRAP_SLOTS, WRAP_TAIL = 4090, 8192, 4


def _wrap_cells():
    ijk = np.stack(np.meshgrid(*[np.arange(32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    home = (_hash_u64(_cell_key(ijk)) & np.uint64(WRAP_SLOTS - 1)).astype(np.int64)
    tail = np.nonzero((home >= WRAP_SLOTS - WRAP_TAIL) & (ijk.sum(1) > 0))[0]
    assert len(tail) > WRAP_TAIL  # more keys than the last slots hold
    rest = np.setdiff1d(np.arange(1, len(ijk)), tail)
    rest = _rng(12).permutation(rest)[:WRAP_CELLS - 1 - len(tail)]
    return np.concatenate([ijk[:1], ijk[tail], ijk[rest]])  # (cell 0: the anchor)


def _wrap_cloud():
    ijk = _wrap_cells()
    xyz = (ijk + 0.5 + _rng(13).uniform(-0.2, 0.2, size=ijk.shape)) * R
    xyz[0] = 0.0
    return xyz


def _cases():
    c = {}
    # fewer points than a wavefront, exactly one, one more (the second wave holds a single lane)
    c["n_17"] = _box(17, 0.0, 0.25, 1)
    c["n_64"] = _box(64, 0.0, 0.3, 2)
    c["n_65"] = _box(65, 0.0, 0.3, 3)
    # points in the first and the last cell of the lattice on every axis: the round's box is clipped at 0 and at cell_lim
    # (the bounding box's corners are the lattice's; a slab of points along each face, and the eight corners themselves)
    faces = [_box(1500, 0.0, 1.6, 4)]
    for ax in range(3):
        for side in (0.0, 1.6):
            f = _box(250, 0.0, 1.6, 5 + 2 * ax + int(side > 0))
            f[:, ax] = side + (0.02 * _rng(20 + ax).uniform(size=250) if side == 0.0 else -0.02 * _rng(30 + ax).uniform(size=250))
            faces.append(f)
    corners = np.array([[x, y, z] for x in (0.0, 1.6) for y in (0.0, 1.6) for z in (0.0, 1.6)])
    c["lattice_faces"] = np.concatenate(faces + [corners])
    # a wave whose group fills the 7 x 7 x 7 box (343 slots, six batches of 64, the last one of 23).  Guaranteed, not hoped for: ONE
    # wave of 64 points, 58 of them in cell (2, 2, 2) and one in each of the cells 0 and 4 along every axis.  A cell is one run of the
    # curve, so the run of 58 holds the wave's middle rank whatever the curve does: the leader sits in (2, 2, 2), every lane is within
    # Chebyshev distance 2 of it, the group's cells span 0 .. 4 per axis and the box grown by one is 7 x 7 x 7, its low faces outside
    # the lattice (the low extremes define the cloud's origin).  With 65 points a second wave holds one lane.
    mid = 2.5 * R + _rng(6).uniform(-0.3 * R, 0.3 * R, size=(58, 3))
    ext = np.full((6, 3), 2.5 * R)
    for ax in range(3):
        ext[2 * ax, ax], ext[2 * ax + 1, ax] = 0.0, 4.5 * R
    c["box_343"] = np.concatenate([mid, ext])
    c["box_343_plus_one"] = np.concatenate([mid, ext, mid[:1] + 0.01 * R])
    # the same spread over many waves: about half a point per cell
    c["sparse_5x5x5"] = _box(700, 0.0, 1.1, 6)
    # waves of three and more rounds: two far-apart clusters whose points alternate along the curve cannot share a group, and
    # a thin diagonal rod crosses more than five cells within 64 points
    t = _rng(7).uniform(size=(900, 1))
    rod = t * np.array([[3.0, 2.9, 3.1]]) + 0.004 * _rng(8).normal(size=(900, 3))
    c["rod_many_rounds"] = rod
    blobs = [np.array(o) + 0.03 * _rng(9 + i).normal(size=(40, 3)) for i, o in enumerate(
        [(0, 0, 0), (0.62, 0, 0), (0, 0.63, 0), (0.61, 0.64, 0), (0, 0, 0.66), (0.6, 0, 0.65), (0, 0.67, 0.6), (0.65, 0.6, 0.62)])]
    c["blobs_interleaved"] = np.concatenate(blobs)
    # isolated points: the 27-cell block of each holds nothing but the point itself
    g = np.stack(np.meshgrid(*[np.arange(6) * 0.45] * 3, indexing="ij"), -1).reshape(-1, 3)
    c["isolated"] = g + 0.01 * _rng(10).uniform(size=g.shape)
    # duplicates: every point three times, and a cell of 300 identical points.  Dense enough (about 130 distinct positions in a ball,
    # 16 in a corner's octant) that no neighbourhood consists of three distinct positions or fewer: such a covariance is singular, its
    # determinant rounding noise of either sign on both sides, and the valid flag not comparable (test_gpu_mme_edges._check_k)
    d = _box(2000, 0.0, 0.4, 11)
    c["duplicates"] = np.concatenate([d, d, d, np.tile(d[:1], (300, 1))])
    # a probe that wraps around the end of the table: 4090 occupied cells (one point each) give a table of 8192 slots; the cells are
    # CHOSEN on the host, from a 32 x 32 x 32 lattice, so that more keys have their home in the last four slots than those hold: linear
    # probing then runs past slot 8191 into slot 0 whatever the order of the inserts.  An anchor point at the origin pins the cloud's
    # frame, a point sits at (i + 0.5 +- 0.2) cell edges: cell i for any edge within 1.5 % of R.
    c["half_full_table"] = _wrap_cloud()
    return c


CASES = _cases()


def _check_mme(eng, xyz):
    mean, ent, val, nv, s = eng.mme(0, R, MIN_K)
    omean, oent, oval, onv, osum = oracle.mme(xyz, R, MIN_K)
    assert nv == onv and np.array_equal(val, oval)  # bit-exact validity
    np.testing.assert_allclose(ent, oent, rtol=1e-8, atol=1e-10)
    return nv


def _check_nn(eng, ref, q):
    eng.upload(1, q, cell_size=R)
    idx, d2 = eng.nn1(1, 0)
    oi, od2 = oracle.nn1(ref, q)
    assert np.array_equal(d2, od2)  # bit-exact squared distances
    assert np.array_equal(idx, oi)  # same neighbour (ties -> smallest index in both)


@pytest.mark.parametrize("name", sorted(CASES))
def test_mme_and_nn_at_the_probe_edge(eng, name):
    xyz = np.ascontiguousarray(CASES[name], np.float64)
    eng.upload(0, xyz, cell_size=R)
    _check_mme(eng, xyz)
    lo, hi = xyz.min(0), xyz.max(0)
    jit = xyz + 0.3 * R * _rng(100).normal(size=xyz.shape)  # (some leave the bounding box: no cell of the reference's grid)
    wide = _rng(101).uniform(lo - 2 * R, hi + 2 * R, size=(max(64, min(len(xyz), 1500)), 3))
    _check_nn(eng, xyz, np.ascontiguousarray(np.concatenate([jit, wide, xyz[:65]])))


# ---- the 16-byte table against hkeys / hvals / cell_start, entry for entry -------------------------------------------------------
EMPTY64, EMPTY32 = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint32(0xFFFFFFFF)


def _table_agrees(eng, slot, which):
    """every slot of the 16-byte table equals what hkeys[s] -> hvals[s] -> cell_start[ci], cell_start[ci + 1] give; an empty slot is all
    ones; every cell has exactly one record -> (occupied slot indices, their home slots, cell_start)"""
    hkeys, hvals, cs, ent = eng.cell_table(slot, which)
    n_slots, n_cells = len(hkeys), len(cs) - 1
    assert n_slots >= 64 and n_slots & (n_slots - 1) == 0 and n_slots >= 2 * n_cells
    assert np.array_equal(ent["key"], hkeys)
    occ = hkeys != EMPTY64
    assert int(occ.sum()) == n_cells
    assert np.all(ent["start"][~occ] == EMPTY32) and np.all(ent["count"][~occ] == EMPTY32)
    ci = hvals[occ].astype(np.int64)
    assert np.array_equal(np.sort(ci), np.arange(n_cells))  # one slot per cell
    assert np.array_equal(ent["start"][occ], cs[ci])
    assert np.array_equal(ent["count"][occ], cs[ci + 1] - cs[ci])
    assert cs[0] == 0 and np.all(np.diff(cs.astype(np.int64)) > 0)
    home = (_hash_u64(hkeys[occ]) & np.uint64(n_slots - 1)).astype(np.int64)
    return np.nonzero(occ)[0], home, cs.astype(np.int64)


def _long_cells_cloud():
    """19 900 points: a uniform part (cells of ~25 points: some cell straddles most multiples of 512, the points of one wave of the
    table's fill, and of 2048, those of one block), one cell of 700 points (longer than a wave's 512) and one of 3 000 (longer than a
    block's 2048, so that a wave whose last cell it is searches past a whole block for its end)"""
    u = _box(16_200, 0.0, 0.95, 40)
    a = np.array([0.35, 0.35, 0.35]) + 0.2 * R * _rng(41).uniform(size=(700, 3))
    b = np.array([0.65, 0.55, 0.45]) + 0.2 * R * _rng(42).uniform(size=(3000, 3))
    return np.ascontiguousarray(np.concatenate([u, a, b]))


def _straddles(cs, step):
    """some cell holds points on both sides of a multiple of `step`"""
    inner = np.arange(step, cs[-1], step)
    return bool(np.any(~np.isin(inner, cs)))


@pytest.mark.parametrize("which", [0, 1], ids=["radius_grid", "nn_grid"])
def test_cell_records_agree_with_the_three_arrays(eng, which):
    xyz = _long_cells_cloud()
    assert len(xyz) <= 20_000
    eng.upload(0, xyz, cell_size=R)
    _, _, cs = _table_agrees(eng, 0, which)
    assert cs[-1] == len(xyz)
    counts = np.diff(cs)
    assert _straddles(cs, 512) and _straddles(cs, 2048)  # cells across the fill's wave and block boundaries
    if which == 0:
        assert counts.max() >= 3000 and np.sum(counts > 512) >= 2  # the two long cells, one beyond a block
    for name in ("n_17", "n_65", "duplicates", "lattice_faces"):  # a table of the minimum size, one cell of 300 equal points, ...
        eng.upload(0, np.ascontiguousarray(CASES[name]), cell_size=R)
        _table_agrees(eng, 0, which)


def test_a_probe_wraps_around_the_end_of_the_table(eng):
    """half_full_table, radius grid: some record lies in a slot BELOW its key's home slot, i.e. its insertion ran past the last slot into
    the first, and so does every probe for that cell; the case's MME parity (above) covers the wrapped probe of k_mme3, its 1-NN parity
    that of the list passes of k_nn_grid, which end on the radius grid"""
    xyz = np.ascontiguousarray(CASES["half_full_table"])
    eng.upload(0, xyz, cell_size=R)
    hkeys = eng.cell_table(0, 0)[0]
    assert len(hkeys) == WRAP_SLOTS and np.array_equal(np.sort(hkeys[hkeys != EMPTY64]), np.sort(_cell_key(_wrap_cells())))  # the cells meant
    slots, home, _ = _table_agrees(eng, 0, 0)
    assert int(np.sum(slots < home)) >= 1
    _table_agrees(eng, 0, 1)


def test_reindex_on_one_engine_never_serves_a_stale_table(eng):
    """the same slot: cloud A, cloud B (other size, other cells, other table size), A again — results of each upload equal the
    oracle's for THAT cloud and A's two passes are bit-identical"""
    a = np.ascontiguousarray(CASES["lattice_faces"])
    b = np.ascontiguousarray(CASES["duplicates"] + 0.37)
    q = _box(700, -0.1, 1.7, 13)
    first = None
    for xyz in (a, b, a):
        eng.upload(0, xyz, cell_size=R)
        for which in (0, 1):
            assert _table_agrees(eng, 0, which)[2][-1] == len(xyz)
        _check_mme(eng, xyz)
        res = eng.mme(0, R, MIN_K)
        _check_nn(eng, xyz, q)
        if xyz is a:
            if first is None:
                first = res
            else:
                assert np.array_equal(first[1].view(np.uint64), res[1].view(np.uint64)) and np.array_equal(first[2], res[2])
