"""k_nn_grid's candidate stream staged 64 wide across the cell runs (csrc/me_nn.hip: wave_run_list, the chunk's head mask, groups of
eight STREAM positions translated through the run list at the end of a round) at the edges of its chunking, against a brute-force
fp64 model (tests/_reg_ref.py d2_exact, the library's own expression): d^2 bit-equal, idx equal, ties to the smallest index.  The
reference order is shuffled, so index order says nothing about position.  Coordinates are dyadic (multiples of 2^-12), so every
difference, square and sum is exact.

How a stream is pinned down without knowing the curve (as tests/test_gpu_mme_flat_stream.py does): the eight cells of one aligned
2 x 2 x 2 block are mutually adjacent.  With the reference AND the queries inside one such block every wavefront, whichever 64
queries it holds, forms one group (one round) whose box holds the block, none of its cells is culled, and the run list is the
eight cell populations in table slot order, x fastest: x + 2 y + 4 z.  The block is taken at the level the search really uses —
the finest sorted level whose occupied cells hold >= 6 points on average (me_index.hip) — which _search_level works out on the host
from the same rule; every cloud here is built so that this is two levels below the cell size handed to upload (cell edge R).

Every query sits a few quanta off a reference point, and EVERY point of the runs a case is about has such a query: whatever place
a point has inside its run, each stream position of those runs is the true neighbour of some query — the first, the middle and the
last member of a group, members of a group that straddles several runs, and the members of the stream's padded last group.

Against a vacuous pass: with timers on, nn_fallback_queries (what the grid passes left to the octree walk) is at most the number of
queries the MODEL calls unsafe — those whose third-smallest exact d^2 is within 2 rank_tol of the smallest, the only ones for which
some partition of the candidates into groups can leave b3 - b1 <= rank_tol — so the grid pass answered the rest."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _mme_ref import HAIR  # noqa: E402
from _reg_ref import d2_exact  # noqa: E402

gpu = pytest.mark.gpu

R = 0.125            # 2^-3: nominal edge of a search cell (the real edge is R * HAIR)
CELL_SIZE = 4.0 * R  # handed to upload: the search level lies two Morton levels below it
Q = 2.0 ** -12       # coordinate quantum
CHUNK = 64           # positions per staged chunk
GROUP = 8            # candidates per ranking group
MORTON_BITS, SORT_DEPTH, NN_OCC = 21, 2, 6.0  # me_internal.hpp: kMortonBits, ME_TUNE_SORT_DEPTH, ME_TUNE_NN_OCC
RANK_TOL = 1e-3 * (R * HAIR) ** 2             # k_nn_grid: rank_tol at the search level


# ---- host model ----------------------------------------------------------------------------------------------------------------------
def _search_level(ref):
    """(levels below the upload cell, cell edge) of the 1-NN grid me_index.hip builds for `ref` at CELL_SIZE: origin snapped to the cell
    lattice, depth from the extent, then the finest sorted level with >= NN_OCC points per occupied cell"""
    cell_h = CELL_SIZE * HAIR
    origin = np.floor(ref.min(0) / cell_h) * cell_h
    ncell = np.floor((ref.max(0) - origin).max() / cell_h) + 1.0
    bits = 1
    while (1 << bits) < ncell:
        bits += 1
    shift = MORTON_BITS - bits
    fine_h = np.ldexp(cell_h, -shift)
    sort_min = max(0, shift - SORT_DEPTH)
    idx_bits = max(1, int(np.ceil(np.log2(len(ref)))))
    assert 3 * (MORTON_BITS - sort_min) + idx_bits <= 64  # the packed sort keeps the full depth: no level is cut
    fine = np.floor((ref - origin) / fine_h).astype(np.int64)
    for k in range(sort_min, MORTON_BITS):
        if len(ref) / len(np.unique(fine >> k, axis=0)) >= NN_OCC:
            return shift - k, float(np.ldexp(fine_h, k)), origin
    return shift - (MORTON_BITS - 1), float(np.ldexp(fine_h, MORTON_BITS - 1)), origin


def _cells(xyz, origin=0.0):
    return np.floor((xyz - origin) / (R * HAIR)).astype(int)


def _stream_facts(counts):
    """(run lengths, chunk offset of every run's first position, stream length) of a block's stream"""
    runs = [c for c in counts if c]
    starts = np.concatenate([[0], np.cumsum(runs)[:-1]])
    return runs, [int(s) % CHUNK for s in starts], int(np.sum(runs))


def brute_nn1(ref, q, chunk=256):
    """-> (idx, d2, unsafe): smallest index of the exactly tied minimum, the minimum, and whether the third-smallest d^2 lies within
    2 RANK_TOL of it"""
    idx = np.empty(len(q), np.int32)
    d2 = np.empty(len(q))
    unsafe = np.zeros(len(q), bool)
    for c0 in range(0, len(q), chunk):
        D = d2_exact(q[c0:c0 + chunk, None, :], ref[None, :, :])
        i = np.argmin(D, axis=1)  # (argmin: the first, i.e. smallest, index of the minimum)
        idx[c0:c0 + chunk], d2[c0:c0 + chunk] = i, D[np.arange(len(i)), i]
        if D.shape[1] >= 3:
            s = np.partition(D, 2, axis=1)[:, :3]
            unsafe[c0:c0 + chunk] = s.max(1) - s.min(1) <= 2.0 * RANK_TOL
    return idx, d2, unsafe


# ---- clouds --------------------------------------------------------------------------------------------------------------------------
def _cell_points(rng, cell, n):
    """n distinct dyadic points in the inner half of search cell `cell` (edge R * HAIR, origin 0)"""
    per_axis = int(round(0.5 * R / Q))  # 256 positions per axis
    flat = rng.choice(per_axis ** 3, size=n, replace=False)
    m = np.stack([flat % per_axis, (flat // per_axis) % per_axis, flat // (per_axis * per_axis)], -1)
    return (np.asarray(cell, np.float64) + 0.25) * R + m * Q


def _block(rng, counts, corner=(0, 0, 0)):
    """one aligned 2 x 2 x 2 block of search cells; counts[x + 2 y + 4 z] points in cell corner + (x, y, z) -> (points, slot of each)"""
    pts, slot = [], []
    for s, n in enumerate(counts):
        if n:
            pts.append(_cell_points(rng, (corner[0] + (s & 1), corner[1] + ((s >> 1) & 1), corner[2] + (s >> 2)), n))
            slot.append(np.full(n, s))
    return np.concatenate(pts), np.concatenate(slot)


def _near(rng, pts):
    """one query per given point, 1 .. 4 quanta off it on each axis (exact; stays inside the point's cell)"""
    return pts + rng.integers(1, 5, pts.shape) * rng.choice([-1.0, 1.0], pts.shape) * Q


def _shuffled(rng, ref):
    return np.ascontiguousarray(ref[rng.permutation(len(ref))])


# runs of 1, 7, 8, 9, 63, 64, 65 and 128: 345 positions, one past a multiple of 8
COUNTS_A = [1, 7, 8, 9, 63, 64, 65, 128]
# the same with the last run one shorter: 344, a multiple of 8 but not of 64
COUNTS_B = [1, 7, 8, 9, 63, 64, 65, 127]
# a run of 3000; 3000 + 7 = 3007 = 46 * 64 + 63: the third run begins on a chunk's LAST position; 3200 = 50 * 64 in all
COUNTS_C = [3000, 7, 9, 1, 8, 64, 65, 46]
# ... and one past a multiple of 64
COUNTS_D = [3000, 7, 9, 1, 8, 64, 65, 47]
BLOCKS = {"a_345": COUNTS_A, "b_344": COUNTS_B, "c_3200": COUNTS_C, "d_3201": COUNTS_D}
ROUND_COUNTS = [9, 20, 7, 14, 11, 9, 13, 21]  # 104 = 64 + 40 points per block


def _block_case(name):
    counts = BLOCKS[name]
    rng = np.random.default_rng(sum(counts))
    pts, slot = _block(rng, counts)
    # a query at every point of every run but the 3000-point one, which gets 16: its points lie 0.004 apart, so most queries among
    # them have three candidates within the rank tolerance (unsafe by the model): the run is there for its length
    big = np.nonzero(np.asarray(counts)[slot] >= 1000)[0]
    pick = np.concatenate([np.nonzero(np.asarray(counts)[slot] < 1000)[0], rng.choice(big, 16, replace=False) if len(big) else big])
    q = _near(rng, pts[pick.astype(int)])
    return _shuffled(rng, pts), np.ascontiguousarray(q[rng.permutation(len(q))])


BALLAST = [(14, 1, 1), (14, 3, 1), (14, 1, 3)]


def _lattice_ref(rng):
    """ONE point at the centre of every cell of a 7 x 7 x 7 lattice — every run of every stream is one point, every group of eight
    straddles eight runs — and three crowded cells seven cells away (in nobody's box) that lift the mean occupancy to the 6 points
    the level rule asks for"""
    g = np.arange(7)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lat = (ijk + 0.5) * R
    ballast = np.concatenate([_cell_points(rng, c, 600) for c in BALLAST])
    return lat, ballast


def _lattice_case():
    rng = np.random.default_rng(343)
    lat, ballast = _lattice_ref(rng)
    mid = lambda axis: (lat + 0.5 * R * np.eye(3)[axis])[lat[:, axis] < 6.0 * R]  # noqa: E731
    inner = np.all((lat > R) & (lat < 6.0 * R), 1)
    parts = {
        "near": _near(rng, lat),                    # the true neighbour at every position of every straddling group
        "tie_x": mid(0),                            # 2-way tie, stream positions j and j + 1: one group but for one pair in eight
        "tie_y": mid(1),                            # 2-way tie, positions a row apart
        "tie_z": mid(2),                            # 2-way tie, positions a layer (>= 9) apart: always two groups
        "tie_8": lat[inner] + 0.5 * R,              # the 8 corners of a cell, spread over >= 3 groups: unsafe, exact through the octree
    }
    q = np.concatenate(list(parts.values()))
    part = np.concatenate([[k] * len(v) for k, v in parts.items()])
    perm = rng.permutation(len(q))
    return _shuffled(rng, np.concatenate([lat, ballast])), np.ascontiguousarray(q[perm]), part[perm]


def _two_rounds_case():
    """two blocks six cells apart, 104 = 64 + 40 queries in each: the queries of a block are contiguous on the curve, so the second of
    the four waves holds 40 of one block and 24 of the other, which no group can join (Chebyshev distance >= 5): two rounds"""
    rng = np.random.default_rng(104)
    a, _ = _block(rng, ROUND_COUNTS)
    b, _ = _block(rng, ROUND_COUNTS[::-1], corner=(6, 0, 0))
    ref = np.concatenate([a, b])
    return _shuffled(rng, ref), np.ascontiguousarray(_near(rng, ref)[rng.permutation(len(ref))])


def _list_pass_case():
    """block a_345 and queries 2.5 .. 3 search cells off its +x face: nothing in the 3 x 3 x 3 block of their search cell, nor in that of
    the level above; the upload cell's block (12 search cells wide) holds the reference: a list pass settles them"""
    rng = np.random.default_rng(77)
    ref, _ = _block(rng, COUNTS_A)
    k = rng.integers(0, int(0.5 * R / Q), (150, 3))
    q = np.array([4.5 * R, 0.75 * R, 0.75 * R]) + k * Q
    return _shuffled(rng, ref), np.ascontiguousarray(q)


_CASES = {}


def _case(name):
    """(ref, q, model, extra) once per process; the model is shared and never written to"""
    if name not in _CASES:
        extra = None
        if name in BLOCKS:
            ref, q = _block_case(name)
        elif name == "lattice":
            ref, q, extra = _lattice_case()
        elif name == "two_rounds":
            ref, q = _two_rounds_case()
        else:
            ref, q = _list_pass_case()
        assert len(ref) <= 4000 and len(q) <= 4000
        _CASES[name] = (ref, q, brute_nn1(ref, q), extra)
    return _CASES[name]


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _nn(eng, q, ref):
    eng.upload(0, q, cell_size=CELL_SIZE)
    eng.upload(1, ref, cell_size=CELL_SIZE)
    eng.timers_enable(True)
    try:
        eng.timers_reset()
        idx, d2 = eng.nn1(0, 1)
        fb, tot = eng.timer("nn_fallback_queries")[1], eng.timer("nn_queries")[1]
    finally:
        eng.timers_enable(False)
    assert tot == len(q)
    return idx, d2, fb


def _check(eng, name, allowed_fallback=None):
    ref, q, (ridx, rd2, unsafe), _ = _case(name)
    idx, d2, fb = _nn(eng, q, ref)
    print(f"\n[nn-flat-stream] {name}: {len(q)} queries on {len(ref)} points, octree walk {fb}, unsafe by the model {int(unsafe.sum())}")
    assert np.array_equal(d2.view(np.uint64), rd2.view(np.uint64)), (name, np.nonzero(d2 != rd2)[0][:10])
    bad = np.nonzero(idx != ridx)[0]
    assert len(bad) == 0, (name, len(bad), bad[:8], idx[bad][:8], ridx[bad][:8])
    assert fb <= (int(unsafe.sum()) if allowed_fallback is None else allowed_fallback), (name, fb, int(unsafe.sum()))


# ---- host only -----------------------------------------------------------------------------------------------------------------------
def test_constructed_streams_hold_what_they_are_built_for():
    """the level rule, the cells, the stream positions and the tie counts of the model — no GPU"""
    for name, counts in BLOCKS.items():
        ref, q, (ridx, rd2, unsafe), _ = _case(name)
        below, edge, origin = _search_level(ref)
        assert below == 2 and edge == R * HAIR and np.all(origin == 0.0), (name, below, edge)
        c = _cells(ref)
        assert c.min() == 0 and c.max() == 1 and np.array_equal(np.bincount(c @ [1, 2, 4]), counts)
        assert _cells(q).min() == 0 and _cells(q).max() == 1                       # one group, one round: the stream is pinned
        assert len(q) > 64 and unsafe.sum() <= len(q) // 10                        # the grid pass has to answer nearly all of them
        assert np.all(rd2 > 0.0) and np.all(rd2 <= 3 * (4 * Q) ** 2)
    runs, at, total = _stream_facts(COUNTS_A)
    assert runs == [1, 7, 8, 9, 63, 64, 65, 128] and total % GROUP == 1            # one past a multiple of 8
    assert 8 in [a % GROUP for a in at] or 0 in [a % GROUP for a in at]            # a run that begins a group ...
    assert any(a % GROUP and (a + r) // GROUP > a // GROUP for a, r in zip(at, runs))  # ... and groups that straddle runs
    assert _stream_facts(COUNTS_B)[2] % GROUP == 0 and _stream_facts(COUNTS_B)[2] % CHUNK != 0
    runs, at, total = _stream_facts(COUNTS_C)
    assert runs[0] == 3000 and at[2] == CHUNK - 1 and total % CHUNK == 0           # a run on a chunk's last position; whole chunks
    assert _stream_facts(COUNTS_D)[2] % CHUNK == 1                                  # one past a multiple of 64
    # the lattice: the level, one point per cell, the ballast out of every box, and the ties
    ref, q, (ridx, rd2, unsafe), part = _case("lattice")
    below, edge, origin = _search_level(ref)
    assert below == 2 and edge == R * HAIR and np.all(origin == 0.0)
    c = _cells(ref)
    lat = np.all(c < 7, 1)
    assert lat.sum() == 343 and len(np.unique(c[lat], axis=0)) == 343 and sorted(map(tuple, np.unique(c[~lat], axis=0))) == sorted(BALLAST)
    assert (c[~lat][:, 0] - 6).min() >= 6                                          # Chebyshev distance > 2 + 2 + 1 from any lattice query
    D = d2_exact(q[:, None, :], ref[None, :, :])
    tied = (D == rd2[:, None]).sum(1)
    for p, n in (("near", 1), ("tie_x", 2), ("tie_y", 2), ("tie_z", 2), ("tie_8", 8)):
        assert np.all(tied[part == p] == n), p
    assert np.array_equal(unsafe, part == "tie_8") and (part == "tie_8").sum() == 125
    assert min((part == p).sum() for p in ("tie_x", "tie_y", "tie_z")) == 294 and _cells(q).max() <= 6
    # two rounds: 104 queries per block, blocks out of each other's reach
    ref, q, (_, _, unsafe), _ = _case("two_rounds")
    assert _search_level(ref)[:2] == (2, R * HAIR)
    cq = _cells(q)[:, 0]
    assert (cq <= 1).sum() == 104 and (cq >= 6).sum() == 104 and sum(ROUND_COUNTS) == 64 + 40 and unsafe.sum() == 0
    # the list pass: out of the search level's reach (and the next level's), inside the upload cell's
    ref, q, (_, rd2, unsafe), _ = _case("list_pass")
    assert _search_level(ref)[:2] == (2, R * HAIR)
    assert np.all(np.sqrt(rd2) > 2.0 * R * HAIR) and unsafe.sum() == 0             # a 3 x 3 x 3 block reaches < 2 cell edges
    assert np.all(_cells(q)[:, 0] == 4) and np.all(_cells(q)[:, 0] // 2 - 1 > _cells(ref)[:, 0].max() // 2)
    assert np.all(np.sqrt(rd2) < 4.5 * R)                                          # closer than the faces of the upload cell's block


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_runs_at_every_chunk_and_group_position(eng, name):
    _check(eng, name)


@gpu
def test_groups_that_straddle_eight_runs_and_their_ties(eng):
    _check(eng, "lattice")


@gpu
def test_a_wave_of_two_rounds(eng):
    _check(eng, "two_rounds")


@gpu
def test_the_list_pass_serves_what_the_search_level_cannot_reach(eng):
    _check(eng, "list_pass")
