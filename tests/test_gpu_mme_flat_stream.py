"""k_mme3's candidate stream staged TILE wide across the cell runs (csrc/me_mme.hip: wave_run_list, the chunk's head mask, the
candidate's index carried in the tile record) at the edges of its chunking, against a brute-force fp64 numpy model.

Coordinates are dyadic (multiples of 2^-12 below 1, radius 2^-3), so every difference, square and sum of the neighbour test is exact
and the model's accepted set is THE accepted set; the three points of the band case that sit one ulp off a dyadic value go through
the library's own expression ((dx*dx + dy*dy) + dz*dz) < r*r, each operation rounded, like every other pair.

How a stream is pinned down without knowing the curve: a cell is one contiguous run of the sorted array, an aligned 2 x 2 x 2 block
of cells is contiguous too, and its eight cells are mutually adjacent.  A cloud that lives in ONE such block therefore makes every
wavefront, whichever 64 points it holds, form one group (one round) and stream all eight cells — none is culled — in table slot
order, x fastest: the stream of EVERY wave is the eight cell populations in the order x + 2 y + 4 z.  The populations are chosen so
that this stream holds the runs and chunk positions the staging has to get right (checked on the host by _stream_facts).

Per case: valid flags exact at min_k = 5, at the median k and at k_i, k_i + 1 of probe points (the smallest, the largest and a
middle neighbour count; in the band case the three queries of the pair): the count of a probe point is read through its flag
turning off between k_i and k_i + 1, and every launch compares ALL flags with (k >= min_k).  Entropies rtol 1e-8 / atol 1e-10, the
bound of the MME parity tests (tests/_mme_ref.py RTOL, ATOL; tests/_tol.py holds the covariance bounds only).

Not buildable: a round whose 7 x 7 x 7 box has ALL 343 slots non-empty.  A wave is 64 curve-consecutive points;
with every cell of the box occupied those lie in at most two face-adjacent aligned 4 x 4 x 4 blocks of cells, which span at most
four cells on two of the axes — the group's cells cannot span five on all three.  `lattice_full` (every cell of a 7 x 7 x 7 block
occupied: every slot of every wave's box inside the lattice is non-empty, the run list has no gaps) and the forced 343-slot box of
test_gpu_cell_probe (seven occupied cells) stand in for it."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mme_ref as M  # noqa: E402
from test_gpu_cell_probe import CASES as PROBE_CASES  # noqa: E402

pytestmark = pytest.mark.gpu

R = 0.125          # 2^-3: r^2 = 2^-6 exactly
Q = 2.0 ** -12     # coordinate quantum
MIN_K = 5


def _tile():
    """TILE of the product launch of k_mme3, read from the source so that the chunk positions below follow the kernel"""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cloud_map_evaluation_amd", "csrc", "me_mme.hip")
    with open(src) as f:
        m = re.search(r"ME_LAUNCH_MME3\((\d+), ME_TUNE_MME_WAVES", f.read())
    assert m, "the product launch of k_mme3"
    return int(m.group(1))


TILE = _tile()


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _cell_points(rng, cell, n):
    """n distinct dyadic points in the inner half of a cell (edge R (1 + 2^-20), origin 0: cell c spans [c R, (c + 1) R) and a hair)"""
    per_axis = int(round(0.5 * R / Q))  # 256 positions per axis
    flat = rng.choice(per_axis ** 3, size=n, replace=False)
    m = np.stack([flat % per_axis, (flat // per_axis) % per_axis, flat // (per_axis * per_axis)], -1)
    return (np.asarray(cell, np.float64) + 0.25) * R + m * Q


def _block(rng, counts, corner=(0, 0, 0)):
    """one aligned 2 x 2 x 2 block of cells; counts[x + 2 y + 4 z] points in cell corner + (x, y, z)"""
    out = []
    for s, n in enumerate(counts):
        if n:
            out.append(_cell_points(rng, (corner[0] + (s & 1), corner[1] + ((s >> 1) & 1), corner[2] + (s >> 2)), n))
    return np.concatenate(out)


def _stream_facts(counts):
    """(run lengths, chunk offset of every run's first position, stream length) of a block's stream"""
    runs = [c for c in counts if c]
    starts = np.concatenate([[0], np.cumsum(runs)[:-1]])
    return runs, [int(s) % TILE for s in starts], int(np.sum(runs))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
CHUNK_COUNTS = None
BAND_COUNTS = [30, 20, 25, 40, 17, 33, 21, 1]
ROUND_COUNTS = [1, TILE - 1, 5, 20, 11, 9, 6, 5]


def _chunk_counts():
    """runs of 1, TILE - 1, TILE, TILE + 1, 2 TILE and 3000 points, then a filler that puts the last run on the LAST position of a
    chunk, and a last run that ends the stream exactly on a chunk boundary"""
    c = [1, TILE - 1, TILE, TILE + 1, 2 * TILE, 3000]
    fill = (TILE - 1 - sum(c)) % TILE or TILE  # the seventh run: the eighth begins at chunk position TILE - 1
    c.append(fill)
    c.append(TILE + 1)  # one position to the chunk's end, then one whole chunk
    return c


def _band_cloud():
    """BAND_COUNTS, with the block's last cell (1, 1, 1) holding ONE point p — a run of one, so p is its first candidate, at a
    position that is neither the first nor the last of its chunk — and three queries whose only offset from p lies along one axis:
    qx at distance exactly r (a tie: excluded), qy one ulp of r inside, qz one ulp of r outside.  All three pairs sit deep inside
    the FP32 band, so the exact test decides them and loads p through the index in its tile record."""
    rng = np.random.default_rng(71)
    xyz = _block(rng, BAND_COUNTS[:7] + [0])
    p = np.array([1.5 * R, 1.5 * R, 1.5 * R])
    qx = p - np.array([R, 0.0, 0.0])                # cell (0, 1, 1)
    qy = p - np.array([0.0, R - 2.0 ** -56, 0.0])   # cell (1, 0, 1): dy = r - ulp, exact
    qz = p - np.array([0.0, 0.0, R + 2.0 ** -55])   # cell (1, 1, 0): dz = r + ulp, exact
    n0 = len(xyz)
    # (the three queries take the place of one random point of their cells: the populations stay BAND_COUNTS)
    keep = np.ones(n0, bool)
    edges = np.concatenate([[0], np.cumsum(BAND_COUNTS[:7])])
    for s in (6, 5, 3):
        keep[edges[s]] = False
    xyz = np.concatenate([xyz[keep], qx[None], qy[None], qz[None], p[None]])
    n = len(xyz)
    return xyz, dict(p=n - 1, qx=n - 4, qy=n - 3, qz=n - 2)


def _lattice_full():
    """every cell of a 7 x 7 x 7 block occupied (two points each; eight cells of 40): whatever box a wave forms, each of its slots
    inside the lattice is a run — full 64-slot batches in the run list, rank = lane"""
    rng = np.random.default_rng(72)
    out = []
    for z in range(7):
        for y in range(7):
            for x in range(7):
                out.append(_cell_points(rng, (x, y, z), 40 if (x % 3 == 1 and y % 3 == 1 and z % 3 == 1) else 2))
    return np.concatenate(out)


def _two_rounds():
    """two 2 x 2 x 2 blocks six cells apart, 104 = 64 + 40 points each: each block is contiguous on the curve, so the second of
    the cloud's four waves holds 40 points of one block and 24 of the other, which no group can join (Chebyshev distance >= 5):
    it needs a second round, and each of its rounds streams one block's eight runs"""
    rng = np.random.default_rng(73)
    return np.concatenate([_block(rng, ROUND_COUNTS), _block(rng, ROUND_COUNTS[::-1], corner=(6, 0, 0))])


def _build():
    global CHUNK_COUNTS
    CHUNK_COUNTS = _chunk_counts()
    band, band_info = _band_cloud()
    c = {
        "chunks": (_block(np.random.default_rng(70), CHUNK_COUNTS), R, {}),
        "band": (band, R, band_info),
        "lattice_full": (_lattice_full(), R, {}),
        "two_rounds": (_two_rounds(), R, {}),
        # the forced 7 x 7 x 7 box of test_gpu_cell_probe (343 slots, six batches; its own radius, coordinates not dyadic)
        "box_343": (np.ascontiguousarray(PROBE_CASES["box_343_plus_one"], np.float64), 0.1, {}),
    }
    return c


CASES = _build()
_MODEL = {}


def _model(name):
    """(k, cov) of a case by brute force in fp64, once per process: the accepted set from the library's own expression over ALL
    pairs, the moments from matrix products of the accept matrix with the coordinates about a dyadic centre (exact sums for the
    dyadic points), cov = (S2 - S1 S1^T / k) / (k - 1)"""
    if name not in _MODEL:
        xyz, r, _ = CASES[name]
        n = len(xyz)
        y = xyz - np.floor(xyz.mean(0) / R) * R
        feat = np.stack([y[:, 0], y[:, 1], y[:, 2], y[:, 0] * y[:, 0], y[:, 0] * y[:, 1], y[:, 0] * y[:, 2], y[:, 1] * y[:, 1],
                         y[:, 1] * y[:, 2], y[:, 2] * y[:, 2]], 1)
        k = np.zeros(n, np.int64)
        s = np.zeros((n, 9))
        for c0 in range(0, n, 512):
            d = xyz[None, :, :] - xyz[c0:c0 + 512, None, :]
            acc = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < r * r  # strict
            acc[np.arange(acc.shape[0]), c0 + np.arange(acc.shape[0])] = False  # the query itself
            k[c0:c0 + 512] = acc.sum(1)
            s[c0:c0 + 512] = acc.astype(np.float64) @ feat
        cov = np.zeros((n, 3, 3))
        ok = k >= 2
        kk = k[ok].astype(np.float64)
        for col, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            v = (s[ok, 3 + col] - s[ok, a] * s[ok, b] / kk) / (kk - 1.0)
            cov[ok, a, b] = cov[ok, b, a] = v
        _MODEL[name] = (k, cov)
    return _MODEL[name]


def _check(eng, name, min_k, entropies=False):
    xyz, r, _ = CASES[name]
    k, cov = _model(name)
    rent, rval, rnv, _ = M.entropy_of(k, cov, min_k)
    mean, ent, val, nv, s = eng.mme(0, r, min_k)
    val = val.astype(bool)
    assert np.array_equal(val, rval), (name, min_k, np.nonzero(val != rval)[0][:10], k[val != rval][:10])
    assert nv == rnv
    # (the flags ARE the counts: no determinant of these neighbourhoods is anywhere near zero)
    assert np.array_equal(rval, k >= min_k), (name, min_k)
    if entropies:
        assert np.array_equal(ent == 0.0, rent == 0.0)
        np.testing.assert_allclose(ent[rval], rent[rval], rtol=M.RTOL, atol=M.ATOL, err_msg=f"{name} min_k={min_k}")


def _probe_counts(eng, name, points):
    """the device's count of each given point equals the model's: valid at min_k = k, not at k + 1 (all other flags compared too)"""
    k, _ = _model(name)
    for i in points:
        ki = int(k[i])
        assert ki >= 2
        _check(eng, name, ki)
        _check(eng, name, ki + 1)


def _run_case(eng, name, extra_points=()):
    xyz, r, _ = CASES[name]
    assert len(xyz) <= 20_000
    eng.upload(0, np.ascontiguousarray(xyz), cell_size=r)
    k, _ = _model(name)
    _check(eng, name, MIN_K, entropies=True)
    big = np.nonzero(k >= MIN_K)[0]
    order = big[np.argsort(k[big], kind="stable")]
    _check(eng, name, int(k[order[len(order) // 2]]))
    _probe_counts(eng, name, list(extra_points) + [int(order[0]), int(order[len(order) // 2]), int(order[-1])])


def test_constructed_streams_hold_what_they_are_built_for():
    """host only: the chunk positions the populations were chosen for, at the kernel's TILE"""
    runs, at, total = _stream_facts(CHUNK_COUNTS)
    assert runs[:6] == [1, TILE - 1, TILE, TILE + 1, 2 * TILE, 3000]
    assert at[2] == 0 and at[7] == TILE - 1          # a run that begins a chunk, and one on a chunk's last position
    assert total % TILE == 0                         # the stream ends exactly on a chunk boundary
    assert sum(len(c[0]) for c in CASES.values()) <= 20_000
    runs, at, total = _stream_facts(BAND_COUNTS)
    assert runs[7] == 1 and 0 < at[7] < TILE - 1     # p: a run of one, first candidate of a run that begins mid-chunk
    xyz, r, info = CASES["band"]
    p = xyz[info["p"]]
    cell = np.floor(xyz / (R * M.HAIR)).astype(int)
    assert [tuple(cell[info[q]]) for q in ("qx", "qy", "qz", "p")] == [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)]
    assert np.sum(np.all(cell == 1, 1)) == 1 and np.array_equal(np.bincount(cell @ [1, 2, 4]), BAND_COUNTS)
    d2 = [float(((xyz[info[q]] - p) ** 2).sum()) for q in ("qx", "qy", "qz")]
    assert d2[0] == r * r
    assert d2[1] < r * r < d2[2] and abs(d2[1] - r * r) < 2.0 ** -56 and abs(d2[2] - r * r) < 2.0 ** -56
    k, _ = _model("band")
    assert min(k[info[q]] for q in ("qx", "qy", "qz")) >= MIN_K
    runs, at, total = _stream_facts(ROUND_COUNTS)
    assert sum(ROUND_COUNTS) == 64 + 40 and total > 2 * TILE


def test_runs_at_every_chunk_position(eng):
    _run_case(eng, "chunks")


def test_band_pair_reads_its_index_from_the_tile_record(eng):
    xyz, r, info = CASES["band"]
    _run_case(eng, "band", extra_points=[info["qx"], info["qy"], info["qz"]])
    # the three decisions themselves: only qy holds p inside its radius
    k, _ = _model("band")
    pi = info["p"]
    d = xyz[pi][None, :] - xyz[[info["qx"], info["qy"], info["qz"]]]
    acc = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r * r
    assert list(acc) == [False, True, False]


def test_every_slot_of_the_box_is_a_run(eng):
    _run_case(eng, "lattice_full")


def test_a_wave_of_two_rounds(eng):
    _run_case(eng, "two_rounds")


def test_the_forced_343_slot_box(eng):
    _run_case(eng, "box_343")
