"""me_statistical_outlier, me_radius_outlier and me_outlier_select_into on the MI355X at their exact edges.  Everything is compared
with ==: avg_dist and the counts bit for bit against the O(n^2) definitions (tests/_outlier_ref.py brute_*), mean, std_dev and
threshold against the device's summation tree restated in numpy (sor_stats_device), the mask on every point, n_kept against the mask.
Every call is made twice in one context and once in a fresh one: the bytes of all three are the same.

The cases: every k = 1 .. 40 (the five TopK<KC> instantiations of both k-NN kernels and the dispatch boundaries between them), clouds
of k - 1, k and k + 1 points, sizes at wave and block edges, the size at which `per` of k_sor_partials steps up, the k-th neighbour
on both sides of the grid pass's settled rule, values equal to the threshold, all duplicates, a dense cell beside singletons; for the
radius filter exact ties at d2 == r^2 in 3-D, the index rebuild rule, small sizes; the selection byte for byte."""
import math
import struct

import numpy as np
import pytest

import _outlier_ref as R

pytestmark = pytest.mark.gpu

SHIFT = np.array([4.0e5, -3.0e5, 50.0])


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _info_bytes(info):
    return struct.pack("<3q3d", info["n_in"], info["n_kept"], info["n_fallback"], info["mean"], info["std_dev"], info["threshold"])


def _same_bytes(a, b):
    assert _info_bytes(a[0]) == _info_bytes(b[0]), (a[0], b[0])
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def _eq(a, b):  # == for two doubles, a NaN equal to a NaN (n = 1: std = 0 / 0)
    return a == b or (math.isnan(a) and math.isnan(b))


def _sor_equal(out, avg_ref, ratio):
    info, avg, keep = out
    n = len(avg_ref)
    assert avg.dtype == np.float64 and np.array_equal(avg, avg_ref), f"{np.count_nonzero(avg != avg_ref)} of {n} avg_dist differ"
    mean, std, thr = R.sor_stats_device(avg_ref, ratio)
    print(f"n={n} ratio={ratio}: {info} model ({mean!r}, {std!r}, {thr!r})")
    assert info["n_in"] == n
    assert _eq(info["mean"], mean) and _eq(info["std_dev"], std) and _eq(info["threshold"], thr)
    assert np.array_equal(keep.astype(bool), R.sor_keep(avg_ref, thr))  # every point, nothing excluded
    assert info["n_kept"] == int(keep.sum())
    assert 0 <= info["n_fallback"] <= n


def _check_sor(xyz, k, ratio=1.0, cell_size=0.0, avg_ref=None):
    """One statistical_outlier call held to the exact model, twice in one context and once in a fresh one; returns the info."""
    if avg_ref is None:
        avg_ref = R.brute_sor_avg(xyz, k)
    with _engine() as e:
        e.upload(0, xyz, cell_size=cell_size)
        a = e.statistical_outlier(0, k, ratio, fetch=True)
        b = e.statistical_outlier(0, k, ratio, fetch=True)
    with _engine() as e:
        e.upload(0, xyz, cell_size=cell_size)
        c = e.statistical_outlier(0, k, ratio, fetch=True)
    _sor_equal(a, avg_ref, ratio)
    _same_bytes(a, b)
    _same_bytes(a, c)
    return a[0]


def _ror_equal(out, counts_ref, nb):
    info, counts, keep = out
    assert counts.dtype == np.int32 and np.array_equal(counts, counts_ref), f"{np.count_nonzero(counts != counts_ref)} counts differ"
    assert np.array_equal(keep.astype(bool), counts_ref > nb)
    assert info["n_in"] == len(counts_ref) and info["n_kept"] == int(keep.sum()) and info["threshold"] == nb


def _check_ror(xyz, nb, radius, cell_size=0.0, counts_ref=None):
    if counts_ref is None:
        counts_ref = R.brute_ror_counts(xyz, radius)
    with _engine() as e:
        e.upload(0, xyz, cell_size=cell_size)
        a = e.radius_outlier(0, nb, radius, fetch=True)
        b = e.radius_outlier(0, nb, radius, fetch=True)
    with _engine() as e:
        e.upload(0, xyz, cell_size=cell_size)
        c = e.radius_outlier(0, nb, radius, fetch=True)
    _ror_equal(a, counts_ref, nb)
    _same_bytes(a, b)
    _same_bytes(a, c)
    return a


# ---- every k: the five instantiations and the boundaries 8|9, 16|17, 24|25, 32|33 ----
def _clumpy_600():
    rng = np.random.default_rng(600)
    centres = rng.random((3, 3))
    clumps = [c + 2e-3 * rng.standard_normal((66 + (j < 2), 3)) for j, c in enumerate(centres)]  # 67 + 67 + 66 = 200
    return np.concatenate([rng.random((400, 3))] + clumps)


@pytest.mark.parametrize("k", range(1, 41))
def test_sor_every_k_on_one_cloud(k):
    xyz = _clumpy_600()
    assert len(xyz) == 600
    info = _check_sor(xyz, k)
    if k == 1:
        assert info["n_kept"] == 0 and info["mean"] == 0.0  # every point's only neighbour is itself


@pytest.mark.parametrize("k", [8, 9, 16, 17, 24, 25, 32, 33, 40])
@pytest.mark.parametrize("dn", [-1, 0, 1])
def test_sor_clouds_of_about_k_points(k, dn):
    n = k + dn
    xyz = np.random.default_rng(100 * k + n).random((n, 3))
    info = _check_sor(xyz, k)
    if n < k:  # fewer points than neighbours: no lane of the grid pass can settle
        assert info["n_fallback"] == n


# ---- sizes at wave and block edges, near the origin and far from it ----
@pytest.mark.parametrize("shifted", [False, True], ids=["unit", "shifted"])
@pytest.mark.parametrize("k", [12, 28])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_sor_sizes(n, k, shifted):
    xyz = np.random.default_rng(n).random((n, 3))
    if shifted:
        xyz = xyz + SHIFT
    avg_ref = R.brute_sor_avg(xyz, k)
    for ratio in (0.5, 2.0):
        info = _check_sor(xyz, k, ratio, avg_ref=avg_ref)
    if n == 1:
        assert info["n_kept"] == 0 and math.isnan(info["threshold"])


def test_sor_where_per_steps_up():
    """n = 256 * 1024 + 1: nb = 1024 and per = 512, block 512 owns one point and blocks 513 .. 1023 none."""
    n = 256 * 1024 + 1
    assert R.sor_launch(n) == (1024, 512) and R.sor_launch(n - 1) == (1024, 256)
    xyz = np.random.default_rng(n).random((n, 3)) * (4.0, 4.0, 0.25)
    _check_sor(xyz, 12, 1.0, avg_ref=R.sor_avg(xyz, 12))


# ---- the settled rule of the grid pass, both sides ----
def _settled_cloud(c, D, k, at_face, rng):
    """A query q with k - 1 points in a clump of diameter s / 8 around it (s = min(c, D)), one point at distance D along +x and 200
    decoys on a shell at 6 D.  q lies at a cell centre, or in x 2^-10 c inside the +x face of its cell — the face position follows
    from the cloud's minimum corner as cloud_build_index derives its lattice: cell_h = c (1 + 2^-20), origin = floor(lo / cell_h) cell_h."""
    s = min(c, D)
    v = rng.standard_normal((k - 1, 3))
    clump = v / np.linalg.norm(v, axis=1)[:, None] * (rng.random((k - 1, 1)) * s / 16.0)
    v = rng.standard_normal((200, 3))
    shell = v / np.linalg.norm(v, axis=1)[:, None] * (6.0 * D)
    off = np.concatenate([np.zeros((1, 3)), clump, [[D, 0.0, 0.0]], shell])
    cell_h = c * (1.0 + 2.0 ** -20)
    q = np.full(3, 40.5) * cell_h
    if at_face:
        for _ in range(3):
            origin = np.floor((q + off).min(0) / cell_h) * cell_h
            cx = math.floor((q[0] - origin[0]) / cell_h)
            face = origin[0] + (cx + 1) * cell_h
            q[0] = face - 2.0 ** -10 * c
        origin = np.floor((q + off).min(0) / cell_h) * cell_h
        assert 0.0 < (origin[0] + (math.floor((q[0] - origin[0]) / cell_h) + 1) * cell_h) - q[0] <= 2.0 ** -9 * c
    return q + off


@pytest.mark.parametrize("at_face", [False, True], ids=["centre", "face"])
@pytest.mark.parametrize("k", [12, 28])
def test_sor_settled_rule_both_sides(k, at_face):
    """The k-th neighbour from well inside the query's 3x3x3 block to well outside it, and a hair either side of every power of two
    of the cell edge.  Every member equals brute force; over the sweep both the grid pass and the walk decide some queries."""
    c = 0.25
    rng = np.random.default_rng(31 * k + at_face)
    n_fallback = n_points = 0
    with _engine() as e, _engine() as f:
        for j in range(-6, 3):
            for hair in (1.0, 1.0 - 2.0 ** -30, 1.0 + 2.0 ** -30):
                D = c * 2.0 ** j * hair
                xyz = _settled_cloud(c, D, k, at_face, rng)
                e.upload(0, xyz, cell_size=c)
                # k: the point at D is the k-th neighbour of the clump's points; k + 1: of q as well
                for kk in (k, k + 1):
                    ref = R.brute_sor_avg(xyz, kk)
                    a = e.statistical_outlier(0, kk, 1.0, fetch=True)
                    _sor_equal(a, ref, 1.0)
                    _same_bytes(a, e.statistical_outlier(0, kk, 1.0, fetch=True))
                    n_fallback += a[0]["n_fallback"]
                    n_points += len(xyz)
        f.upload(0, xyz, cell_size=c)  # (a fresh context on the last member)
        _same_bytes(a, f.statistical_outlier(0, k + 1, 1.0, fetch=True))
    print(f"k={k} at_face={at_face}: {n_fallback} of {n_points} queries took the walk")
    assert 0 < n_fallback < n_points


# ---- equality with the threshold is a drop ----
def _pairs(n, wide=False):
    """n / 2 pairs 0.25 apart on a lattice of pitch 8.0; with wide, the first pair is 0.5 apart."""
    m = n // 2
    g = np.arange(8, dtype=np.float64) * 8.0
    base = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:m]
    other = base + (0.25, 0.0, 0.0)
    if wide:
        other[0, 0] = base[0, 0] + 0.5
    return np.stack([base, other], 1).reshape(-1, 3)


@pytest.mark.parametrize("n", [2, 64, 1000])
def test_sor_equality_with_the_threshold_drops(n):
    xyz = _pairs(n)
    for ratio in (0.5, 2.0):
        with _engine() as e:
            e.upload(0, xyz)
            info, avg, keep = e.statistical_outlier(0, 2, ratio, fetch=True)
        assert np.all(avg == 0.125)  # (0 + 0.25) / 2; every sum of these is exact in any order
        assert (info["mean"], info["std_dev"], info["threshold"]) == (0.125, 0.0, 0.125)
        assert info["n_kept"] == 0 and not keep.any()  # v < threshold is strict
        _check_sor(xyz, 2, ratio)
    # one pair 0.5 apart: its two points lie above the rest.  (With n = 2 that pair is the whole cloud, every avg is 0.25 == threshold
    # again and nothing can be kept; from n = 4 on the threshold lies above 0.125.)
    info = _check_sor(_pairs(n, wide=True), 2, 2.0)
    if n == 2:
        assert info["n_kept"] == 0 and info["threshold"] == 0.25
    else:
        assert info["n_kept"] >= 1


@pytest.mark.parametrize("k", [1, 9, 40])
def test_sor_all_duplicates(k):
    xyz = np.tile([[1.25, -2.5, 0.75]], (300, 1))
    info = _check_sor(xyz, k, 2.0, avg_ref=np.zeros(300))
    assert info["mean"] == 0.0 and info["n_kept"] == 0
    assert np.array_equal(R.brute_sor_avg(xyz, k), np.zeros(300))


@pytest.mark.parametrize("k", [16, 32])
def test_sor_dense_cell_beside_singletons(k):
    """3000 points within 1e-3 of one location: runs far longer than the 64-entry LDS tile, next to runs of one."""
    rng = np.random.default_rng(k)
    c = 0.05
    dense = np.array([0.525, 0.525, 0.525]) + (rng.random((3000, 3)) - 0.5) * (2e-3 / math.sqrt(3.0))
    cells = rng.integers(1, 4, (100, 3)) * rng.choice([-1, 1], (100, 3))  # one to three cells away along every axis
    single = np.array([0.525, 0.525, 0.525]) + (cells + (rng.random((100, 3)) - 0.5) * 0.8) * c
    xyz = np.concatenate([dense, single])[rng.permutation(3100)]
    _check_sor(xyz, k, 2.0, cell_size=c)


# ---- radius filter ----
def _lattice():
    g = np.arange(-4, 5, dtype=np.float64) * 0.125
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


@pytest.mark.parametrize("cell_size", [0.125, 0.25, 0.5, 1.0, 0.625])
def test_ror_exact_ties_in_3d(cell_size):
    """{-4 .. 4}^3 x 0.125 at r = 0.625: the offsets (3, 4, 0), (0, 3, 4), (5, 0, 0), their permutations and sign changes lie at
    d2 == r^2 exactly and are not counted.  Cell sizes 0.125 x 2^m put every point on a cell face of the upload's lattice (the call
    re-indexes at r); 0.625 keeps the resident index."""
    from cloud_map_evaluation_amd.engine import MapEvalError

    xyz, r = _lattice(), 0.625
    ref = R.brute_ror_counts(xyz, r)
    o = np.stack(np.meshgrid(*[np.arange(-5, 6)] * 3, indexing="ij"), -1).reshape(-1, 3)
    inside = o[(o * o).sum(1) < 25]  # the integer statement of the same count: strictly inside, the 30 ties at 25 excluded
    centre = np.flatnonzero((xyz == 0).all(1))[0]
    assert ref[centre] == len(inside) == ref.max() and ((o * o).sum(1) == 25).sum() == 30
    for nb in (0, int(ref.min()), int(ref.max()) - 1, int(ref.max())):
        info, counts, keep = _check_ror(xyz, nb, r, cell_size=cell_size, counts_ref=ref)
        assert info["n_kept"] == int((ref > nb).sum())
    assert info["n_kept"] == 0  # nb = counts.max(): strict >
    with _engine() as e:
        e.upload(0, xyz, cell_size=cell_size)
        assert e.radius_outlier(0, 0, r)["n_kept"] == len(xyz)
        e.radius_outlier(0, int(ref.max()), r)
        with pytest.raises(MapEvalError, match="keeps no point"):
            e.select_kept_into(0)
        assert np.array_equal(e.download(0), xyz)  # the refused selection left the cloud alone


def test_ror_index_rule_keep_or_rebuild():
    """The resident index is kept when r (1 + 2^-20) <= cell_h <= 1.5 r (1 + 2^-20) and rebuilt at r otherwise: the counts are the
    same either way, and the slot stays usable for a k-NN pass."""
    n, r = 4097, 0.0625
    xyz = np.random.default_rng(n).random((n, 3))
    ref = R.brute_ror_counts(xyz, r)
    avg_ref = R.brute_sor_avg(xyz, 12)
    x = r * (1.0 + 2.0 ** -20)
    outs = []
    for cell_size in (r, np.nextafter(x, 0.0), np.nextafter(x, np.inf), 1.5 * r, 1.6 * r, 0.5 * r):
        with _engine() as e:
            e.upload(0, xyz, cell_size=float(cell_size))
            a = e.radius_outlier(0, 3, r, fetch=True)
            _ror_equal(a, ref, 3)
            _sor_equal(e.statistical_outlier(0, 12, 1.0, fetch=True), avg_ref, 1.0)
            _same_bytes(a, e.radius_outlier(0, 3, r, fetch=True))  # (after the k-NN pass, on the index the first call left)
        outs.append(a)
    for a in outs[1:]:
        _same_bytes(outs[0], a)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ror_sizes(n):
    xyz = np.random.default_rng(n).random((n, 3)) - 0.5
    r = 0.3
    info, counts, keep = _check_ror(xyz, 2, r)
    if n == 1:
        assert counts[0] == 1 and info["n_kept"] == 0
    _check_ror(xyz + SHIFT, 2, r)


# ---- selection ----
def test_selection_in_cloud_order_byte_for_byte():
    rng = np.random.default_rng(1000)
    xyz = np.concatenate([rng.random((900, 3)), rng.random((100, 3)) * 4.0 - 1.5])[rng.permutation(1000)]
    nrm = rng.standard_normal((1000, 3))
    with _engine() as a, _engine() as b:
        a.upload(0, xyz)
        a.set_normals(0, nrm)
        info, avg, keep = a.statistical_outlier(0, 12, 1.0, fetch=True)
        _sor_equal((info, avg, keep), R.brute_sor_avg(xyz, 12), 1.0)
        sel = keep.astype(bool)
        assert 0 < sel.sum() < 1000
        assert a.select_kept_into(0, b, 1) == info["n_kept"]
        assert b.download(1).tobytes() == xyz[sel].tobytes() and b.get_normals(1).tobytes() == nrm[sel].tobytes()
        assert a.download(0).tobytes() == xyz.tobytes()  # the source is untouched, its mask still there
        assert a.select_kept_into(0) == info["n_kept"]
        assert a.download(0).tobytes() == xyz[sel].tobytes() and a.get_normals(0).tobytes() == nrm[sel].tobytes()
    with _engine() as a, _engine() as b:  # a mask that keeps every point returns the cloud unchanged
        a.upload(0, xyz)
        a.set_normals(0, nrm)
        assert a.radius_outlier(0, 0, 0.05)["n_kept"] == 1000
        assert a.select_kept_into(0, b, 0) == 1000
        assert b.download(0).tobytes() == xyz.tobytes() and b.get_normals(0).tobytes() == nrm.tobytes()
        assert a.select_kept_into(0) == 1000
        assert a.download(0).tobytes() == xyz.tobytes() and a.get_normals(0).tobytes() == nrm.tobytes()
