"""The voxel run records the index build's gather emits (k_gather<true, 2> through vox_emit_row, me_vox_rows.hpp) — the voxel path
me_run_suite_from and every rank of the distributed step take — against the oracle's VoxelMap (voxel_calculator.cpp:21-56) at the
edges where a per-row reduction goes wrong: partial rows and 512-point block edges, rows of one run (the DPP wave sum) and of many
(segmented sums, overflow regions), points on voxel faces, floor(x / vs) where x * (1 / vs) rounds the other way, survey-sized
offsets, and the 63-bit budget of the compact sort key.

Which voxel path ran is read from the "voxel" timer of the one context that built the table, so that a silent fallback cannot pass
for a check of the fused path:
  FUSED       1 scope   k_vox_reduce over the gather's records
  STANDALONE  2 scopes  k_vox_records + k_vox_reduce (no hint, or a hint for another voxel size)
  THREE_PASS  3 scopes  k_vox_count_runs + k_vox_pass1 + (k_vox_mean, k_vox_pass2, k_vox_final): the records overflowed their
                        regions, or the compact key does not fit 63 bits (then no one-pass build is tried at all)
  4 scopes              k_vox_records ran, its records overflowed, and the three-pass build followed."""
import numpy as np
import pytest

from tests._tol import SIGMA_TOL, assert_sigma_close

pytestmark = pytest.mark.gpu

FUSED, STANDALONE, THREE_PASS = 1, 2, 3


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _build(eng, pts, vs, hint, slot=1, cell_size=0.1):
    """Upload under `hint` (the index build emits the records then), build the table -> (table, "voxel" scopes of the build).
    cell_size: the lattice of the bench's nn_radius (me_run_suite_from builds on it), whose finest sorted cells are 2.5 cm."""
    eng.set_voxel_hint(hint)
    try:
        eng.upload(slot, pts, cell_size=cell_size)
        eng.timers_enable(True)
        eng.timers_reset()
        table = eng.voxel_gaussians(slot, vs)
        scopes = eng.timer("voxel")[1]
        eng.timers_enable(False)
    finally:
        eng.set_voxel_hint(0.0)
    return table, scopes


def _exact_sigma(pts, vs, keys):
    """The stored covariance of every voxel (M2 / (n - 1)^2 for n > 10 — the post-pass's and computeVoxelEntropy's divisions —, M2
    otherwise) from a two-pass sum in extended precision."""
    k = np.floor(pts / vs).astype(np.int64)
    order = np.lexsort((k[:, 2], k[:, 1], k[:, 0]))
    k, p = k[order], pts[order].astype(np.longdouble)
    heads = np.flatnonzero(np.r_[True, (k[1:] != k[:-1]).any(1)])
    assert np.array_equal(k[heads], keys)
    cnt = np.diff(np.r_[heads, len(k)])
    mu = np.add.reduceat(p, heads, axis=0) / cnt[:, None]
    d = p - np.repeat(mu, cnt, axis=0)
    m2 = np.add.reduceat(d[:, :, None] * d[:, None, :], heads, axis=0)
    div = np.where(cnt > 10, (cnt - 1.0) ** 2, 1.0)
    return (m2 / div[:, None, None]).astype(np.float64)


def _against_the_oracle(table, pts, vs, exact_sigma=False):
    import oracle

    keys, n, mu, sig, ent = table
    ok, on, omu, osig, oent = oracle.VoxelMap(pts, vs).export()
    assert np.array_equal(keys, ok), "voxel keys differ from the oracle"
    assert np.array_equal(n, on), "voxel populations differ from the oracle"
    np.testing.assert_allclose(mu, omu, rtol=1e-9, atol=1e-12)
    # a one-point voxel: whatever the reference's order leaves in it (0 / 0 is NaN), NaN for NaN
    nan = np.isnan(osig).any(axis=(1, 2))
    assert np.array_equal(np.isnan(sig), np.isnan(osig))
    if exact_sigma:
        # far from the origin the reference's streaming Welford update on absolute coordinates loses digits (1e-8 of the matrix at
        # 10^5 m and 0.1 m voxels): the device (sums about the voxel centre) against the exact value, and no further from the
        # reference than the reference is from the exact value
        ex = _exact_sigma(pts, vs, ok)
        scale = np.maximum(np.abs(ex).max(axis=(1, 2), keepdims=True), 1e-300)
        assert np.max(np.abs(sig - ex) / scale) < SIGMA_TOL, "covariance differs from the exact value"
        assert np.max(np.abs(sig - osig) / scale) <= np.max(np.abs(osig - ex) / scale) + SIGMA_TOL
    elif (~nan).any():
        assert_sigma_close(sig[~nan], osig[~nan], SIGMA_TOL)
    big = on > 10  # the post-pass evaluates the entropy for n > 10 only (voxel_calculator.cpp:46-50), the others keep 0
    np.testing.assert_allclose(ent[big], oent[big], rtol=0, atol=1e-8)
    assert np.array_equal(ent[~big], oent[~big], equal_nan=True)
    return on


def _identical(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), "fused and standalone tables differ"


def _fused_and_standalone(eng, pts, vs, cell_size=0.1, exact_sigma=False):
    """The fused table against the oracle, and the standalone one bit for bit against it -> the oracle's populations."""
    fused, k = _build(eng, pts, vs, vs, cell_size=cell_size)
    assert k == FUSED, f"{k} voxel scopes: the gather's run records were not used"
    on = _against_the_oracle(fused, pts, vs, exact_sigma)
    plain, k = _build(eng, pts, vs, 0.0, cell_size=cell_size)
    assert k == STANDALONE, f"{k} voxel scopes"
    _identical(fused, plain)
    return on


def _scene(n, seed=3):
    from cloud_map_evaluation_amd import synth

    est, gt = synth.scan_pair(n, density=2500.0, seed=seed)
    return est.numpy(), gt.numpy()


# ---------------------------------------------------------------------------------------------------------
def test_the_hint_selects_the_fused_path_and_both_paths_agree_bit_for_bit(eng):
    _, pts = _scene(200_000)
    for vs in (3.0, 0.5):
        _fused_and_standalone(eng, pts, vs)
        # a hint for another voxel size: the records are for that size, the build makes its own
        other, k = _build(eng, pts, vs, 2.0 * vs)
        assert k == STANDALONE
        fused, _ = _build(eng, pts, vs, vs)
        _identical(fused, other)


@pytest.mark.parametrize("overlap", [True, False])
def test_a_callers_hint_survives_run_suite_from(overlap):
    """me_run_suite_from sets the hint to its own vmd_voxel_size for the call and gives the caller's back (me_suite.hip: VoxHint): an
    index built after the call emits the records for the caller's voxel size again, not the call's — on the primary context and on
    the twin.  A fresh engine: with overlap the twin is made inside the call, while the call's hint is in force."""
    from cloud_map_evaluation_amd.engine import Engine, Param

    est, gt = _scene(200_000)
    with Engine(0) as eng:
        eng.set_voxel_hint(0.5)
        one = eng.run_suite_from(est, gt, Param(icp_max_distance_=1.0, nn_radius_=0.1, vmd_voxel_size_=3.0), overlap=overlap)
        assert one.n_w_voxels > 0
        for ctx in (eng, eng.twin()):
            ctx.upload(1, gt, cell_size=0.1)
            ctx.timers_enable(True)
            ctx.timers_reset()
            table = ctx.voxel_gaussians(1, 0.5)
            assert ctx.timer("voxel")[1] == FUSED, "the caller's hint was not restored"
            ctx.timers_reset()
            ctx.voxel_gaussians(1, 3.0)  # (the call's size: nothing emitted its records)
            assert ctx.timer("voxel")[1] == STANDALONE, "the call's hint outlived the call"
            ctx.timers_enable(False)
            _against_the_oracle(table, gt, 0.5)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 511, 512, 513, 100_003])
def test_row_and_block_boundaries(eng, n):
    """Rows are 64 consecutive sorted points, a k_gather<true, 2> block holds 512: partial last rows and blocks, a cloud of one row,
    of one point (its voxel's covariance is what the reference's order makes of one point).  The points fill two voxels: a sparse
    cloud would give a row of 64 points dozens of runs, more than its overflow region holds (the three-pass build then takes over)."""
    rng = np.random.default_rng(n)
    pts = rng.uniform([-0.45, 0.05, 0.05], [0.45, 0.95, 0.95], (n, 3))  # two 1 m voxels: x < 0 and x >= 0
    on = _fused_and_standalone(eng, pts, 1.0)
    assert on.sum() == n and len(on) <= 2


def test_one_voxel_larger_than_the_cloud(eng):
    """Every row is a single run: the DPP wave sum (wave_sum_to_lane0) carries every record; full rows, and a partial last row."""
    rng = np.random.default_rng(1)
    pts = rng.uniform(0.05, 0.95, (100_003, 3)) + np.array([-4.0, 2.0, -1.0])
    on = _fused_and_standalone(eng, pts, 1.0)
    assert len(on) == 1 and on[0] == len(pts)


def test_tens_of_points_per_voxel(eng):
    """Populations of ~20 - 100 per voxel on the scanned surfaces: a row of 64 sorted points crosses several voxels — rows of 2, 3 and more runs, the further
    runs stored through the overflow regions."""
    _, pts = _scene(200_000)
    on = _fused_and_standalone(eng, pts, 0.3)
    assert 20 <= np.median(on) <= 100


def test_scattered_points_with_the_hint_take_the_three_pass_build(eng):
    """test_gpu_parity.py's scattered scene (~64 runs per row: the regions overflow) with the hint set: the gather's records are
    found too few and the three-pass build follows them — k_vox_records does not run (3 scopes; 4 without the hint)."""
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-60.0, 60.0, (150_000, 3)), rng.normal(0.0, 0.8, (60_000, 3)) + np.array([7.3, -2.1, 4.4])])
    table, k = _build(eng, pts, 1.0, 1.0, cell_size=0.0)  # (as there: the automatic cells)
    assert k == THREE_PASS, f"{k} voxel scopes"
    on = _against_the_oracle(table, pts, 1.0)
    assert on.max() > 100 and (on == 1).sum() > 10_000
    plain, k = _build(eng, pts, 1.0, 0.0, cell_size=0.0)
    assert k == 1 + THREE_PASS, f"{k} voxel scopes"
    _identical(table, plain)


def _face_cloud(vs, centre, rng, n=150_000):
    """Points on and next to voxel faces: in each third of the cloud one coordinate lies on one of ten face planes — k * vs as it
    rounds, or 1 - 4 ulps either side of it, one value per plane, preferring the faces where floor(x * (1 / vs)) names the other
    voxel — and the other two inside one voxel; as many points again fill the same voxels.  (Points on both sides of one face would alternate along a row of sorted points:
    dozens of runs, more than a row's overflow region holds, and the three-pass build would take over.)  Sorted by voxel key: the
    index build's sort keeps the input order inside its finest sorted cell."""
    k0 = np.round(np.asarray(centre, float) / vs)
    parts = []
    for d in range(3):
        ks = k0[d] + np.arange(-40, 40)
        cand = [ks * vs]  # per face: the face as k * vs rounds, then 1 - 4 ulps either side
        up, dn = cand[0].copy(), cand[0].copy()
        for _ in range(4):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
            cand += [up, dn]
        cand = np.stack(cand, 1)
        odd = np.floor(cand / vs) != np.floor(cand * (1.0 / vs))
        rows = np.concatenate([np.flatnonzero(odd.any(1))[:5], np.arange(0, 80, 8)])[:10]
        vals = np.array([cand[r, odd[r].argmax()] if odd[r].any() else cand[r, rng.integers(0, 9)] for r in rows])
        m = n // 3
        p = (k0 + 2 + 3 * d + rng.uniform(0.1, 0.9, (m, 3))) * vs
        p[:, d] = vals[rng.integers(0, len(vals), m)]
        # as many points again inside the same voxels: a voxel whose points all share one coordinate is exactly flat — there the
        # reference's Welford update leaves a zero determinant (entropy 0) and the device's two-pass sums a residue of rounding
        # (entropy ~ -35), a separate matter from the keys this test is about
        q = p.copy()
        q[:, d] = (np.floor(q[:, d] / vs) + rng.uniform(0.1, 0.9, m)) * vs
        parts += [p, q]
    pts = np.concatenate(parts)
    key = np.floor(pts / vs)
    return pts[np.lexsort((key[:, 2], key[:, 1], key[:, 0]))]


@pytest.mark.parametrize("vs", [0.1, 0.3, 0.25])
@pytest.mark.parametrize("offset", [0.0, 1.0e5])
def test_voxel_faces_and_rounding(eng, vs, offset):
    """Points on and next to the voxel faces, negative coordinates included, with a voxel size that has no exact binary form (0.1,
    0.3) and one that has (0.25); near the origin and at survey offsets (10^5 m: floor indices near 10^6, under the 2^20 limit).  The
    key is floor(x / vs) (getVoxelIndex, voxel_calculator.cpp:241-245).  With vs = 0.1 the set holds coordinates for which
    floor(x * (1 / vs)) is the neighbouring voxel — the textbook one is x = 0.3 (0.3 / 0.1 = 2.9999999999999996, 0.3 * 10 = 3.0000000000000004)."""
    rng = np.random.default_rng(int(vs * 100) + int(offset))
    centre = np.array([offset, -offset, 0.5 * offset])
    pts = _face_cloud(vs, centre, rng)
    if offset == 0.0:
        pts = np.concatenate([pts, [[0.3, 0.35, -0.3]]])
    assert (pts < np.floor(centre / vs) * vs - 2.0 * vs).any(), "negative side of the centre"
    differ = int((np.floor(pts / vs) != np.floor(pts * (1.0 / vs))).sum())
    assert np.floor(0.3 / 0.1) == 2.0 and np.floor(0.3 * (1.0 / 0.1)) == 3.0
    if vs == 0.1:
        assert differ > 10, "the set was meant to hold values where floor(x / vs) != floor(x * (1 / vs))"
    elif vs == 0.25:
        assert differ == 0  # (a power of two: the reciprocal is exact)
    on = _fused_and_standalone(eng, pts, vs, exact_sigma=True)
    assert on.sum() == len(pts)


def _corner_clusters(extent, n=100_000, seed=6):
    """Eight dense clusters at the corners of [0, extent]: the bounding box spans the extent, every row of sorted points lies in a
    few voxels."""
    rng = np.random.default_rng(seed)
    corners = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)], float) * (np.asarray(extent, float) - 1.5)
    pts = rng.uniform(0.0, 1.5, (n, 3)) + corners[rng.integers(0, 8, n)]
    pts[:8] = corners + 0.75  # (every corner occupied)
    key = np.floor(pts)
    return pts[np.lexsort((key[:, 2], key[:, 1], key[:, 0]))]  # (in voxel-key order inside the coarse sorted cells of a 40 km box)


def _bits_for(r):  # me_vox_rows.hpp vox_bits_for: the bits that hold 0 .. r
    b = 1
    while (1 << b) <= r:
        b += 1
    return b


@pytest.mark.parametrize("z_extent,fits", [(5000.0, True), (10_000.0, False)])
def test_compact_key_budget(eng, z_extent, fits):
    """vox_make_pack: the one-pass key is (compact voxel key << pos_bits) | row | lane and must fit 63 bits:
    bx + by + bz + 1 + pos_bits <= 63.  n = 100 000: pos_bits = vox_bits_for((n - 1) >> 6 = 1562) + 6 = 11 + 6 = 17.  Voxel size 1,
    x and y spanning floor indices 0 .. 39 999 (16 bits each: 2^15 <= 39 999 < 2^16); z spanning 0 .. 4 999 (13 bits:
    2^12 <= 4 999 < 2^13) -> 16 + 16 + 13 + 1 + 17 = 63: inside, fused; z spanning 0 .. 9 999 (14 bits) -> 64: declined — no
    record anywhere, the three-pass build straight away, with or without the hint."""
    n = 100_000
    pts = _corner_clusters((40_000.0, 40_000.0, z_extent), n)
    lo, hi = np.floor(pts.min(0) / 1.0).astype(np.int64), np.floor(pts.max(0) / 1.0).astype(np.int64)
    bits = [_bits_for(int(h - l)) for l, h in zip(lo, hi)]
    pos_bits = _bits_for(max(1, (n - 1) >> 6)) + 6
    assert pos_bits == 17 and bits[:2] == [16, 16] and bits[2] == (13 if fits else 14)
    assert (sum(bits) + 1 + pos_bits <= 63) == fits
    cell = 50.0  # (the octree's level table does not reach 0.1 m cells across 40 km)
    if fits:
        _fused_and_standalone(eng, pts, 1.0, cell_size=cell)
    else:
        table, k = _build(eng, pts, 1.0, 1.0, cell_size=cell)
        assert k == THREE_PASS, f"{k} voxel scopes: the fused path was meant to be declined"
        _against_the_oracle(table, pts, 1.0)
        plain, k = _build(eng, pts, 1.0, 0.0, cell_size=cell)
        assert k == THREE_PASS, f"{k} voxel scopes: the one-pass build was meant to be declined"
        _identical(table, plain)


# ---------------------------------------------------------------------------------------------------------
def _suite_against_the_oracle(eng, est, gt, P):
    """me_run_suite_from (both lanes), then its cached tables and AWD / SCS / n_w against the oracle (the map moved by
    initial_matrix_), and the sequential call: the voxel path of a hinted index build on both clouds, the same numbers."""
    import oracle

    one = eng.run_suite_from(est, gt, P, overlap=True)
    e, g = np.asarray(est.cpu() if hasattr(est, "cpu") else est), np.asarray(gt.cpu() if hasattr(gt, "cpu") else gt)
    moved = oracle.transform(e, P.initial_matrix_)
    assert np.array_equal(eng.download(0), moved)
    vs = P.vmd_voxel_size_
    eng.timers_enable(True)
    eng.timers_reset()
    tables = [eng.voxel_gaussians(s, vs) for s in (0, 1)]
    assert eng.timer("voxel")[1] == 0, "the call's voxel tables were not cached"
    _against_the_oracle(tables[0], moved, vs)
    _against_the_oracle(tables[1], g, vs)
    ov = oracle.awd_scs(oracle.VoxelMap(g, vs), oracle.VoxelMap(moved, vs))
    assert one.n_w_voxels == len(ov["rows"]) > 10
    np.testing.assert_allclose([one.awd, one.scs], [ov["awd"], ov["scs"]], rtol=1e-9)
    # the path: each cloud's table through the gather's records, as a hinted index build of the same points takes it — FUSED, or
    # (a row with more runs than its overflow region holds) the three-pass build after them; never k_vox_records (2 or 4 scopes)
    eng.timers_enable(False)
    want = sum(_build(eng, c, vs, vs)[1] for c in (moved, g))
    assert want in (2 * FUSED, FUSED + THREE_PASS, 2 * THREE_PASS)
    eng.timers_enable(True)
    eng.timers_reset()
    seq = eng.run_suite_from(est, gt, P, overlap=False)
    assert eng.timer("voxel")[1] == want, f"{eng.timer('voxel')[1]} voxel scopes, {want} expected: the gather's records were not used"
    eng.timers_enable(False)
    for k in ("full_chamfer", "mme_est", "mme_gt", "mme_est_valid", "mme_gt_valid", "awd", "scs", "n_w_voxels"):
        assert getattr(one, k) == getattr(seq, k), k
    return one


@pytest.fixture(scope="module")
def suite_pair():
    return _scene(200_000)


def _P(**kw):
    from cloud_map_evaluation_amd.engine import Param

    return Param(icp_max_distance_=1.0, nn_radius_=0.1, vmd_voxel_size_=3.0, evaluate_gt_mme_=True, **kw)


@pytest.mark.parametrize("where", ["host", "device"])
def test_suite_voxel_tables_against_the_oracle(eng, suite_pair, where):
    import torch

    est, gt = suite_pair
    if where == "device":
        dev = torch.device("cuda", 0)
        est, gt = torch.from_numpy(est).to(dev), torch.from_numpy(gt).to(dev)
    _suite_against_the_oracle(eng, est, gt, _P())


def test_suite_without_mme_against_the_oracle(eng, suite_pair):
    """evaluate_mme_ = False: the octrees are built with the index (not deferred to cloud_finish_octree)."""
    est, gt = suite_pair
    one = _suite_against_the_oracle(eng, est, gt, _P(evaluate_mme_=False))
    assert one.mme_est_valid == 0


def test_suite_with_initial_matrix_against_the_oracle(eng, suite_pair):
    """A non-identity initial_matrix_: the map is moved after its MME (map_eval.cpp:56, :1206), its index built again, and the
    records emitted again for the moved points."""
    est, gt = suite_pair
    c, s = np.cos(0.01), np.sin(0.01)
    T = np.array([[c, -s, 0, 0.03], [s, c, 0, -0.02], [0, 0, 1, 0.01], [0, 0, 0, 1.0]])
    P = _P()
    P.initial_matrix_ = T
    _suite_against_the_oracle(eng, est, gt, P)
