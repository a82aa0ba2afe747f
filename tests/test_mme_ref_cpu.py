"""tests/_mme_ref.py judged on the CPU, before a GPU sees any of it: on every constructed input of test_gpu_mme_edges.py the
brute-force model is held against the oracle (oracle.mme, the serial and the parallel loop) and against np_mme of
test_oracle_metrics.py — valid flags and counts equal, entropies within the project's bound (rtol 1e-8, atol 1e-10) — and the
properties the inputs were built to have (exact ties, a populated band, many rounds per wave, k ranges, grid shifts) are asserted
on the model alone.  Each case prints its tie count, band population, rounds per wave and the largest disagreement between the
CPU references (DESIGN 4.3.1 quotes them)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mme_ref as R  # noqa: E402
from test_oracle_metrics import np_mme  # noqa: E402

def _worst(ent, ref, valid):
    """largest |ent - ref| over the valid points, in units of the bound atol + rtol |ref|"""
    if not valid.any():
        return 0.0, 0.0
    err = np.abs(ent[valid] - ref[valid])
    return float(err.max()), float((err / (R.ATOL + R.RTOL * np.abs(ref[valid]))).max())


def _hold_to_the_references(label, xyz, r, min_k, k, cov, cell_h):
    """the model at (xyz, r, min_k) against the oracle's two loops, np_mme and the k-d tree's radius count; prints the case's figures"""
    import oracle

    ent, valid, nv, s = R.entropy_of(k, cov, min_k)
    assert np.array_equal(k, oracle.radius_count(xyz, xyz, r).astype(np.int64) - 1)  # the accepted set, counted by the k-d tree
    worst = (0.0, 0.0)
    for what, (oent, oval) in (("oracle serial", oracle.mme(xyz, r, min_k, mode=0)[1:3]), ("oracle parallel", oracle.mme(xyz, r, min_k, mode=2)[1:3]),
                               ("np_mme", np_mme(xyz, r, min_k))):
        oval = np.asarray(oval).astype(bool)
        assert np.array_equal(valid, oval), (label, what, int(valid.sum()), int(oval.sum()))
        assert np.array_equal(ent == 0.0, oent == 0.0), (label, what)
        np.testing.assert_allclose(oent[valid], ent[valid], rtol=R.RTOL, atol=R.ATOL, err_msg=f"{label} {what}")
        worst = max(worst, _worst(oent, ent, valid), key=lambda t: t[1])
    assert nv == int(valid.sum()) and np.all(ent[~valid] == 0.0)
    # no neighbourhood the case validates is thin enough for k_mme_refine (twice the threshold is far outside its rounding)
    margin = R.thin_margin(k, cov, cell_h, min_k)
    assert margin > 2.0, (label, margin)
    bi, bj, bacc, btie = R.band(xyz, r, cell_h)
    rounds = R.rounds_per_wave(xyz, cell_h / R.HAIR)
    print(f"\n[mme-ref] {label}: n={len(xyz)} r={r:.6g} min_k={min_k} k={k.min()}..{k.max()} valid={nv} ties={int(btie.sum())} "
          f"band={len(bi)} (accepted {int(bacc.sum())}) rounds/wave median={np.median(rounds):.0f} max={rounds.max()} "
          f"thin margin={margin:.3g} cpu refs differ by {worst[0]:.2e} ({worst[1]:.2e} of the bound)")


@pytest.mark.parametrize("name", list(R.CASES))
def test_model_against_the_oracle_and_numpy(name):
    xyz, r, min_k, _ = R.case(name)
    _hold_to_the_references(name, xyz, r, min_k, *R.case_moments(name), R.grid(xyz, r)[0])


@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("c", R.REUSE_CELLS)
@pytest.mark.parametrize("name", list(R.REUSE_MIN_K))
def test_model_against_the_oracle_and_numpy_at_the_reuse_radii(name, c, i):
    """(d) the two clouds at every radius mme_run is asked for on an index of cell c; band, rounds and thinness on THAT grid"""
    xyz, r = R.case(name)[0], R.reuse_radii(c)[i]
    k, cov = R.case_moments(name, r)
    assert (k >= R.REUSE_MIN_K[name]).mean() > 0.3
    _hold_to_the_references(f"{name} cell={c} r={r:.6g}", xyz, r, R.REUSE_MIN_K[name], k, cov, c * R.HAIR)
    if i == 4:  # (the radius that forces a rebuild is then served on its own grid)
        assert R.thin_margin(k, cov, r * R.HAIR, R.REUSE_MIN_K[name]) > 2.0


@pytest.mark.parametrize("steps,inside,on", [(2, 26, 6), (3, 92, 30)])
def test_lattice_ties_are_exact_and_excluded(steps, inside, on):
    """(a) r = 2 s: 26 neighbours inside, the 6 at d^2 == r^2 out; r = 3 s: 92 and the 30 of (3,0,0), (2,2,1).  r (1 + 2^-30)
    takes them in.  The counts come from the model; the lattice arithmetic only says what they must be."""
    assert R.lattice_counts(steps) == (inside, on)
    strict, incl = f"lattice_r{steps}", f"lattice_r{steps}_ties_in"
    xyz, r, min_k, info = R.case(strict)
    A = R.accepted(xyz, r)
    k = R.case_moments(strict)[0]
    assert np.array_equal(A.sum(1), k) and np.array_equal(A, A.T)
    it = info["interior"]
    assert it.sum() == 7 ** 3 and np.all(k[it] == inside) and min_k == inside and np.all(k[~it] <= inside)
    bi, bj, bacc, btie = R.band(xyz, r, R.grid(xyz, r)[0])
    assert not bacc.any() and btie.all()                      # every band pair of the lattice is an exact tie, none accepted
    assert np.all(np.bincount(bi, minlength=len(xyz))[it] == on)
    assert R.entropy_of(k, R.case_moments(strict)[1], inside + 1)[2] == 0   # min_k = k_interior + 1 validates nothing at all
    assert np.all(R.entropy_of(k, R.case_moments(strict)[1], inside)[1] == (k == inside)) and np.all((k == inside)[it])
    xyz2, r2, min_k2, _ = R.case(incl)
    k2 = R.case_moments(incl)[0]
    assert r2 > r and np.array_equal(xyz, xyz2) and np.all(k2[it] == inside + on) and min_k2 == inside + on
    assert k2.max() <= 128  # the min_k sweep of the device test reaches every k


@pytest.mark.parametrize("name", ["probes_k5", "probes_k10", "rounds_k5", "rounds_k10"])
def test_probe_clusters_populate_the_band_with_both_outcomes(name):
    """(b) >= 1000 (query, candidate) pairs in the band; for every |delta| both outcomes; no accidental d^2 == r^2; the query's valid
    flag IS the band decision; clusters >= 6 r apart."""
    xyz, r, min_k, info = R.case(name)
    k, cov = R.case_moments(name)
    ent, valid, _, _ = R.entropy_of(k, cov, min_k)
    q, sh, delta, lab = info["query"], info["shell"], info["delta"], info["label"]
    d2 = R.d2_lib(xyz[q], xyz[sh])
    assert not np.any(d2 == r * r)
    acc = d2 < r * r
    assert np.array_equal(k[q], (min_k - 1) + acc) and np.array_equal(valid[q], acc)
    for a in np.unique(np.abs(delta)):
        out = acc[np.abs(delta) == a]
        assert out.any() and not out.all(), a
        assert np.array_equal(out, delta[np.abs(delta) == a] < 0) or a < 2.0 ** -35  # (below ~1e-11 the rounding of the shell point decides)
    bi, bj, bacc, btie = R.band(xyz, r, R.grid(xyz, r)[0])
    assert len(bi) >= 1000 and not btie.any() and 0.3 < bacc.mean() < 0.7
    assert k.max() <= 128
    # isolation: no pair of different clusters within 6 r (brute force over the cluster centres' lattice sites is the construction;
    # here it is checked on the points)
    for rows, cols, acc in R._row_chunks(xyz, 6.0 * r):
        assert not (acc & (lab[rows][:, None] != lab[cols][None, :])).any()


@pytest.mark.parametrize("name", ["probes_k5", "probes_k10", "rounds_k5", "rounds_k10", "blob_between_sparse"])
def test_many_rounds_per_wave(name):
    """(c) median distinct clusters per 64 Morton-consecutive points >= 5 (clusters are > 2 cells apart, so each is a round of its
    own); the blob's run lies strictly inside the sorted order."""
    xyz, r, _, info = R.case(name)
    per_wave = R.clusters_per_wave(xyz, r, info["label"])
    rounds = R.rounds_per_wave(xyz, r)
    if name == "blob_between_sparse":
        order = R.morton_order(xyz, r)
        pos = np.nonzero(info["label"][order] == info["blob"])[0]
        assert pos.min() >= 64 and pos.max() < len(xyz) - 64 and pos.max() - pos.min() + 1 == len(pos) >= 2048
        assert rounds[pos.min() // 64] >= 2 and rounds[pos.max() // 64] >= 2 and rounds.max() >= 5
        w = np.arange(len(rounds))
        sparse = (w < pos.min() // 64) | (w > pos.max() // 64)
        assert np.median(per_wave[sparse]) >= 5
    else:
        assert np.median(per_wave) >= 5 and np.median(rounds) >= 5
    print(f"\n[mme-ref] {name}: clusters per wave median {np.median(per_wave):.0f}, rounds per wave median {np.median(rounds):.0f} max {rounds.max()}")


@pytest.mark.parametrize("n", R.SIZES)
def test_ball_sizes_have_k_equal_n_minus_1(n):
    """(e) every pair of a ball of radius 0.45 r is a neighbour pair"""
    xyz, r, _, info = R.case(f"ball_{n}")
    k = R.case_moments(f"ball_{n}")[0]
    assert np.all(k == n - 1) and info["k"] == n - 1
    if n >= 4:
        assert R.thin_margin(*R.case_moments(f"ball_{n}"), R.grid(xyz, r)[0], n - 1) > 2.0
    c = R.cells(*R.case(f"scattered_{n}")[:2])
    assert np.all(c.max(0) - c.min(0) <= (5, 5, 4))


def test_far_blobs_land_on_shift_0_and_1_and_one_notch_past():
    """(f) the bits_cell loop of cloud_build_index, restated: the two separations give shift 0 and 1, the next one no grid"""
    for shift in (0, 1):
        xyz, r, _, info = R.case(f"far_shift{shift}")
        assert R.grid(xyz, r)[2] == shift
        assert np.all(R.case_moments(f"far_shift{shift}")[0] == info["k"])
    with pytest.raises(ValueError, match="cell size too small"):
        R.grid(R.far_blobs(0.01, -1)[0], 0.01)


def test_utm_shift_keeps_k_where_no_pair_is_near_the_radius():
    """(f) k per point is that of the unshifted cloud wherever no pair of it lies within 2^-20 r^2 of r^2; that share is < 1 %"""
    xyz, r, _, _ = R.case("scan")
    near = R.near_radius_share(xyz, r)
    print(f"\n[mme-ref] scan: {near.mean():.4%} of the points have a pair within 2^-20 r^2 of r^2")
    assert near.mean() < 0.01
    k = R.case_moments("scan")[0]
    for name in ("scan_utm", "scan_utm_neg"):
        assert np.array_equal(R.case_moments(name)[0][~near], k[~near])


def test_reuse_radii_bracket_the_rebuild_condition():
    """(d) mme_run rebuilds when cell_h > 1.5 want_h or cell_h < want_h, both carrying the same (1 + 2^-20): c vs 1.5 r"""
    for c in R.REUSE_CELLS:
        assert [c <= 1.5 * r and r <= c for r in R.reuse_radii(c)] == [True, True, True, True, False]
