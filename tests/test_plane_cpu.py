"""The numpy model of the plane segmentation (tests/_plane_ref.py) against its own scalar restatement and against labellings that can
be derived by hand.  No GPU."""
import numpy as np
import pytest

import _globreg_ref as G
import _plane_ref as R


@pytest.mark.parametrize("scene,n,t,H,P,seed", [("planes", 60, 0.08, 40, 3, 0), ("planes", 45, 0.05, 33, 2, 7),
                                                 ("lattice", 0, 0.25, 48, 4, 1), ("collinear", 30, 0.1, 16, 2, 0)])
def test_vectorised_model_equals_scalar_restatement(scene, n, t, H, P, seed):
    if scene == "planes":
        xyz = G.three_planes(n // 3, side=4.0, seed=seed + 1)
    elif scene == "lattice":
        xyz = R.lattice_planes(5, 4, 3)
    else:
        xyz = R.collinear(n)
    m = R.segment(xyz, t, H, P, 3, seed)
    scores, labels, winners = R.segment_scalar(xyz, t, H, P, 3, seed)
    assert np.array_equal(m["scores"], scores)
    assert np.array_equal(m["labels"], labels)
    assert [r["h"] for r in m["records"]] == winners
    if scene == "collinear":
        assert m["info"]["n_planes"] == 0 and np.all(m["scores"] == -1) and m["info"]["rounds"] == 1
    else:
        assert m["info"]["n_planes"] >= 2


def test_lattice_planes_have_the_derivable_labelling():
    xyz = R.lattice_planes()
    sizes = [144, 100, 64]
    for seed in (0, 1, 2):
        m = R.segment(xyz, 0.25, 200, 4, 3, seed)
        # plane r takes every point of the r-th largest generating plane; the fourth round finds fewer than three points
        assert m["info"]["n_planes"] == 3 and m["info"]["rounds"] == 4 and m["info"]["n_labelled"] == len(xyz)
        assert np.array_equal(m["labels"], R.lattice_expected_labels(xyz))
        assert np.all(m["scores"][3] == -1)
        for r, axis in enumerate((2, 0, 1)):
            rec = m["records"][r]
            want = np.zeros(4)
            want[axis] = 1.0
            assert rec["count"] == sizes[r] and np.array_equal(rec["plane"], want)  # the normals are exactly the axes, d = 0
            assert m["scores"][r].max() == sizes[r] and int(np.argmax(m["scores"][r])) == rec["h"]
            # the least-squares plane of exact inliers is the same plane
            pl, w, _ = R.refit_exact(xyz[m["labels"] == r])
            assert abs(w[0]) < 1e-15 and np.allclose(pl, want, rtol=0, atol=1e-14)


def test_min_inliers_ends_the_extraction():
    xyz = R.lattice_planes()
    m = R.segment(xyz, 0.25, 200, 4, 80, 0)  # the y = 0 plane has 64 points
    assert m["info"]["n_planes"] == 2 and m["info"]["rounds"] == 3 and m["scores"][2].max() == 64
    assert np.all(m["labels"][xyz[:, 1] == 0] == -1)


@pytest.mark.parametrize("m", [1, 2, 3, 2 ** 31])
def test_sampling_stays_inside_the_remaining_list(m):
    ks = R.samples(11, np.arange(4096), 3, m)
    assert ks.shape == (4096, 3) and ks.min() >= 0 and ks.max() < m
    if m == 3:
        assert set(np.unique(ks)) == {0, 1, 2}
    # the counter names the round and the user: another round draws other samples
    if m == 2 ** 31:
        assert not np.array_equal(ks, R.samples(11, np.arange(4096), 4, m))
        assert not np.array_equal(ks, G.samples(11, np.arange(4096), m))


def test_threshold_is_strict():
    g = R.lattice_planes(12, 2, 2, shuffle_seed=None)
    g = g[g[:, 2] == 0]
    below = np.nextafter(0.25, 0.0)
    extra = np.array([[2.5, 3.5, 0.25], [7.5, 1.5, -0.25], [4.5, 9.5, below], [10.5, 6.5, -below]])
    xyz = np.concatenate([g, extra])
    m = R.segment(xyz, 0.25, 64, 1, 3, 0)
    assert np.array_equal(m["records"][0]["plane"], [0, 0, 1, 0])
    assert list(m["labels"][-4:]) == [-1, -1, 0, 0] and m["records"][0]["count"] == len(g) + 2
