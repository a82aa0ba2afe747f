"""DBSCAN clustering and the cluster-size filter on the MI355X (me_cluster.hip) against the numpy / scipy model (tests/_cluster_ref.py):
labels, counts, cluster numbers and sizes of EVERY point equal (all of it is integer arithmetic on the same d2), the diameter case, the
strict radius, small clouds against the literal Open3D loop, run-to-run and permutation identity, the ghost scene through the filter and
the selection, states and arguments, and coarse alignment with the filter."""
import math

import numpy as np
import pytest

import _cluster_ref as R

pytestmark = pytest.mark.gpu

SETTINGS = [(0.05, 10), (0.1, 10), (0.1, 1), (0.05, 2), (0.1, 10 ** 6)]


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


_SCENES = {}


def _scene(n, kind="scan"):
    from cloud_map_evaluation_amd import synth

    key = (n, kind)
    if key not in _SCENES:
        if kind == "scan":
            est, _ = synth.scan_pair(n, density=2500.0, seed=51, outlier_ratio=0.002)
        else:
            est, _ = synth.campus_pair(n, density=2500.0, seed=52, outlier_ratio=0.002)
        _SCENES.clear()
        _SCENES[key] = est.numpy()
    return _SCENES[key]


def _assert_equal(e, slot, got, ref, what):
    info, labels, counts = got
    l_ref, c_ref, m_ref = ref
    n = len(l_ref)
    core = c_ref >= what[1]
    n_border = int(((l_ref >= 0) & ~core).sum())
    sizes_ref = R.cluster_sizes(l_ref, m_ref)
    print(f"{what}: n {n}, clusters {m_ref}, core {int(core.sum())}, border {n_border}, noise {int((l_ref < 0).sum())}, "
          f"largest {int(sizes_ref.max()) if m_ref else 0}; device {info}")
    assert np.array_equal(counts, c_ref), f"{what}: {np.count_nonzero(counts != c_ref)} counts differ"
    assert np.array_equal(labels, l_ref), f"{what}: {np.count_nonzero(labels != l_ref)} labels differ"
    assert info == {"n_in": n, "n_clusters": m_ref, "n_core": int(core.sum()), "n_border": n_border, "n_noise": int((l_ref < 0).sum()),
                    "largest": int(sizes_ref.max()) if m_ref else 0}
    assert np.array_equal(e.cluster_sizes(slot), sizes_ref)


@pytest.mark.parametrize("n,kind", [(100_000, "scan"), (1_000_000, "scan"), (1_000_000, "campus"), (5_000_000, "scan")])
def test_every_point_equals_the_model(n, kind):
    xyz = _scene(n, kind)
    settings = [s for s in SETTINGS if n < 5_000_000 or s[0] == 0.05]  # (the model's pair list at eps 0.1 outgrows host memory at 5 M)
    with _engine() as a, _engine() as b:
        a.upload(0, xyz, cell_size=0.1)
        b.upload(0, xyz)  # automatic cell: the grid is rebuilt at eps
        pr_eps, pr = None, None
        for eps, mp in sorted(settings):
            if eps != pr_eps:
                pr_eps, pr = eps, R.pairs(xyz, eps)
            ref = R.dbscan(xyz, eps, mp, pr)
            _assert_equal(a, 0, a.cluster_dbscan(0, eps, mp, fetch=True), ref, (eps, mp, "cell 0.1"))
            if mp == 10:
                _assert_equal(b, 0, b.cluster_dbscan(0, eps, mp, fetch=True), ref, (eps, mp, "automatic cell"))
            if (n, kind, eps, mp) == (1_000_000, "scan", 0.05, 10):
                assert ref[2] > 100  # the many-cluster regime
            if (n, kind, eps, mp) == (1_000_000, "scan", 0.1, 10):
                assert R.cluster_sizes(ref[0], ref[2]).max() > 900_000  # one giant cluster


def test_chain_diameter_and_rows_exactly_eps_apart():
    rng = np.random.default_rng(5)
    n = 100_000
    x = np.arange(n) * 0.09
    xyz = np.stack([x, np.zeros(n), np.zeros(n)], 1) + rng.uniform(-0.002, 0.002, (n, 3))
    xyz = xyz[rng.permutation(n)]
    ref = R.dbscan(xyz, 0.1, 2)
    assert ref[2] == 1 and (ref[0] == 0).all()  # one cluster 9 km long, no noise
    with _engine() as e:
        e.upload(0, xyz)
        _assert_equal(e, 0, e.cluster_dbscan(0, 0.1, 2, fetch=True), ref, (0.1, 2, "chain"))
    # two rows of dyadic coordinates, spacing 0.0625, offset in y by exactly eps = 0.125: d2 == eps^2 does not connect
    k = 4096
    row = np.arange(k) * 0.0625
    xyz = np.concatenate([np.stack([row, np.zeros(k), np.zeros(k)], 1), np.stack([row, np.full(k, 0.125), np.zeros(k)], 1)])
    xyz = xyz[rng.permutation(len(xyz))]
    ref = R.dbscan(xyz, 0.125, 2)
    assert ref[2] == 2
    with _engine() as e:
        e.upload(0, xyz)
        _assert_equal(e, 0, e.cluster_dbscan(0, 0.125, 2, fetch=True), ref, (0.125, 2, "rows"))


def _lattice(spacing, k=5):
    g = np.arange(k, dtype=np.float64) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def _bridge():
    a = np.stack([-np.arange(21) * 0.05, np.zeros(21), np.zeros(21)], 1)
    b = np.stack([0.6 + np.arange(21) * 0.05, np.zeros(21), np.zeros(21)], 1)
    return np.concatenate([a, [[0.3, 0.0, 0.0]], b])


@pytest.mark.parametrize("case", ["dup", "n1", "n2", "n_lt_min", "lattice_eps", "lattice_below", "bridge", "blobs"])
def test_small_clouds_against_the_open3d_loop(case):
    rng = np.random.default_rng(11)
    eps, mps = 0.25, (1, 2, 5)
    if case == "dup":
        base = R.blobs(rng, 3, 40, 0.1, 1.5, 30)
        xyz = np.concatenate([base, base, base])  # every point three times
    elif case == "n1":
        xyz = rng.random((1, 3))
    elif case == "n2":
        xyz = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]])
    elif case == "n_lt_min":
        xyz, mps = rng.random((4, 3)) * 0.1, (5, 6)
    elif case == "lattice_eps":
        xyz = _lattice(eps)
    elif case == "lattice_below":
        xyz = _lattice(eps * (1.0 - 2.0 ** -30))
    elif case == "bridge":
        xyz, eps, mps = _bridge()[rng.permutation(43)], 0.31, (5,)
    else:
        xyz = R.blobs(rng, 5, 90, 0.12, 2.0, 100)
    for mp in mps:
        l_ref, c_ref, m_ref = R.brute_open3d(xyz, eps, mp, seed=3)
        with _engine() as e:
            e.upload(0, xyz)
            _assert_equal(e, 0, e.cluster_dbscan(0, eps, mp, fetch=True), (l_ref, c_ref, m_ref), (eps, mp, case))
        if case == "bridge":
            i = int(np.nonzero(c_ref == 3)[0][0])  # the point between the rows: a border point of both, the smaller id wins
            assert m_ref == 2 and l_ref[i] == 0
        if case == "lattice_eps" and mp == 2:
            assert m_ref == 0
        if case == "lattice_below" and mp == 2:
            assert m_ref == 1


def test_identical_from_run_to_run_and_under_a_permutation():
    xyz = _scene(100_000)
    perm = np.random.default_rng(2).permutation(len(xyz))
    with _engine() as e:
        e.upload(0, xyz, cell_size=0.1)
        i1, l1, c1 = e.cluster_dbscan(0, 0.05, 10, fetch=True)
        s1 = e.cluster_sizes(0)
        i2, l2, c2 = e.cluster_dbscan(0, 0.05, 10, fetch=True)
        assert i1 == i2 and np.array_equal(l1, l2) and np.array_equal(c1, c2) and np.array_equal(s1, e.cluster_sizes(0))
        e.upload(0, xyz[perm], cell_size=0.1)
        i3, l3, c3 = e.cluster_dbscan(0, 0.05, 10, fetch=True)
    back_l, back_c = np.empty_like(l3), np.empty_like(c3)
    back_l[perm], back_c[perm] = l3, c3
    assert np.array_equal(back_c, c1) and i3["n_clusters"] == i1["n_clusters"] and i3["n_core"] == i1["n_core"]
    core = c1 >= 10
    pairs = set(zip(l1[core].tolist(), back_l[core].tolist()))  # the same partition of the core points
    assert len(pairs) == i1["n_clusters"] == len({a for a, _ in pairs}) == len({b for _, b in pairs})
    assert np.array_equal(back_l == -1, l1 == -1)
    assert np.array_equal(l3, R.dbscan(xyz[perm], 0.05, 10)[0])


def _ghost_scene():
    scene = _scene(1_000_000)
    rng = np.random.default_rng(77)
    lo, hi = scene.min(0), scene.max(0)
    blobs = []
    for _ in range(40):
        m = int(rng.integers(200, 2001))
        c = np.array([rng.uniform(lo[0], hi[0]), rng.uniform(lo[1], hi[1]), hi[2] + rng.uniform(2.0, 6.0)])
        blobs.append(c + rng.normal(0.0, 0.05, (m, 3)))
    ghost = np.concatenate(blobs)
    xyz = np.concatenate([scene, ghost])
    is_ghost = np.concatenate([np.zeros(len(scene), bool), np.ones(len(ghost), bool)])
    p = rng.permutation(len(xyz))
    return xyz[p], is_ghost[p]


def test_ghost_scene_filter_and_selection():
    xyz, is_ghost = _ghost_scene()
    l_ref, c_ref, m_ref = R.dbscan(xyz, 0.1, 10)
    sizes = R.cluster_sizes(l_ref, m_ref)
    keep_ref = R.cluster_keep(l_ref, m_ref, 5000)
    print(f"ghost scene: {m_ref} clusters, the five largest {np.sort(sizes)[-5:].tolist()}, {int(keep_ref[is_ghost].sum())} of "
          f"{int(is_ghost.sum())} blob points kept, {int((~keep_ref[~is_ghost]).sum())} of {int((~is_ghost).sum())} scene points dropped")
    assert keep_ref[is_ghost].sum() == 0  # no ghost survives
    assert (~keep_ref[~is_ghost]).sum() < 0.01 * (~is_ghost).sum()  # only the sparse outliers go
    with _engine() as a, _engine() as b:
        a.upload(0, xyz, cell_size=0.1)
        _assert_equal(a, 0, a.cluster_dbscan(0, 0.1, 10, fetch=True), (l_ref, c_ref, m_ref), (0.1, 10, "ghost"))
        info, keep = a.cluster_keep(0, 5000, fetch=True)
        assert np.array_equal(keep.astype(bool), keep_ref)
        assert info["n_in"] == len(xyz) and info["n_kept"] == int(keep_ref.sum()) and info["threshold"] == 5000
        assert a.select_kept_into(0, b, 1) == int(keep_ref.sum())
        assert np.array_equal(b.download(1), xyz[keep_ref])
        assert np.array_equal(a.download(0), xyz)
        _, k1 = a.cluster_keep(0, 1, keep_largest=1, fetch=True)
        assert np.array_equal(k1.astype(bool), R.cluster_keep(l_ref, m_ref, 1, 1)) and np.array_equal(k1.astype(bool), keep_ref)
        _, k2 = a.cluster_keep(0, 1, keep_largest=2, fetch=True)
        assert np.array_equal(k2.astype(bool), R.cluster_keep(l_ref, m_ref, 1, 2))
        second = int(np.sort(sizes)[-2])
        assert int(k2.sum()) - int(k1.sum()) == second and is_ghost[k2.astype(bool) & ~k1.astype(bool)].all()
        a.cluster_keep(0, 5000)
        assert a.select_kept_into(0) == int(keep_ref.sum())  # in place
        assert np.array_equal(a.download(0), xyz[keep_ref])
    with _engine() as e:  # the one-liner
        e.upload(0, xyz, cell_size=0.1)
        n_kept, info = e.remove_small_clusters(0, 0.1, 10, min_cluster_size=5000)
        assert n_kept == info["n_kept"] == int(keep_ref.sum()) and info["n_clusters"] == m_ref
        assert np.array_equal(e.download(0), xyz[keep_ref])


def test_states_and_arguments():
    from cloud_map_evaluation_amd.engine import MapEvalError

    xyz = _scene(100_000)
    with _engine() as e:
        e.upload(0, xyz, cell_size=0.1)
        with pytest.raises(MapEvalError, match="no cluster labels"):
            e.cluster_keep(0, 1)
        with pytest.raises(MapEvalError, match="no cluster labels"):
            e.cluster_sizes(0)
        for eps in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(MapEvalError, match="eps"):
                e.cluster_dbscan(0, eps, 10)
        with pytest.raises(MapEvalError, match="min_points"):
            e.cluster_dbscan(0, 0.1, 0)
        with pytest.raises(MapEvalError, match="slot"):
            e.cluster_dbscan(2, 0.1, 10)
        with pytest.raises(MapEvalError):
            e.cluster_dbscan(1, 0.1, 10)  # nothing uploaded there
        e.cluster_dbscan(0, 0.1, 10)
        with pytest.raises(MapEvalError, match="min_cluster_size"):
            e.cluster_keep(0, 0)
        with pytest.raises(MapEvalError, match="keep_largest"):
            e.cluster_keep(0, 1, keep_largest=-1)
        e.cluster_keep(0, 10 ** 9)  # keeps nothing: the selection refuses an empty cloud
        with pytest.raises(MapEvalError, match="keeps no point"):
            e.select_kept_into(0)
        shift = np.eye(4)
        shift[:3, 3] = (0.5, 0.25, 0.0)
        e.transform_cloud(0, shift)  # a change of the cloud drops labels and mask
        with pytest.raises(MapEvalError, match="no cluster labels"):
            e.cluster_keep(0, 1)
        e.cluster_dbscan(0, 0.1, 10)
        e.voxel_downsample(0, 0.5)
        with pytest.raises(MapEvalError, match="no cluster labels"):
            e.cluster_keep(0, 1)
    with _engine() as e:
        e.set_slab(0, float(xyz[:, 0].min()) - 1, float(np.median(xyz[:, 0])), 1.0)
        e.upload(0, xyz, cell_size=0.1)
        with pytest.raises(MapEvalError, match="slab"):
            e.cluster_dbscan(0, 0.1, 10)
    # a cloud uploaded with a transform is labelled in its cloud order
    yaw = math.radians(30.0)
    T = np.eye(4)
    T[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
    T[:3, 3] = (3.0, -2.0, 0.5)
    with _engine() as e:
        e.upload(0, xyz, T=T, cell_size=0.1)
        moved = e.download(0)
        _assert_equal(e, 0, e.cluster_dbscan(0, 0.05, 10, fetch=True), R.dbscan(moved, 0.05, 10), (0.05, 10, "transformed"))


def _angle_deg(R_):
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R_) - 1.0) / 2.0))))


def test_coarse_align_with_the_cluster_filter():
    """The pair and pose of test_gpu_outlier.py::test_coarse_align_with_outlier_filter, the statistical AND the cluster filter on: the
    same bounds.  The cluster filter alone is printed, not asserted.  Seen on an MI355X: see DESIGN.md section 4.9."""
    from cloud_map_evaluation_amd import synth

    est, gt = synth.scan_pair(5_000_000, outlier_ratio=0.001)
    est, gt = est.numpy(), gt.numpy()
    yaw = math.radians(135.0)
    Tm = np.eye(4)
    Tm[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
    Tm[:3, 3] = (12.0, -7.0, 1.5)
    est_m = est @ Tm[:3, :3].T + Tm[:3, 3]
    Ttrue = np.linalg.inv(Tm)
    c = est_m.mean(0)

    def err(T):
        dr = _angle_deg(T[:3, :3] @ Ttrue[:3, :3].T)
        dt = float(np.linalg.norm((T[:3, :3] @ c + T[:3, 3]) - (Ttrue[:3, :3] @ c + Ttrue[:3, 3])))
        return dr, dt

    with _engine() as e:
        e.upload(0, est_m, cell_size=0.1)
        e.upload(1, gt, cell_size=0.1)
        before = e.download(0)
        T0 = e.coarse_align(1.0, max_iterations=200_000)
        T0b = e.coarse_align(1.0, max_iterations=200_000, cluster_eps=0.0, cluster_min_points=7, cluster_min_size=3)
        assert np.array_equal(T0, T0b) and e.last_coarse_clusters is None  # cluster_eps = 0: the call without the new arguments
        T1 = e.coarse_align(1.0, max_iterations=200_000, outlier_nb_neighbors=20, cluster_eps=0.1, cluster_min_size=5000)
        dr, dt = err(T1)
        print("statistical + cluster filter: %.2f deg, %.3f m; outliers %s; clusters %s" % (dr, dt, e.last_coarse_outliers, e.last_coarse_clusters))
        assert dr < 1.0 and dt < 0.5
        assert len(e.last_coarse_clusters) == 2 and all(ci["n_kept"] <= ci["n_in"] for ci in e.last_coarse_clusters)
        assert e.last_coarse_clusters[0]["n_in"] == e.last_coarse_outliers[0]["n_kept"]
        assert np.array_equal(e.download(0), before) and e.size(0) == len(est_m) and e.size(1) == len(gt)  # the resident clouds are untouched
        T2 = e.coarse_align(1.0, max_iterations=200_000, cluster_eps=0.1, cluster_min_size=5000)
        print("cluster filter alone: %.2f deg, %.3f m; clusters %s" % (*err(T2), e.last_coarse_clusters))  # (no assertion: nobody had run it)
        assert np.array_equal(e.download(0), before)
