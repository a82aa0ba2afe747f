"""me_cluster_dbscan, me_cluster_sizes and me_cluster_keep on the MI355X at their exact edges, on the small clouds of
tests/_cluster_edge_cases.py (tests/test_cluster_cpu.py proves with the model alone that each does what it is built for).  Everything
is integer and compared with == on every point against R.dbscan over the exact O(n^2) pair list R.brute_pairs: labels, counts, the
info, the sizes, the keep-mask.  Every dbscan call is made twice in one context and once in a fresh one: the bytes of all three agree.

What each case reaches in me_cluster.hip:
  sizes            n across wave and block edges; min_points 1: every lane pending in k_cluster_union, no border candidate (clusters,
                   k_cluster_border skipped: m > 0, nb == 0); 2 and 4: the stream entered with some lanes of a wave pending (core lanes
                   in the union, the compacted candidates in the border pass, 0 .. 64 of them per wave); n + 1: no lane pending, no
                   root (m == 0: numbering, border pass and k_cluster_largest skipped, nb > 0 wherever a point has a neighbour).
                   block_keyed_atomic: n >= 1024 holds >= 600 points of one cell, contiguous in the sorted order, so a whole block has
                   one root / one label (one atomic per block); blocks of the sheet and the isolated points hold many keys and invalid
                   lanes (one per wave and key); the last block of every n that is no multiple of 256 has lanes past the end.
  shapes           the union-find: 64 sets arriving at one root, two trees of 2000 that meet at their far end only, a closed loop, a
                   comb, 4097 coincident points (every pair an edge, one cell far longer than the 64-entry tile)
  border rules     one border point between three clusters; candidates without a core neighbour; both skipped-launch combinations;
                   600 border points of ONE cluster and no other candidate: whole blocks of k_cluster_border with one key
  keep             ties in size cut by keep_largest, keep_largest >= m (no sort), a threshold equal to a size, no cluster at all, more
                   clusters than one block of the k_cluster_rank_* kernels (257)."""
import struct

import numpy as np
import pytest

import _cluster_edge_cases as E
import _cluster_ref as R

pytestmark = pytest.mark.gpu

INFO_KEYS = ("n_in", "n_clusters", "n_core", "n_border", "n_noise", "largest")


def _engine():
    from cloud_map_evaluation_amd.engine import Engine

    return Engine(0)


def _bytes(out):
    info, labels, counts, sizes = out
    assert labels.dtype == np.int32 and counts.dtype == np.int32 and sizes.dtype == np.int64
    return struct.pack("<6q", *[info[k] for k in INFO_KEYS]) + labels.tobytes() + counts.tobytes() + sizes.tobytes()


def _run(e, eps, mp):
    info, labels, counts = e.cluster_dbscan(0, eps, mp, fetch=True)
    return info, labels, counts, e.cluster_sizes(0)


def _model(xyz, eps, mp, pr=None):
    return R.dbscan(xyz, eps, mp, R.brute_pairs(xyz, eps) if pr is None else pr)


def _equal(out, ref, mp, what=""):
    """One result against the model, every point; the device's own sizes against its own labels."""
    info, labels, counts, sizes = out
    l_ref, c_ref, m_ref = ref
    n = len(l_ref)
    core = c_ref >= mp
    sizes_ref = R.cluster_sizes(l_ref, m_ref)
    want = {"n_in": n, "n_clusters": m_ref, "n_core": int(core.sum()), "n_border": int(((l_ref >= 0) & ~core).sum()),
            "n_noise": int((l_ref < 0).sum()), "largest": int(sizes_ref.max()) if m_ref else 0}
    print(f"{what} n={n} min_points={mp}: device {info} model {want}")
    assert np.array_equal(counts, c_ref), f"{np.count_nonzero(counts != c_ref)} counts differ, first at {np.flatnonzero(counts != c_ref)[:8]}"
    assert np.array_equal(labels, l_ref), f"{np.count_nonzero(labels != l_ref)} labels differ, first at {np.flatnonzero(labels != l_ref)[:8]}"
    assert info == want
    assert np.array_equal(sizes, sizes_ref)
    assert int(sizes.sum()) == info["n_core"] + info["n_border"]
    assert np.array_equal(sizes, np.bincount(labels[labels >= 0], minlength=info["n_clusters"]))


def _check(xyz, eps, mp, cell_size=0.0, ref=None, what=""):
    """One cluster_dbscan call held to the model, twice in one context and once in a fresh one; -> (info, labels, counts, sizes)."""
    if ref is None:
        ref = _model(xyz, eps, mp)
    with _engine() as e:
        e.upload(0, xyz, cell_size=cell_size)
        a = _run(e, eps, mp)
        b = _run(e, eps, mp)
    with _engine() as e:
        e.upload(0, xyz, cell_size=cell_size)
        c = _run(e, eps, mp)
    _equal(a, ref, mp, what)
    assert _bytes(a) == _bytes(b), "the second call in one context differs"
    assert _bytes(a) == _bytes(c), "a fresh context differs"
    return a


# ---- 1. sizes ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 4097])
def test_sizes(n):
    from cloud_map_evaluation_amd.engine import MapEvalError

    xyz, eps = E.clumpy(n)
    pr = R.brute_pairs(xyz, eps)
    for mp in (1, 2, 4, n + 1):
        info = _check(xyz, eps, mp, ref=_model(xyz, eps, mp, pr), what="clumpy")[0]
        if mp == 1:
            assert info["n_core"] == n and info["n_border"] == 0 and info["n_noise"] == 0
        if mp == n + 1:
            assert info["n_core"] == 0 and info["n_clusters"] == 0 and info["n_noise"] == n
    with _engine() as e:  # no cluster at all: the filter keeps nothing
        e.upload(0, xyz)
        info, labels, counts = e.cluster_dbscan(0, eps, n + 1, fetch=True)
        assert (labels == -1).all() and len(e.cluster_sizes(0)) == 0
        kinfo, keep = e.cluster_keep(0, 1, 0, fetch=True)
        assert not keep.any() and keep.shape == (n,) and kinfo["n_kept"] == 0 and kinfo["n_in"] == n and kinfo["threshold"] == 1
        kinfo, keep = e.cluster_keep(0, 1, 1, fetch=True)
        assert not keep.any() and kinfo["n_kept"] == 0
        with pytest.raises(MapEvalError, match="keeps no point"):
            e.select_kept_into(0)


# ---- 2. min_points at the count ----
def test_min_points_at_the_count():
    xyz, eps, table = E.lattice_counts(5)
    pr = R.brute_pairs(xyz, eps)
    for mp in (4, 5, 6, 7, 8):
        info = _check(xyz, eps, mp, ref=_model(xyz, eps, mp, pr), what="lattice")[0]
        assert (info["n_core"], info["n_border"], info["n_noise"], info["n_clusters"]) == table[mp]


# ---- 3. the strict radius in all 26 directions ----
def _stencil(offset):
    xyz, eps, exact, inside = E.stencil_ties(offset)
    info, labels, counts, sizes = _check(xyz, eps, 2, what="stencil")
    assert info["n_clusters"] == 26 and (sizes == 2).all() and info["n_noise"] == 52
    assert (labels[exact] == -1).all() and (counts[exact] == 1).all()  # d2 == eps^2 is no neighbour, whichever cell the partner is in
    assert np.array_equal(labels[inside], np.stack([np.arange(26)] * 2, 1)) and (counts[inside] == 2).all()


def test_strict_radius_in_all_26_directions():
    _stencil((0.0, 0.0, 0.0))


# ---- 4. survey and negative coordinates ----
@pytest.mark.parametrize("offset", [E.SURVEY, E.STRADDLE], ids=["survey", "straddle"])
def test_translated(offset):
    xyz, eps, table = E.lattice_counts(5, offset)
    E.check_lattice_counts(xyz, eps)  # (dyadic: the translated lattice is still exact)
    pr = R.brute_pairs(xyz, eps)
    for mp in (4, 5, 6, 7, 8):
        info = _check(xyz, eps, mp, ref=_model(xyz, eps, mp, pr), what="lattice")[0]
        assert (info["n_core"], info["n_border"], info["n_noise"], info["n_clusters"]) == table[mp]
    _stencil(offset)  # (the builder re-asserts ties, one-ulp pairs and cells at the translated coordinates)
    xyz, eps = E.clumpy(4097)
    xyz = xyz + np.asarray(offset)
    pr = R.brute_pairs(xyz, eps)
    for mp in (2, 4):
        _check(xyz, eps, mp, ref=_model(xyz, eps, mp, pr), what="clumpy")
    xyz, eps, m = E.shapes("u")
    xyz = xyz + np.asarray(offset)
    assert _check(xyz, eps, 2, what="u")[0]["n_clusters"] == m


# ---- 5. the index rebuild rule ----
def test_index_rebuild_rule():
    xyz, eps = E.clumpy(4097)
    assert eps == 0.1
    n = len(xyz)
    pr = R.brute_pairs(xyz, eps)
    refs = {mp: _model(xyz, eps, mp, pr) for mp in (2, 4)}
    first = {}
    for cell_size in (0.0, 0.5 * eps, eps, 1.5 * eps, float(np.nextafter(1.5 * eps * (1.0 + 2.0 ** -20), np.inf)), 3.0 * eps):
        with _engine() as e:
            e.upload(0, xyz, cell_size=cell_size)
            for mp in (2, 4):
                out = _run(e, eps, mp)
                _equal(out, refs[mp], mp, f"cell_size {cell_size!r}")
                assert _bytes(out) == first.setdefault(mp, _bytes(out)), f"cell_size {cell_size!r} differs from the first"
                idx, d2 = e.nn1(0, 0)  # the slot is still usable after a rebuild at eps
                assert np.array_equal(idx, np.arange(n)) and (d2 == 0.0).all()


# ---- 6. union-find shapes ----
def _same_partition(xyz_a, out_a, xyz_b, out_b, mp):
    """The two clouds are permutations of each other: the same partition of the core points."""
    ia, ib = np.lexsort(xyz_a.T), np.lexsort(xyz_b.T)
    assert np.array_equal(xyz_a[ia], xyz_b[ib])
    la, lb, ca, cb = out_a[1][ia], out_b[1][ib], out_a[2][ia], out_b[2][ib]
    assert np.array_equal(ca, cb)
    core = ca >= mp
    m = out_a[0]["n_clusters"]
    pairs = set(zip(la[core].tolist(), lb[core].tolist()))
    assert out_b[0]["n_clusters"] == m == len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})


def _numbered_by_smallest_core_index(out, mp):
    info, labels, counts, _ = out
    core = counts >= mp
    first = [int(np.flatnonzero(core & (labels == k))[0]) for k in range(info["n_clusters"])]
    assert first == sorted(first)


@pytest.mark.parametrize("kind", ["star", "u", "u_open", "ring", "comb"])
def test_union_find_shapes(kind):
    xyz, eps, m = E.shapes(kind)
    base = _check(xyz, eps, 2, what=kind)
    assert base[0]["n_clusters"] == m and base[0]["n_noise"] == 0
    _numbered_by_smallest_core_index(base, 2)
    for seed in (1, 2):
        other = E.shapes(kind, seed)[0]
        with _engine() as e:
            e.upload(0, other)
            out = _run(e, eps, 2)
        _equal(out, _model(other, eps, 2), 2, f"{kind} order {seed}")
        _same_partition(xyz, base, other, out, 2)
        _numbered_by_smallest_core_index(out, 2)


def test_union_find_dense_cell():
    xyz, eps, want = E.shapes("dense")
    pr = R.brute_pairs(xyz, eps)
    outs = {}
    for mp in (1, 4097, 4098):
        outs[mp] = _check(xyz, eps, mp, ref=_model(xyz, eps, mp, pr), what="dense")
        assert outs[mp][0]["n_clusters"] == want[mp]
        assert sorted(np.unique(outs[mp][2]).tolist()) == [1, 4097]
    assert outs[1][3].tolist() in ([4097, 1], [1, 4097]) and outs[4097][3].tolist() == [4097] and outs[4098][0]["n_noise"] == 4098
    for seed in (1, 2):
        other = E.shapes("dense", seed)[0]
        for mp in (1, 4097):
            with _engine() as e:
                e.upload(0, other)
                out = _run(e, eps, mp)
            _equal(out, _model(other, eps, mp), mp, f"dense order {seed}")
            _same_partition(xyz, outs[mp], other, out, mp)
            _numbered_by_smallest_core_index(out, mp)


# ---- 7. border rules ----
def test_border_rules():
    xyz, eps, parts = E.border_rules()
    mp = E.BORDER_MIN_POINTS
    shared, pair = int(parts["shared"][0]), parts["pair"]
    winners = []
    for perm in E.border_permutations():
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        ref = _model(xyz[perm], eps, mp)
        winners.append([k for k in range(3) if ref[0][inv[parts[f"blob{k}"][0]]] == 0][0])  # (on the model)
        info, labels, counts, sizes = _check(xyz[perm], eps, mp, ref=ref, what="border")
        assert info["n_clusters"] == 3 and info["n_border"] == 1 and info["n_noise"] == 3
        assert labels[inv[shared]] == 0 and counts[inv[shared]] == 4  # the smallest id of its three clusters
        assert (labels[inv[pair]] == -1).all() and (counts[inv[pair]] == 2).all()  # candidates without a core neighbour: noise
        assert sizes.tolist() == [7, 6, 6]
        # min_points 3, the same order: the shared point is core itself and joins the three chains
        info = _check(xyz[perm], eps, 3, what="border at 3")[0]
        assert (info["n_clusters"], info["n_core"], info["n_border"], info["n_noise"]) == (1, 19, 0, 3)
    assert winners == [0, 1, 2, 0, 1, 2]  # cluster 0 is another blob from each order to the next, each blob twice


def test_skipped_launches():
    xyz, eps = E.blobs_and_singletons()  # clusters and no border candidate: m > 0, nb == 0
    info, labels, counts, sizes = _check(xyz, eps, 3, what="blobs and singletons")
    assert info["n_clusters"] == 5 and info["n_border"] == 0 and not ((counts >= 2) & (counts < 3)).any()
    xyz, eps = E.many_pairs(257)  # border candidates and no cluster: m == 0, nb > 0
    info, labels, counts, sizes = _check(xyz, eps, 3, what="loose pairs")
    assert info["n_clusters"] == 0 and info["n_border"] == 0 and info["n_noise"] == 514 and (counts == 2).all()


def test_border_points_of_one_cluster_fill_whole_blocks():
    xyz, eps, mp = E.halo()
    info, labels, counts, sizes = _check(xyz, eps, mp, what="halo")
    assert (info["n_clusters"], info["n_core"], info["n_border"], info["n_noise"]) == (1, 8, 600, 0) and sizes.tolist() == [608]


# ---- 8. cluster_keep ----
def _keep_equal(e, labels, m, min_size, keep_largest):
    info, keep = e.cluster_keep(0, min_size, keep_largest, fetch=True)
    ref = R.cluster_keep(labels, m, min_size, keep_largest)
    assert keep.dtype == np.uint8 and set(np.unique(keep).tolist()) <= {0, 1}
    assert np.array_equal(keep.astype(bool), ref), (min_size, keep_largest, np.flatnonzero(keep.astype(bool) != ref)[:8])
    assert info["n_kept"] == int(keep.sum()) and info["threshold"] == min_size and info["n_in"] == len(labels)
    return keep.astype(bool)


def test_keep_on_tied_sizes():
    xyz, eps, sizes_want = E.tied_sizes()
    m = len(sizes_want)
    with _engine() as e, _engine() as f:
        e.upload(0, xyz)
        out = _run(e, eps, 1)
        _equal(out, _model(xyz, eps, 1), 1, "tied sizes")
        labels = out[1]
        assert np.array_equal(out[3], sizes_want)
        for keep_largest in (0, 1, 2, 3, 4, m - 1, m, m + 1, 10 ** 12):
            for min_size in (1, 3, 9, 10):
                keep = _keep_equal(e, labels, m, min_size, keep_largest)
                if min_size == 1 and keep_largest in (2, 3):
                    assert np.unique(labels[keep]).tolist() == [1, 2, 4][:keep_largest]  # the tie: the smaller ids
                if min_size == 10:
                    assert not keep.any()
                elif keep.any():  # the selection takes exactly the kept points, in cloud order
                    assert e.select_kept_into(0, f, 1) == int(keep.sum())
                    assert f.download(1).tobytes() == xyz[keep].tobytes()
        assert e.download(0).tobytes() == xyz.tobytes()


def test_keep_on_many_clusters_and_on_one():
    from cloud_map_evaluation_amd.engine import MapEvalError

    xyz, eps = E.many_pairs(257)
    with _engine() as e, _engine() as f:
        e.upload(0, xyz)
        out = _run(e, eps, 2)
        _equal(out, _model(xyz, eps, 2), 2, "many pairs")
        labels = out[1]
        assert out[0]["n_clusters"] == 257 and (out[3] == 2).all()
        keep = _keep_equal(e, labels, 257, 1, 100)
        assert np.array_equal(np.flatnonzero(keep), np.arange(200)) and np.unique(labels[keep]).tolist() == list(range(100))
        assert e.select_kept_into(0, f, 0) == 200 and f.download(0).tobytes() == xyz[:200].tobytes()
        for keep_largest in (1, 256, 257, 258):
            for min_size in (1, 2):
                _keep_equal(e, labels, 257, min_size, keep_largest)
        for keep_largest in (0, 100):
            assert not _keep_equal(e, labels, 257, 3, keep_largest).any()
            with pytest.raises(MapEvalError, match="keeps no point"):
                e.select_kept_into(0)
        assert e.download(0).tobytes() == xyz.tobytes()
    xyz, eps, _ = E.lattice_counts(5)  # one cluster: keep_largest == m, the branch without the sort
    with _engine() as e, _engine() as f:
        e.upload(0, xyz)
        out = _run(e, eps, 6)
        _equal(out, _model(xyz, eps, 6), 6, "one cluster")
        assert out[0]["n_clusters"] == 1
        for min_size in (1, 117, 118):
            keep = _keep_equal(e, out[1], 1, min_size, 1)
            assert int(keep.sum()) == (117 if min_size <= 117 else 0)
        _keep_equal(e, out[1], 1, 1, 1)
        assert e.select_kept_into(0, f, 1) == 117 and f.download(1).tobytes() == xyz[out[1] >= 0].tobytes()
