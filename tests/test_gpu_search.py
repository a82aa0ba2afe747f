"""me_knn_search / me_hybrid_search / me_radius_search on the MI355X against the brute-force model of tests/_search_ref.py.  Every
comparison is exact: np.array_equal on the indices and on the bit patterns of d2.  Sizes around a wave and a block in both directions
and inside one cloud, the tie rule and the strict radius on a dyadic lattice, duplicates, agreement with me_nn1 and with
me_estimate_normals' lists, rows longer than the sort tile next to rows of 0 and 1, queries inside, at the edge of and far outside the
reference's frame, the mask, the two-call protocol and the errors, the state rule (nothing resident is touched), one case at 10^6."""
import ctypes as C
import functools

import numpy as np
import pytest

import _search_ref as S

pytestmark = pytest.mark.gpu

ME_ERR_ARG = -1
ME_ERR_STATE = -3


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(dev, model, what=""):
    """(idx, d2) pairs or (offsets / counts, idx, d2) triples, exactly"""
    assert len(dev) == len(model)
    for k, (a, b) in enumerate(zip(dev, model)):
        if a.dtype == np.float64:
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"{what}: d2 differs (array {k})"
        else:
            assert a.dtype == b.dtype and np.array_equal(a, b), f"{what}: integers differ (array {k})"


def _sheet(n, seed, z=0.0, noise=0.004, lo=(0.0, 0.0), hi=(1.0, 1.0)):
    rng = np.random.default_rng(seed)
    p = np.empty((n, 3))
    p[:, 0] = lo[0] + (hi[0] - lo[0]) * rng.random(n)
    p[:, 1] = lo[1] + (hi[1] - lo[1]) * rng.random(n)
    p[:, 2] = z + noise * rng.standard_normal(n)
    return np.ascontiguousarray(p)


def _blob(n, seed, centre, sigma):
    return np.ascontiguousarray(np.asarray(centre, np.float64) + sigma * np.random.default_rng(seed).standard_normal((n, 3)))


def _engine(a, b=None, cell=0.0):
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    e.upload(0, a, cell_size=cell)
    if b is not None:
        e.upload(1, b, cell_size=cell)
    return e


# ---- 1. sizes around a wave and a block, both directions and both self searches ------------------------------------------------
def _size_cloud(slot, n):
    return _sheet(n, 100 + n) if slot == 0 else _sheet(n, 200 + n, z=0.01)


@functools.lru_cache(maxsize=2)
def _self_order(slot, n):  # (a slot's cloud depends on its size alone: the model of its self search is shared between the cases)
    c = _size_cloud(slot, n)
    return S.ordered(c, c)


@pytest.mark.parametrize("nr", [1, 39, 40, 41, 3000])
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257, 4097])
def test_sizes_directions_and_padding(nq, nr):
    """slot 0 holds nq points, slot 1 nr: 0 -> 1, 1 -> 0, 0 -> 0 and 1 -> 1 for k = 1, 2, 20, 40 (padding with -1 / inf wherever the
    reference holds fewer than k points), and the radius and hybrid lists of the same four pairs at one radius"""
    cl = [_size_cloud(0, nq), _size_cloud(1, nr)]
    r = 0.06
    with _engine(cl[0], cl[1]) as e:
        for qs, rs in ((0, 1), (1, 0), (0, 0), (1, 1)):
            order = _self_order(qs, len(cl[qs])) if qs == rs else S.ordered(cl[qs], cl[rs])
            for k in (1, 2, 20, 40):
                dev = e.knn_search(qs, rs, k)
                _same(dev, S.knn_from(order, k), f"knn {qs}->{rs} k={k}")
                if len(cl[rs]) < k:
                    assert (dev[0][:, len(cl[rs]):] == -1).all() and np.isposinf(dev[1][:, len(cl[rs]):]).all()
            _same(e.radius_search(qs, rs, r), S.radius_from(order, r), f"radius {qs}->{rs}")
            _same(e.hybrid_search(qs, rs, r, 7), S.hybrid_from(order, r, 7), f"hybrid {qs}->{rs}")
            if qs == rs:  # a point is its own first neighbour
                assert np.array_equal(e.knn_search(qs, rs, 1)[0][:, 0], np.arange(len(cl[qs]), dtype=np.int32))


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------
def _lattice():
    return np.array([(i / 8, j / 8, k / 8) for i in range(-6, 7) for j in range(-6, 7) for k in range(-3, 4)], np.float64)


def test_lattice_the_index_rule_and_the_strict_radius():
    """step 1/8: all distances are exact multiples of 1/64 and most are shared by many points, so the index rule alone orders the
    rows; radius 5/8: the points at d2 == r2 (3-4-0, 5-0-0) are excluded"""
    pts = _lattice()
    other = pts + [0.0, 0.0, 1 / 8]
    centre = int(np.flatnonzero((pts == 0).all(axis=1))[0])
    cells = [(i, j, k) for i in range(-6, 7) for j in range(-6, 7) for k in range(-3, 4)]
    own = sum(1 for i, j, k in cells if i * i + j * j + k * k < 25)
    shifted = sum(1 for i, j, k in cells if i * i + j * j + (k + 1) * (k + 1) < 25)  # the other lattice: one step up
    assert own == sum(1 for i, j, k in cells if i * i + j * j + k * k <= 25) - 20  # (the 20 lattice points on the sphere: test_search_cpu)
    with _engine(pts, other) as e:
        for qs, rs, ref, want in ((0, 0, pts, own), (0, 1, other, shifted)):
            order = S.ordered(pts, ref)
            off, idx, d2 = e.radius_search(qs, rs, 5 / 8)
            _same((off, idx, d2), S.radius_from(order, 5 / 8), f"lattice radius {qs}->{rs}")
            assert off[centre + 1] - off[centre] == want
            assert d2.max() == 24 / 64  # nothing at 25/64
            for k in (7, 27, 40):
                _same(e.knn_search(qs, rs, k), S.knn_from(order, k), f"lattice knn {qs}->{rs} k={k}")
            _same(e.hybrid_search(qs, rs, 5 / 8, 40), S.hybrid_from(order, 5 / 8, 40), f"lattice hybrid {qs}->{rs}")
        row = e.knn_search(0, 0, 27)
        assert np.array_equal(row[1][centre] * 64, [0] + [1] * 6 + [2] * 12 + [3] * 8)
        for a, b in ((1, 7), (7, 19), (19, 27)):
            assert (np.diff(row[0][centre, a:b]) > 0).all()


def test_duplicates_the_smaller_index_first():
    p = _sheet(300, 5)
    both = np.concatenate([p, p])
    with _engine(both) as e:
        idx, d2 = e.knn_search(0, 0, 2)
        assert np.array_equal(idx[:, 0], np.tile(np.arange(300, dtype=np.int32), 2))
        assert np.array_equal(idx[:, 1], np.tile(np.arange(300, dtype=np.int32), 2) + 300)
        assert (d2 == 0).all() and not np.signbit(d2).any()
        _same(e.radius_search(0, 0, 0.05), S.radius(both, both, 0.05), "duplicates radius")


# ---- 3. consistency with what exists ------------------------------------------------------------------------------------------------
def test_agrees_with_nn1_normals_lists_and_between_hybrid_and_radius():
    a, b = _sheet(4097, 21), np.concatenate([_sheet(3000, 22, z=0.01), _blob(500, 23, (0.5, 0.5, 0.0), 0.01)])
    with _engine(a, b) as e:
        for qs, rs in ((0, 1), (1, 0)):
            ni, nd = e.nn1(qs, rs)
            ki, kd = e.knn_search(qs, rs, 1)
            assert np.array_equal(ki[:, 0], ni) and np.array_equal(_bits(kd[:, 0]), _bits(nd))
        for s in (0, 1):
            _, li, ld = e.estimate_normals(s, 20, with_neighbours=True)
            _same(e.knn_search(s, s, 20), (li, ld), f"knn {s}->{s} against me_estimate_normals")
        for qs, rs, r, m in ((0, 1, 0.03, 5), (1, 0, 0.07, 40), (1, 1, 0.03, 12)):
            off, idx, d2 = e.radius_search(qs, rs, r)
            cnt, hi, hd = e.hybrid_search(qs, rs, r, m)
            lens = np.diff(off)
            assert np.array_equal(cnt, np.minimum(lens, m).astype(np.int32)) and lens.max() > m and lens.min() < m
            for i in range(len(lens)):
                c = cnt[i]
                assert np.array_equal(hi[i, :c], idx[off[i]:off[i] + c]) and np.array_equal(_bits(hd[i, :c]), _bits(d2[off[i]:off[i] + c]))
                assert (hi[i, c:] == -1).all() and np.isposinf(hd[i, c:]).all()


# ---- 4. rows longer than the sort tile ----------------------------------------------------------------------------------------------
def test_long_rows_next_to_rows_of_zero_and_one():
    """3000 reference points in a blob of sigma 0.004 well inside r = 0.05 of 70 queries, beside a sparse sheet (spacing ~0.7) whose
    points each have one query 0.001 away, and five queries with nothing within r"""
    from cloud_map_evaluation_amd import _lib

    tile = _lib.load().me_search_sort_tile()
    sparse = _sheet(200, 31, noise=0.0, lo=(2.0, 2.0), hi=(12.0, 12.0))
    ref = np.concatenate([_blob(3000, 32, (0.5, 0.5, 0.0), 0.004), sparse])
    q = np.concatenate([_blob(70, 33, (0.5, 0.5, 0.0), 0.004), sparse + [0.0, 0.0, 0.001], _sheet(5, 34, z=3.0, lo=(20.0, 20.0), hi=(21.0, 21.0))])
    rng = np.random.default_rng(35)
    q, ref = q[rng.permutation(len(q))], ref[rng.permutation(len(ref))]
    with _engine(q, ref) as e:
        off, idx, d2 = e.radius_search(0, 1, 0.05)
        lens = np.diff(off)
        assert lens.max() == 3000 > tile and (lens == 0).sum() == 5 and (lens == 1).sum() >= 150
        _same((off, idx, d2), S.radius(q, ref, 0.05), "long rows")
        # the blob alone in slot 1, every row of the self search is long
        blob = _blob(1500, 36, (0.0, 0.0, 0.0), 0.004)
        e.upload(1, blob)
        off, idx, d2 = e.radius_search(1, 1, 0.5)
        assert (np.diff(off) == 1500).all() and 1500 > tile
        _same((off, idx, d2), S.radius(blob, blob, 0.5), "all rows long")


# ---- 5. frame edges --------------------------------------------------------------------------------------------------------------------
def test_queries_inside_at_the_edge_of_and_far_outside_the_reference_frame():
    cell = 0.05
    ref = _sheet(3000, 41)
    inside = _sheet(200, 42, z=0.01)
    edge = _sheet(100, 43, z=0.0, lo=(1.0, 0.0), hi=(1.0 + cell, 1.0))       # within one cell beyond the frame's +x face
    edge2 = _sheet(100, 44, z=0.0, lo=(-cell, -cell), hi=(0.0, 0.0))         # ... and beyond the -x / -y corner
    far = _sheet(50, 45, z=0.0, lo=(1.0 + 100 * cell, 0.0), hi=(1.0 + 101 * cell, 1.0))  # 100 cell widths outside
    q = np.concatenate([inside, edge, edge2, far])
    with _engine(q, ref, cell=cell) as e:
        order = S.ordered(q, ref)
        off, idx, d2 = e.radius_search(0, 1, cell)
        _same((off, idx, d2), S.radius_from(order, cell), "frame edges radius")
        lens = np.diff(off)
        assert (lens[-50:] == 0).all() and lens[:200].mean() > 5 and lens[200:300].max() > 0 and lens[300:400].max() > 0
        for k in (1, 20):
            _same(e.knn_search(0, 1, k), S.knn_from(order, k), f"frame edges knn k={k}")
        cnt, hi, hd = e.hybrid_search(0, 1, cell, 10)
        _same((cnt, hi, hd), S.hybrid_from(order, cell, 10), "frame edges hybrid")
        assert (cnt[-50:] == 0).all()


# ---- 6. mask -----------------------------------------------------------------------------------------------------------------------------
def test_mask_gives_empty_or_padded_rows_and_leaves_the_others():
    a, b = _sheet(1000, 51), _sheet(1200, 52, z=0.01)
    mask = (np.random.default_rng(53).random(1000) < 0.4).astype(np.uint8)
    with _engine(a, b) as e:
        full_k = e.knn_search(0, 1, 8)
        full_r = e.radius_search(0, 1, 0.05)
        full_h = e.hybrid_search(0, 1, 0.05, 6)
        _same(e.knn_search(0, 1, 8, mask=mask), S.mask_rows_knn(*full_k, mask), "masked knn")
        _same(e.radius_search(0, 1, 0.05, mask=mask), S.mask_rows_csr(*full_r, mask), "masked radius")
        cnt, hi, hd = e.hybrid_search(0, 1, 0.05, 6, mask=mask)
        _same((hi, hd), S.mask_rows_knn(full_h[1], full_h[2], mask), "masked hybrid")
        assert np.array_equal(cnt, full_h[0] * (mask != 0))
        none = np.zeros(1000, np.uint8)
        off, idx, d2 = e.radius_search(0, 1, 0.05, mask=none)
        assert off[-1] == 0 and (off == 0).all() and len(idx) == len(d2) == 0
        assert (e.knn_search(0, 1, 3, mask=none)[0] == -1).all() and (e.hybrid_search(0, 1, 0.05, 3, mask=none)[0] == 0).all()
        with pytest.raises(ValueError):
            e.knn_search(0, 1, 3, mask=np.ones(999, np.uint8))


# ---- 7. protocol and errors ----------------------------------------------------------------------------------------------------------------
def test_sizing_and_filling_calls_agree_and_a_short_capacity_writes_nothing():
    a, b = _sheet(500, 61), _sheet(600, 62, z=0.01)
    with _engine(a, b) as e:
        L, ctx = e._L, e._ctx
        off0 = np.empty(501, np.int64)
        total = C.c_int64(-7)
        assert L.me_radius_search(ctx, 0, 1, 0.05, 0, off0.ctypes.data, 0, 0, 0, C.byref(total)) == 0
        t = total.value
        assert t == off0[-1] > 0 and np.array_equal(off0, e.radius_search(0, 1, 0.05, counts_only=True))
        off1 = np.empty(501, np.int64)
        idx, d2 = np.empty(t, np.int32), np.empty(t, np.float64)
        total2 = C.c_int64(-7)
        assert L.me_radius_search(ctx, 0, 1, 0.05, 0, off1.ctypes.data, idx.ctypes.data, d2.ctypes.data, t, C.byref(total2)) == 0
        assert total2.value == t and np.array_equal(off0, off1)
        _same((off1, idx, d2), S.radius(a, b, 0.05), "filling call")
        # one entry short: ME_ERR_ARG, the message names the needed total, and no output is touched
        off2, idx2, d22 = np.full(501, -5, np.int64), np.full(t, -5, np.int32), np.full(t, -5.0)
        total3 = C.c_int64(-7)
        rc = L.me_radius_search(ctx, 0, 1, 0.05, 0, off2.ctypes.data, idx2.ctypes.data, d22.ctypes.data, t - 1, C.byref(total3))
        assert rc == ME_ERR_ARG and str(t) in L.me_last_error(ctx).decode()
        assert (off2 == -5).all() and (idx2 == -5).all() and (d22 == -5.0).all() and total3.value == -7
        # idx and d2 come together
        assert L.me_radius_search(ctx, 0, 1, 0.05, 0, 0, idx.ctypes.data, 0, t, C.byref(total)) == ME_ERR_ARG
        assert L.me_radius_search(ctx, 0, 1, 0.05, 0, 0, 0, d2.ctypes.data, t, C.byref(total)) == ME_ERR_ARG
        assert L.me_knn_search(ctx, 0, 1, 3, 0, idx.ctypes.data, 0) == ME_ERR_ARG
        assert L.me_hybrid_search(ctx, 0, 1, 0.05, 3, 0, 0, 0, d2.ctypes.data) == ME_ERR_ARG


def test_bad_arguments_fail_loudly():
    from cloud_map_evaluation_amd.engine import Engine, MapEvalError

    a, b = _sheet(100, 71), _sheet(100, 72)
    with _engine(a, b) as e:
        for k in (0, -1, 41):
            with pytest.raises(MapEvalError, match="k must be"):
                e.knn_search(0, 1, k)
            with pytest.raises(MapEvalError, match="max_nn must be"):
                e.hybrid_search(0, 1, 0.1, k)
        for r in (0.0, -0.1, float("nan"), float("inf")):
            with pytest.raises(MapEvalError, match="radius must be"):
                e.radius_search(0, 1, r)
            with pytest.raises(MapEvalError, match="radius must be"):
                e.hybrid_search(0, 1, r, 3)
        L, ctx = e._L, e._ctx
        idx, d2 = np.empty((100, 3), np.int32), np.empty((100, 3), np.float64)
        total = C.c_int64(0)
        for qs, rs in ((2, 0), (0, 2), (-1, 1), (1, -1)):
            assert L.me_knn_search(ctx, qs, rs, 3, 0, idx.ctypes.data, d2.ctypes.data) == ME_ERR_ARG
            assert "bad slot" in L.me_last_error(ctx).decode()
            assert L.me_hybrid_search(ctx, qs, rs, 0.1, 3, 0, 0, idx.ctypes.data, d2.ctypes.data) == ME_ERR_ARG
            assert L.me_radius_search(ctx, qs, rs, 0.1, 0, 0, 0, 0, 0, C.byref(total)) == ME_ERR_ARG
    # an empty cloud: me_upload_cloud rejects it (ME_ERR_ARG), so the slot it was offered to holds no cloud, and every search that
    # names that slot, as query or as reference, fails with ME_ERR_STATE as the header says
    with Engine(0) as e:
        e.upload(0, a)
        assert e._L.me_upload_cloud(e._ctx, 1, a.ctypes.data, 0, 0, 0.0) == ME_ERR_ARG and "empty" in e._L.me_last_error(e._ctx).decode()
        assert e.size(1) <= 0
        idx, d2 = np.full((100, 3), -5, np.int32), np.full((100, 3), -5.0)
        total = C.c_int64(-7)
        for qs, rs in ((0, 1), (1, 0), (1, 1)):
            assert e._L.me_knn_search(e._ctx, qs, rs, 3, 0, idx.ctypes.data, d2.ctypes.data) == ME_ERR_STATE
            assert "not uploaded" in e._L.me_last_error(e._ctx).decode()
            assert e._L.me_hybrid_search(e._ctx, qs, rs, 0.1, 3, 0, 0, idx.ctypes.data, d2.ctypes.data) == ME_ERR_STATE
            assert e._L.me_radius_search(e._ctx, qs, rs, 0.1, 0, 0, 0, 0, 0, C.byref(total)) == ME_ERR_STATE
        assert (idx == -5).all() and (d2 == -5.0).all() and total.value == -7
        _same(e.knn_search(0, 0, 3), S.knn(a, a, 3), "the uploaded slot still serves")


# ---- 8. state -------------------------------------------------------------------------------------------------------------------------------
def test_searches_leave_everything_resident_intact_and_repeat_byte_for_byte():
    """the header's rule: the searches walk the octree and re-index nothing, so the 1-NN results, the normals and the MME results of
    both slots are still fetchable and unchanged after searches at radii unrelated to the index's cell"""
    a, b = _sheet(3000, 81), _sheet(2500, 82, z=0.01)
    with _engine(a, b, cell=0.05) as e:
        e.estimate_normals(0, 20)
        e.estimate_normals(1, 10)
        e.mme(0, 0.05, 5)
        e.mme(1, 0.05, 5)
        e.nn1(0, 1)
        e.nn1(1, 0)  # (last: every earlier call is free to re-index, nothing after this one may)
        before = [e.nn_fetch(0), e.nn_fetch(1), (e.get_normals(0), e.get_normals(1)), e.mme_fetch(0), e.mme_fetch(1)]
        first = []
        for qs, rs in ((0, 1), (1, 0), (0, 0), (1, 1)):
            first.append(e.knn_search(qs, rs, 20))
            first.append(e.radius_search(qs, rs, 0.13))
            first.append(e.hybrid_search(qs, rs, 0.011, 9))
        after = [e.nn_fetch(0), e.nn_fetch(1), (e.get_normals(0), e.get_normals(1)), e.mme_fetch(0), e.mme_fetch(1)]
        for x, y in zip(before, after):
            for u, v in zip(x, y):
                assert u.tobytes() == v.tobytes()
        again = []
        for qs, rs in ((0, 1), (1, 0), (0, 0), (1, 1)):
            again.append(e.knn_search(qs, rs, 20))
            again.append(e.radius_search(qs, rs, 0.13))
            again.append(e.hybrid_search(qs, rs, 0.011, 9))
        for x, y in zip(first, again):
            for u, v in zip(x, y):
                assert u.tobytes() == v.tobytes()
        _same(first[1], S.radius(a, b, 0.13), "radius 0->1 at 2.6 cells")


# ---- 9. one case at scale -----------------------------------------------------------------------------------------------------------------
def test_a_million_points_against_brute_force_on_a_subsample(capsys):
    """10^6 + 10^6 points on two sheets of 10 m x 10 m (spacing ~1 cm).  k = 20 on all queries, judged on 2000 random ones whose model
    rows come from brute force over the whole reference; the radius lists (r = 3.1 cm, about 30 neighbours) with a mask of the same 2000
    queries, judged on all of them.  Prints the kernel times (me_timer_get) of the searches."""
    n = 1_000_000
    a = _sheet(n, 91, lo=(0.0, 0.0), hi=(10.0, 10.0))
    b = _sheet(n, 92, z=0.01, lo=(0.0, 0.0), hi=(10.0, 10.0))
    pick = np.sort(np.random.default_rng(93).choice(n, 2000, replace=False))
    mask = np.zeros(n, np.uint8)
    mask[pick] = 1
    r = 0.031
    mi, md, rows = S.rows_bruteforce(a[pick], b, 20, r, threads=16)
    with _engine(a, b) as e:
        e.timers_enable(True)
        ki, kd = e.knn_search(0, 1, 20)
        off, idx, d2 = e.radius_search(0, 1, r, mask=mask)
        times = {name: e.timer(name) for name in ("knn_search", "radius_count", "radius_fill", "radius_sort")}
    with capsys.disabled():
        print("\n[search at 10^6] " + ", ".join(f"{k} {v[0]:.2f} ms / {v[1]} launches" for k, v in times.items()))
    assert np.array_equal(ki[pick], mi) and np.array_equal(_bits(kd[pick]), _bits(md))
    lens = np.diff(off)
    assert lens[mask == 0].sum() == 0 and off[-1] == len(idx) == sum(len(i) for i, _ in rows)
    assert 20 < lens[pick].mean() < 45
    for p, (ri, rd) in zip(pick, rows):
        assert np.array_equal(idx[off[p]:off[p + 1]], ri) and np.array_equal(_bits(d2[off[p]:off[p + 1]]), _bits(rd))
