"""The inputs of the preparation / output edge suite (tests/test_prep_edges_cpu.py, tests/test_gpu_prep_edges.py).  Every case is a
dict with a "name" and a "check": a function of no arguments that asserts, on the numpy model (tests/_prep_ref.py) alone, that the edge
the case is named after is present in its data.  These asserts are conditions, not measurements: a case that misses its edge fails on
the CPU.  Every cloud is shuffled with a fixed seed, so that no sorted order is the cloud's order."""
import numpy as np

import _prep_ref as R

SIZES = (1, 2, 255, 256, 257, 4097)
SURVEY_SHIFT = (-4.5e5, 5.2e6, -300.0)  # integers: a dyadic lattice shifted by them stays exact
FACE_KS = (1, 2, 3, 5, 8)
C_MAX = float(np.nextafter(2097151.5, 0.0))  # with the minimum at 0 and vs = 1: the largest coordinate whose index is still 2097151
BBOX_SIZES = (262144, 262145)  # a 1024 x 256 grid filled exactly, and the first size at which its block 0 takes a second trip
JET_RATIOS = (0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0)  # e / dis at which one channel of Jet sits on a breakpoint
DIS = (0.25, 4.0)
GATE = 0.75
GATES = ((-1.0, 0), (0.0, 0), (0.0, 1), (GATE, 0), (GATE, 1))


def _rng(*key):
    return np.random.default_rng([20240607, *[int(k) for k in key]])


def _shuffled(a, *key):
    return np.ascontiguousarray(np.asarray(a, np.float64)[_rng(*key, 99).permutation(len(a))])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _nbrs(v):
    return [float(np.nextafter(v, -np.inf)), float(v), float(np.nextafter(v, np.inf))]


# =============================================================================================================================================
# down-sample
# =============================================================================================================================================
def _ds_case(name, xyz, vs, check, normals=None, **extra):
    return dict(name=name, xyz=xyz, vs=vs, normals=normals, check=check, **extra)


def ds_size_cases(n):
    """V = 1, V = n and an ordinary mix at n points."""
    r = _rng(1, n)
    one = r.random((n, 3)) * 0.25  # spread < vs / 2 = 0.5: one voxel whatever the minimum is
    per = np.stack([np.arange(n, dtype=np.float64), r.random(n) * 0.25, r.random(n) * 0.25], axis=1)
    mix = r.random((n, 3)) * 4.0
    one, per, mix = _shuffled(one, 1, n), _shuffled(per, 2, n), _shuffled(mix, 3, n)

    def chk(xyz, want_v):
        def f():
            ref = R.downsample(xyz, 1.0)
            assert len(ref["points"]) == want_v(len(xyz)) and ref["counts"].sum() == len(xyz)
        return f

    cs = [_ds_case(f"size/{n}/one_voxel", one, 1.0, chk(one, lambda m: 1)),
          _ds_case(f"size/{n}/one_point_per_voxel", per, 1.0, chk(per, lambda m: m))]
    if n >= 255:
        def chk_mix():
            ref = R.downsample(mix, 1.0)
            assert 27 <= len(ref["points"]) <= 125 and ref["counts"].max() > 1
        cs.append(_ds_case(f"size/{n}/mix", mix, 1.0, chk_mix))
    return cs


def _face_points(shift):
    """vs = 0.5, minimum exactly `shift`, so the origin is shift - 0.25: points at origin + k vs and one ulp below, per axis and on the
    corner, among 200 points on the 2^-10 lattice.  -> (xyz, tags): tags[i] = (axis or 3 for the corner, k, on_face)."""
    r = _rng(2)
    shift = np.asarray(shift, np.float64)
    pts, tags = [shift.copy()], [(-1, 0, False)]
    fill = np.floor(r.random((200, 3)) * 4096.0) / 1024.0  # [0, 4) on the 2^-10 lattice
    for q in fill:
        pts.append(shift + q)
        tags.append((-1, 0, False))
    for k in FACE_KS:
        c = -0.25 + k * 0.5
        for a in range(3):
            q = np.floor(r.random(3) * 4096.0) / 1024.0 + 1.0 / 2048.0  # the other two coordinates: strictly inside their voxels
            p = shift + q
            p[a] = shift[a] + c
            pts.append(p.copy())
            tags.append((a, k, True))
            p[a] = np.nextafter(p[a], -np.inf)
            pts.append(p.copy())
            tags.append((a, k, False))
        corner = shift + c
        pts.append(corner.copy())
        tags.append((3, k, True))
        pts.append(np.nextafter(corner, -np.inf))
        tags.append((3, k, False))
    return np.array(pts), tags


def ds_face_case(shift=(0.0, 0.0, 0.0), with_normals=False):
    xyz0, tags0 = _face_points(shift)
    perm = _rng(3, 99).permutation(len(xyz0))
    xyz, tags = np.ascontiguousarray(xyz0[perm]), [tags0[i] for i in perm]
    nrm = None
    if with_normals:
        v = _rng(4).normal(size=xyz.shape)
        nrm = v / np.linalg.norm(v, axis=1, keepdims=True)

    def check():
        lo = R.bbox(xyz)[0]
        assert np.array_equal(lo, np.asarray(shift, np.float64))  # the minimum is exactly the shift: origin = shift - 0.25
        assert np.array_equal((lo - 0.25) + 0.5, lo + 0.25)        # ... and the lattice is exact at this magnitude
        f = R.voxel_index(xyz, 0.5)
        for (a, k, on), fi in zip(tags, f):
            axes = range(3) if a == 3 else ([a] if a >= 0 else [])
            for d in axes:  # a face point belongs to the UPPER voxel; one ulp below, to the lower one where fp64 can tell them apart
                if on:
                    assert fi[d] == k
                elif k >= 2:
                    assert fi[d] == k - 1
        for d in range(3):
            for k in FACE_KS:
                assert (f[:, d] == k).sum() >= 1 and (f[:, d] == k - 1).sum() >= 1
        ref = R.downsample(xyz, 0.5, nrm)
        assert ref is not R.REFUSED and ref["counts"].max() > 1

    name = "face/" + ("survey" if any(shift) else "origin") + ("/normals" if with_normals else "")
    return _ds_case(name, xyz, 0.5, check, normals=nrm)


def ds_division_case():
    """vs = 0.1, minimum 0: points next to the faces at which floor(d / vs) and floor(d * (1 / vs)) name different voxels.  The
    library divides, as Open3D does; a multiplication by the reciprocal would move these points across their face."""
    vs = 0.1
    origin = 0.0 - vs * 0.5
    pts = [np.zeros(3)]
    r = _rng(16)
    for axis in range(3):
        found = 0
        for k in range(1, 4000):
            c = origin + k * vs
            for p in (float(np.nextafter(np.nextafter(c, -np.inf), -np.inf)), *_nbrs(c), float(np.nextafter(np.nextafter(c, np.inf), np.inf))):
                d = p - origin
                if np.floor(d / vs) != np.floor(d * (1.0 / vs)):
                    q = r.random(3) * 3.0 + 0.01
                    q[axis] = p
                    pts.append(q)
                    found += 1
            if found >= 8:
                break
    xyz = _shuffled(np.array(pts), 16)

    def check():
        assert (R.bbox(xyz)[0] == 0.0).all()
        f = R.voxel_index(xyz, vs)
        with_reciprocal = np.floor((xyz - (R.bbox(xyz)[0] - vs * 0.5)) * (1.0 / vs))
        for d in range(3):
            assert (f[:, d] != with_reciprocal[:, d]).sum() >= 8
        assert f.max() <= 4000 and R.downsample(xyz, vs) is not R.REFUSED

    return _ds_case("face/division", xyz, vs, check)


def _order_sensitive(n, key):
    """coordinates random * 2^-k, k uniform in 0 .. 40, all inside [0, 0.5)"""
    r = _rng(5, key)
    return r.random((n, 3)) * 0.5 * np.exp2(-r.integers(0, 41, size=(n, 3)).astype(np.float64))


def ds_sum_order_case(among=False, with_normals=False):
    big = _order_sensitive(5000, 0)
    xyz = big
    if among:  # the same voxel among 300 ordinary ones
        xyz = np.concatenate([big, 2.0 + _rng(6).random((1500, 3)) * 7.0])
    xyz = _shuffled(xyz, 7, among)
    nrm = _order_sensitive(len(xyz), 1) - 0.125 if with_normals else None

    def check():
        ref = R.downsample(xyz, 1.0, nrm)
        v = int(np.argmax(ref["counts"]))
        assert ref["counts"][v] == 5000 and v == 0
        assert len(ref["counts"]) == 1 if not among else len(ref["counts"]) >= 300
        members = np.nonzero(ref["voxel_of"] == v)[0]
        assert (np.diff(members) > 0).all()
        for arr, got in ((xyz, ref["points"]),) + (((nrm, ref["normals"]),) if with_normals else ()):
            seq = np.zeros(3)
            for i in members:  # the expected mean, stated once more: one addition per point, in index order
                seq = seq + arr[i]
            assert np.array_equal(_bits(seq / 5000.0), _bits(got[v]))
            srt = np.zeros(3)
            for d in range(3):
                s = 0.0
                for x in np.sort(arr[members, d]):
                    s = s + x
                srt[d] = s
            assert (_bits(srt / 5000.0) != _bits(got[v])).any(), "the sorted-by-value sum gives the same bits: the case proves nothing"
            back = np.zeros(3)
            for i in members[::-1]:
                back = back + arr[i]
            assert (_bits(back / 5000.0) != _bits(got[v])).any(), "the backwards sum gives the same bits"

    name = "sum_order/" + ("among_300" if among else "alone") + ("/normals" if with_normals else "")
    return _ds_case(name, xyz, 1.0, check, normals=nrm)


def ds_key_field_case(bump_axis=None):
    """vs = 1, minimum 0: integer coordinate c has index c.  Indices reach 2097151 on every axis while the others are 0, and the pairs
    (fy=1, fz=0) / (fy=0, fz=2097151) and (fx=1, 0, 0) / (0, 2097151, 2097151) order the voxels across a 21-bit field.
    bump_axis: that axis' largest coordinate one ulp up (2097151.5: index 2097152) -> refused."""
    M = C_MAX
    base = [(0, 0, 0), (M, 0, 0), (0, M, 0), (0, 0, M), (M, M, M), (0, 1, 0), (1, 0, 0), (0, M, M), (M, 0, M), (M, M, 0),
            (2097151.0, 0, 0), (0, 2097151.0, 0.25), (0.25, 0, 2097151.0),  # second members of three of the voxels above
            (0, 1, 0.25), (1, 0.25, 0), (5, 7, 11), (5.25, 7, 11)]
    xyz = np.array(base, np.float64)
    if bump_axis is not None:
        xyz[1 + bump_axis, bump_axis] = 2097151.5
    xyz = _shuffled(xyz, 8)

    def check():
        f = R.voxel_index(xyz, 1.0)
        ref = R.downsample(xyz, 1.0)
        if bump_axis is not None:
            assert f[:, bump_axis].max() == 2097152.0 and ref is R.REFUSED
            other = [d for d in range(3) if d != bump_axis]
            assert f[:, other].max() == 2097151.0
            return
        assert ref is not R.REFUSED
        for d in range(3):
            assert (f[:, d] == 2097151.0).sum() >= 3 and (f[:, d] == 0.0).sum() >= 3
        vox = {tuple(t) for t in ref["index"].tolist()}
        assert {(0, 1, 0), (0, 0, 2097151), (1, 0, 0), (0, 2097151, 2097151)} <= vox
        assert ref["counts"].max() >= 2

    return _ds_case("key_fields" if bump_axis is None else f"limit/axis{bump_axis}", xyz, 1.0, check)


def ds_huge_voxel_case():
    xyz = _shuffled(_rng(9).random((257, 3)) * 10.0 - 5.0, 9)

    def check():
        ref = R.downsample(xyz, 1e300)
        assert len(ref["points"]) == 1 and (ref["index"] == 0).all()

    return _ds_case("huge_voxel", xyz, 1e300, check)


def bbox_variants(n):
    """Where the single minimum of each axis sits: (ix, iy, iz), three different wavefronts each."""
    pos = [0, 255, 256, n - 1] if n == 262144 else [0, 255, 256, 262143, 262144]
    return [tuple(pos[(s + d) % len(pos)] for d in range(3)) for s in range(len(pos))]


def ds_bbox_case(n, where):
    """n points on the 1/8 lattice in [1, 65), the only coordinate below 1 of each axis (a 0) at the index `where` names.  vs = 4:
    a box that misses one of the minima moves the origin by 1 and with it a quarter of the points to another voxel."""
    xyz = np.floor(_rng(10, n).random((n, 3)) * 512.0) / 8.0 + 1.0
    for d in range(3):
        xyz[where[d], d] = 0.0

    def check():
        for d in range(3):
            assert np.nonzero(xyz[:, d] < 1.0)[0].tolist() == [where[d]]
        assert len({w // 64 for w in where}) == 3  # three different wavefronts
        ref = R.downsample(xyz, 4.0)
        moved = xyz.copy()
        for d in range(3):
            moved[where[d], d] = 1.0
            assert not np.array_equal(R.voxel_index(moved, 4.0)[:, d], ref["index"][:, d])  # the box shows in the voxels
            moved[where[d], d] = 0.0

    return _ds_case(f"bbox/{n}/{'-'.join(map(str, where))}", xyz, 4.0, check, where=where)


def ds_small_cases():
    """every down-sample case but the 262 144-point ones"""
    cs = []
    for n in SIZES:
        cs += ds_size_cases(n)
    cs += [ds_face_case(), ds_face_case(SURVEY_SHIFT), ds_face_case(with_normals=True), ds_division_case(),
           ds_sum_order_case(), ds_sum_order_case(among=True), ds_sum_order_case(among=True, with_normals=True),
           ds_key_field_case(), ds_huge_voxel_case()]
    return cs


def ds_refused_cases():
    return [ds_key_field_case(bump_axis=a) for a in range(3)]


BAD_VOXEL_SIZES = (float("inf"), float("nan"), 0.0, -1.0)


# =============================================================================================================================================
# transform
# =============================================================================================================================================
def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def matrices():
    rigid = np.eye(4)
    rigid[:3, :3] = _rot(0.3, -1.1, 2.0)
    rigid[:3, 3] = (1.5, -20.25, 0.3)
    shear = np.array([[2.0, 0.5, 0.0, 1.0], [0.0, 0.75, 0.25, -2.0], [0.125, 0.0, 3.0, 0.5], [0.0, 0.0, 0.0, 1.0]])
    proj2 = rigid.copy()
    proj2[3] = (0.0, 0.0, 0.0, 2.0)
    projx = np.eye(4)
    projx[:3, :3] = _rot(-0.7, 0.2, 0.4)
    projx[:3, 3] = (0.1, 0.2, -0.3)
    projx[3] = (0.125, 0.0, 0.0, 1.0)
    return {"rigid": rigid, "scale_shear": shear, "proj_w2": proj2, "proj_x": projx}


def identities():
    neg = np.eye(4)
    neg[neg == 0.0] = -0.0
    return {"identity": np.eye(4), "identity_negative_zeros": neg}


W_ZERO = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])  # h3 = x


def tf_cloud(n):
    """x in [-4, 8] with both ends present from n = 2 on (h3 = 0.125 x + 1 of proj_x stays in [0.5, 2]); y, z in [-3, 3)"""
    r = _rng(11, n)
    xyz = np.stack([r.random(n) * 12.0 - 4.0, r.random(n) * 6.0 - 3.0, r.random(n) * 6.0 - 3.0], axis=1)
    xyz[0, 0] = 8.0
    if n > 1:
        xyz[1, 0] = -4.0
    return _shuffled(xyz, 11, n)


def tf_cases():
    cs = []
    for n in SIZES:
        xyz = tf_cloud(n)
        for name, T in matrices().items():
            def check(xyz=xyz, T=T, name=name, n=n):
                out = R.transform(xyz, T)
                assert np.isfinite(out).all() and not np.array_equal(out, xyz)
                assert not (np.signbit(xyz) & (xyz == 0)).any()
                if name == "proj_x":
                    w = R.homogeneous_w(xyz, T)
                    assert w.min() >= 0.5 and w.max() == 2.0 and (n == 1 or w.min() == 0.5)
                if name == "proj_w2":
                    assert (R.homogeneous_w(xyz, T) == 2.0).all()
            cs.append(dict(name=f"transform/{name}/{n}", xyz=xyz, T=T, check=check))
    return cs


def tf_w_zero_case(all_nan=False):
    """one point with h3 = x = 0: (0 / 0, 1.25 / 0, -0.5 / 0) = (NaN, inf, -inf); all_nan: the point is the origin, 0 / 0 three times,
    the one result that fmin / fmax would drop from a bounding box without a word"""
    xyz = tf_cloud(257).copy()
    xyz[100] = (0.0, 0.0, 0.0) if all_nan else (0.0, 1.25, -0.5)

    def check():
        out = R.transform(xyz, W_ZERO)
        bad = ~np.isfinite(out).all(axis=1)
        assert np.nonzero(bad)[0].tolist() == [100] and (xyz[:, 0] == 0.0).sum() == 1
        assert np.isnan(out[100]).all() == all_nan and np.isinf(out[100]).any() != all_nan
        assert np.isfinite(np.delete(out, 100, axis=0)).all()

    return dict(name="transform/w_zero" + ("_all_nan" if all_nan else ""), xyz=xyz, T=W_ZERO, check=check)


# =============================================================================================================================================
# render_distance
# =============================================================================================================================================
def planted_d2(dis):
    p = []
    for r in JET_RATIOS:
        p += _nbrs(r * dis)
    p += [float(np.nextafter(dis, np.inf)), 100.0 * dis, -1.0]  # the clamp (d2 == dis is among the ratios) and a non-query entry
    p += _nbrs(GATE) + _nbrs(GATE * GATE)
    return list(dict.fromkeys(p))  # distinct, order kept


def rd_case(n, dis):
    r = _rng(12, n, int(dis * 4))
    plant = planted_d2(dis)[:n]
    rest = r.random(n - len(plant)) * 1.5 * dis + 2.0 ** -20
    d2 = _shuffled(np.array(plant + rest.tolist()), 12, n)
    xyz = r.random((n, 3)) * 4.0

    def check():
        assert len(np.unique(_bits(d2))) == n  # all distinct: a colour written to the wrong point shows
        if n < len(planted_d2(dis)):
            return
        q = np.where(d2 > dis, dis, d2) / dis
        for ratio in JET_RATIOS:  # on the breakpoint and on both sides of it
            lo, mid, hi = _nbrs(ratio * dis)
            assert (d2 == mid).any() and (d2 == lo).any() and (d2 == hi).any()
            assert (q == ratio).any()
            args = R.jet_args(np.array([ratio]))[0]  # the odd multiples of 1/8 put a channel's argument ON a breakpoint of jet_base
            assert any(a in R.JET_BREAKS for a in args) == (ratio in (0.125, 0.375, 0.625, 0.875))
        assert (d2 == dis).any() and (d2 == np.nextafter(dis, np.inf)).any() and (d2 == 100 * dis).any() and (d2 == -1.0).any()
        for g in (GATE, GATE * GATE):
            for v in _nbrs(g):
                assert (d2 == v).any()
        assert R.inliers(d2, GATE, 0).sum() != R.inliers(d2, GATE, 1).sum()
        assert 0 < R.inliers(d2, 0.0, 1).sum() < R.inliers(d2, 0.0, 0).sum()  # the negatives; the negatives and the zero

    return dict(name=f"render_distance/{n}/dis{dis}", xyz=xyz, d2=d2, dis=dis, check=check)


def rd_cases():
    return [rd_case(n, dis) for n in SIZES for dis in DIS]


# =============================================================================================================================================
# render_entropy
# =============================================================================================================================================
E_MIN, E_MAX = -7.0, -5.0  # the extremes of the range, carried by INVALID points


def re_body_case(n, tail=False):
    """negative entropies in [-6.5, -5.5]; valid +0.0 and -0.0; the range's extremes on invalid points at the first and the last cloud
    index (tail: both at indices >= 262144, the second trip of the 1024-block range kernel)"""
    r = _rng(13, n)
    ent = -6.5 + r.random(n)
    valid = r.random(n) < 0.7
    i_min, i_max = (n - 2, n - 1) if tail else (0, n - 1)
    z0, z1, inner_lo, inner_hi = n // 3, n // 2, n // 5, n // 7
    ent[[z0, z1]] = (0.0, -0.0)
    valid[[z0, z1]] = True
    ent[[inner_lo, inner_hi]] = (-6.5, -5.5)  # the extremes among the VALID points: the range a validity-aware kernel would find
    valid[[inner_lo, inner_hi]] = True
    ent[[i_min, i_max]] = (E_MIN, E_MAX)
    valid[[i_min, i_max]] = False
    xyz = r.random((n, 3)) * 4.0

    def check():
        ref = R.render_entropy(xyz, ent, valid)
        assert (ref["min_abs"], ref["max_abs"]) == (5.0, 7.0)
        nzv = ent[valid & (ent != 0)]
        assert (abs(nzv.max()), abs(nzv.min())) == (5.5, 6.5)  # skipping the invalid points would give another range
        assert np.signbit(ent[z1]) and not np.signbit(ent[z0]) and ent[z0] == 0 and ent[z1] == 0
        assert 0 < ref["n_valid"] < n and np.array_equal(ref["xyz"], xyz[valid])
        zeros = np.isin(np.nonzero(valid)[0], [z0, z1])
        assert np.isnan(ref["ne"][zeros]).all() and (ref["rgb"][zeros] == 0.0).all()  # coloured (through NaN), not in the range
        assert np.isfinite(ref["ne"][~zeros]).all()
        ex = R.jet_exact_mask(ref["ne"])
        assert ex[~zeros].any() and not ex[~zeros].all()  # both bounds of the comparison are exercised
        if tail:
            assert min(i_min, i_max) >= 262144

    return dict(name=f"render_entropy/body/{n}" + ("/tail" if tail else ""), xyz=xyz, ent=ent, valid=valid, check=check)


def re_tiny_cases():
    xyz = _rng(14).random((2, 3))
    e1, v1 = np.array([-6.0]), np.array([True])
    e2, v2 = np.array([E_MIN, -5.5]), np.array([False, True])

    def c1():
        ref = R.render_entropy(xyz[:1], e1, v1)
        assert ref["min_abs"] == ref["max_abs"] == 6.0 and np.isnan(ref["ne"]).all()

    def c2():
        ref = R.render_entropy(xyz, e2, v2)
        assert (ref["min_abs"], ref["max_abs"], ref["n_valid"]) == (5.5, 7.0, 1) and ref["ne"][0] == 0.0

    return [dict(name="render_entropy/1", xyz=xyz[:1], ent=e1, valid=v1, check=c1),
            dict(name="render_entropy/2", xyz=xyz, ent=e2, valid=v2, check=c2)]


def re_degenerate_cases(n=257):
    r = _rng(15, n)
    xyz = r.random((n, 3)) * 4.0
    some = r.random(n) < 0.6
    body = -6.5 + r.random(n)
    equal = np.where(r.random(n) < 0.2, 0.0, -6.25)
    cs = []

    def add(name, ent, valid, cond):
        def check():
            cond(R.render_entropy(xyz, ent, valid))
        cs.append(dict(name=f"render_entropy/{name}", xyz=xyz, ent=ent, valid=valid, check=check))

    def c_equal(ref):
        assert ref["min_abs"] == ref["max_abs"] == 6.25 and np.isnan(ref["ne"]).all() and (ref["rgb"] == 0.0).all()
        assert ref["n_valid"] > 0 and (equal == 0).any() and (equal != 0).any()

    def c_none(ref):
        assert ref["n_valid"] == 0 and ref["xyz"].shape == (0, 3) and ref["rgb"].shape == (0, 3)
        assert ref["min_abs"] == abs(body.max()) and ref["max_abs"] == abs(body.min()) and ref["min_abs"] < ref["max_abs"]

    def c_zero(ref):
        assert ref["min_abs"] == np.inf and ref["max_abs"] == np.inf and ref["n_valid"] > 0
        assert np.isnan(ref["ne"]).all() and (ref["rgb"] == 0.0).all()

    def c_all(ref):
        assert ref["n_valid"] == n and np.isfinite(ref["ne"]).all()
        assert ref["ne"].min() == 0.0 and abs(ref["ne"].max() - 1.0) < 1e-12

    add("all_equal", equal, some, c_equal)
    add("no_valid", body, np.zeros(n, bool), c_none)
    add("no_nonzero", np.where(r.random(n) < 0.5, 0.0, -0.0), some, c_zero)
    add("all_valid", body, np.ones(n, bool), c_all)
    return cs


RE_TAIL_N = 262147


def re_small_cases():
    return re_tiny_cases() + [re_body_case(n) for n in SIZES if n >= 255] + re_degenerate_cases()


def all_small_cases():
    return ds_small_cases() + ds_refused_cases() + tf_cases() + [tf_w_zero_case(), tf_w_zero_case(all_nan=True)] + rd_cases() + re_small_cases()
