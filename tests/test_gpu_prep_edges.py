"""Cloud preparation and output on the MI355X at their exact edges: me_voxel_downsample / _into (csrc/me_voxel.hip), the upload with T,
me_transform_cloud and the bounding box (csrc/me_index.hip), me_render_distance / me_render_entropy fed through me_set_nn_result /
me_set_mme_result (csrc/me_render.hip), against the numpy model of tests/_prep_ref.py on the cases of tests/_prep_edge_cases.py (each
of which proves on the CPU that its edge is in its data: tests/test_prep_edges_cpu.py).  The largest input has 262 147 points.

EXACT (np.array_equal on the uint64 views): every down-sampled position and averaged normal, every transformed point through the
three routes, every distance colour, every inlier flag, the entropy renderer's points, count, min_abs and max_abs, and every entropy
colour channel that a last-place difference of `log` cannot move (_prep_ref.jet_exact_mask).  WITHIN atol = 1e-9, the bound
tests/test_gpu_render.py holds for the same kernel: the other entropy colour channels (the device's log against the host's)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _prep_edge_cases as E  # noqa: E402
import _prep_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ME_ERR_ARG, ME_ERR_STATE, ME_ERR_CAPACITY = -1, -3, -4


@pytest.fixture(scope="module")
def eng():
    from cloud_map_evaluation_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _cuda(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
    torch.cuda.synchronize()  # (the raw ABI below reads it on the library's stream)
    return t


def _dp(a):
    return a.ctypes.data_as(C.c_void_p)


def _rc(eng, fn, *args):
    """a call of the raw ABI -> its return code"""
    return int(getattr(eng._L, fn)(eng._ctx, *args))


def _refused(eng, call, code):
    from cloud_map_evaluation_amd.engine import MapEvalError

    with pytest.raises(MapEvalError, match=rf"^\[{code}\]"):
        call()


# =============================================================================================================================================
# down-sample
# =============================================================================================================================================
DS = E.ds_small_cases()


@pytest.mark.parametrize("c", DS, ids=[c["name"] for c in DS])
def test_downsample_equals_the_model_bit_for_bit(eng, c):
    from cloud_map_evaluation_amd.engine import MapEvalError

    ref = R.downsample(c["xyz"], c["vs"], c["normals"])
    eng.upload(0, c["xyz"])
    if c["normals"] is not None:
        eng.set_normals(0, c["normals"])
    v = eng.voxel_downsample(0, c["vs"])
    assert v == len(ref["points"]) == eng.size(0), c["name"]
    assert _same(eng.download(0), ref["points"]), c["name"]
    if c["normals"] is not None:
        assert _same(eng.get_normals(0), ref["normals"]), c["name"]
    # out of place: the same positions, no normals, the source as it was
    eng.upload(0, c["xyz"])
    if c["normals"] is not None:
        eng.set_normals(0, c["normals"])
    assert eng.downsample_into(0, eng, 1, c["vs"]) == len(ref["points"])
    assert _same(eng.download(1), ref["points"]), c["name"]
    assert _same(eng.download(0), c["xyz"])
    with pytest.raises(MapEvalError, match="no normals"):
        eng.get_normals(1)


def _slot_state(eng, slot):
    idx, d2 = eng.nn_fetch(slot)
    return eng.size(slot), eng.download(slot), idx, d2


def _state_equal(a, b):
    return a[0] == b[0] and _same(a[1], b[1]) and np.array_equal(a[2], b[2]) and _same(a[3], b[3])


def _refusal_leaves_both_slots(eng, xyz, vs):
    other = E.ds_key_field_case()["xyz"] + 0.125
    eng.upload(0, xyz)
    eng.upload(1, other)
    eng.nn1(0, 1)
    eng.nn1(1, 0)
    before = _slot_state(eng, 0), _slot_state(eng, 1)
    _refused(eng, lambda: eng.voxel_downsample(0, vs), ME_ERR_ARG)
    assert _state_equal(_slot_state(eng, 0), before[0]) and _state_equal(_slot_state(eng, 1), before[1])
    _refused(eng, lambda: eng.downsample_into(0, eng, 1, vs), ME_ERR_ARG)
    assert _state_equal(_slot_state(eng, 0), before[0]) and _state_equal(_slot_state(eng, 1), before[1])


@pytest.mark.parametrize("axis", range(3))
def test_index_2097152_is_refused_and_the_slots_are_untouched(eng, axis):
    c = E.ds_refused_cases()[axis]  # (the same cloud one ulp lower, index 2097151, is accepted: the key_fields case above)
    _refusal_leaves_both_slots(eng, c["xyz"], c["vs"])


@pytest.mark.parametrize("vs", E.BAD_VOXEL_SIZES, ids=str)
def test_bad_voxel_size_is_refused_and_the_slots_are_untouched(eng, vs):
    _refusal_leaves_both_slots(eng, E.ds_key_field_case()["xyz"], vs)


_BBOX_REF = {}


def _bbox_ref(n, where):
    if (n, where) not in _BBOX_REF:
        c = E.ds_bbox_case(n, where)
        _BBOX_REF[(n, where)] = (c, R.downsample(c["xyz"], c["vs"])["points"])
    return _BBOX_REF[(n, where)]


@pytest.mark.parametrize("route", ["numpy", "cuda"])
@pytest.mark.parametrize("n", E.BBOX_SIZES)
def test_bounding_box_minimum_in_every_corner_of_the_grid(eng, n, route):
    """numpy upload: k_bbox; cuda upload: k_ingest.  A minimum the box misses moves the lattice origin and with it the voxels."""
    for where in E.bbox_variants(n):
        c, want = _bbox_ref(n, where)
        eng.upload(0, c["xyz"] if route == "numpy" else _cuda(c["xyz"]))
        assert eng.voxel_downsample(0, c["vs"]) == len(want), c["name"]
        assert _same(eng.download(0), want), c["name"]


def test_borrowed_input_is_read_in_place_and_left_alone():
    import torch

    from cloud_map_evaluation_amd.engine import Engine

    c = E.ds_face_case()
    want = R.downsample(c["xyz"], c["vs"])["points"]
    with Engine(0, borrow_device_input=True) as e:
        t = _cuda(c["xyz"])
        e.upload(0, t)
        assert e.voxel_downsample(0, c["vs"]) == len(want)
        assert _same(e.download(0), want)
        torch.cuda.synchronize()
        assert _same(t.cpu().numpy(), c["xyz"])  # the caller's tensor, byte for byte


# =============================================================================================================================================
# transform
# =============================================================================================================================================
TF = E.tf_cases()


@pytest.mark.parametrize("c", TF, ids=[c["name"] for c in TF])
def test_transform_three_routes_equal_the_model_bit_for_bit(eng, c):
    want = R.transform(c["xyz"], c["T"])
    eng.upload(0, c["xyz"], T=c["T"])  # k_transform after the copy
    a = eng.download(0)
    eng.upload(0, _cuda(c["xyz"]), T=c["T"])  # k_ingest
    b = eng.download(0)
    eng.upload(0, c["xyz"])
    eng.transform_cloud(0, c["T"])  # k_transform on the resident cloud
    d = eng.download(0)
    assert _same(a, want) and _same(b, want) and _same(d, want), c["name"]


@pytest.mark.parametrize("name", list(E.identities()))
def test_identity_keeps_the_bytes_and_the_nn_result(eng, name):
    T = E.identities()[name]
    xyz, other = E.tf_cloud(257), E.tf_cloud(4097)
    eng.upload(0, xyz)
    eng.upload(1, other)
    eng.nn1(0, 1)
    before = _slot_state(eng, 0)
    eng.transform_cloud(0, T)
    assert _state_equal(_slot_state(eng, 0), before)
    for src in (xyz, _cuda(xyz)):
        eng.upload(0, src, T=T)
        assert _same(eng.download(0), xyz)


@pytest.mark.parametrize("route", ["upload_T", "upload_T_cuda", "transform_cloud"])
def test_downsample_after_a_projective_transform_follows_the_moved_points(eng, route):
    c = [t for t in TF if t["name"] == "transform/proj_x/4097"][0]
    want = R.downsample(R.transform(c["xyz"], c["T"]), 0.5)["points"]
    if route == "transform_cloud":
        eng.upload(0, c["xyz"])
        eng.transform_cloud(0, c["T"])
    else:
        eng.upload(0, c["xyz"] if route == "upload_T" else _cuda(c["xyz"]), T=c["T"])
    assert eng.voxel_downsample(0, 0.5) == len(want)
    assert _same(eng.download(0), want)


def _reads_as_not_uploaded(eng, slot, n):
    buf, idx, d2 = np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros(max(n, 4097))
    m = C.c_int64(0)
    assert _rc(eng, "me_cloud_size", slot) == -1
    assert _rc(eng, "me_download_cloud", slot, _dp(buf)) == ME_ERR_STATE
    assert _rc(eng, "me_nn1", slot, 1 - slot, _dp(idx), _dp(d2)) == ME_ERR_STATE      # as the query
    assert _rc(eng, "me_nn1", 1 - slot, slot, None, None) == ME_ERR_STATE            # as the reference
    assert _rc(eng, "me_voxel_downsample", slot, 0.5, C.byref(m)) == ME_ERR_STATE
    assert (buf == 0).all() and (d2 == 0).all()


@pytest.mark.parametrize("all_nan", [False, True], ids=["nan_inf", "all_nan"])
def test_a_zero_divisor_is_refused_and_the_slot_stays_unusable_until_the_next_upload(eng, all_nan):
    c = E.tf_w_zero_case(all_nan)
    T = np.ascontiguousarray(c["T"], np.float64).reshape(16)
    n = len(c["xyz"])
    other = E.tf_cloud(4097)
    eng.upload(1, other)
    # on the resident cloud
    eng.upload(0, c["xyz"])
    assert _rc(eng, "me_transform_cloud", 0, _dp(T)) == ME_ERR_ARG
    _reads_as_not_uploaded(eng, 0, n)
    eng.upload(0, c["xyz"])  # a fresh upload into the slot works
    assert _same(eng.download(0), c["xyz"])
    eng.nn1(0, 1)
    # in the upload itself, from the host and from the device
    assert _rc(eng, "me_upload_cloud", 0, _dp(c["xyz"]), n, _dp(T), 0.0) == ME_ERR_ARG
    _reads_as_not_uploaded(eng, 0, n)
    t = _cuda(c["xyz"])
    assert _rc(eng, "me_upload_cloud_device", 0, C.c_void_p(t.data_ptr()), n, _dp(T), 0.0) == ME_ERR_ARG
    _reads_as_not_uploaded(eng, 0, n)
    eng.upload(0, c["xyz"])
    assert _same(eng.download(0), c["xyz"]) and _same(eng.download(1), other)


# =============================================================================================================================================
# render_distance
# =============================================================================================================================================
RD = E.rd_cases()


@pytest.mark.parametrize("c", RD, ids=[c["name"] for c in RD])
def test_render_distance_colours_and_gates_bit_for_bit(eng, c):
    n, d2, dis = len(c["d2"]), c["d2"], c["dis"]
    eng.upload(0, c["xyz"])
    eng.set_nn_result(0, 1, d2)
    want = R.render_distance(d2, dis)
    for gate, mode in E.GATES:
        rgb, inl = eng.renderDistanceOnPointCloud(0, dis, gate, mode)
        assert _same(rgb, want), (c["name"], gate, mode)
        assert np.array_equal(inl, R.inliers(d2, gate, mode)), (c["name"], gate, mode)
    raw = np.full((n, 3), -7.0)  # the raw ABI without an inlier array
    assert _rc(eng, "me_render_distance", 0, dis, E.GATE, 1, _dp(raw), None) == 0
    assert _same(raw, want)


def test_render_distance_refusals(eng):
    c = RD[-1]
    n = len(c["d2"])
    eng.upload(0, c["xyz"])
    rgb, inl = np.full((n, 3), -7.0), np.full(n, 9, np.uint8)
    assert _rc(eng, "me_render_distance", 0, c["dis"], -1.0, 0, _dp(rgb), _dp(inl)) == ME_ERR_STATE  # no NN result yet
    eng.set_nn_result(0, 1, c["d2"])
    for dis in (0.0, -1.0, float("nan")):
        assert _rc(eng, "me_render_distance", 0, dis, -1.0, 0, _dp(rgb), _dp(inl)) == ME_ERR_ARG
    assert (rgb == -7.0).all() and (inl == 9).all()


# =============================================================================================================================================
# render_entropy
# =============================================================================================================================================
RE = E.re_small_cases()


def _check_entropy(eng, c):
    ref = R.render_entropy(c["xyz"], c["ent"], c["valid"])
    eng.upload(0, c["xyz"])
    eng.set_mme_result(0, c["ent"], c["valid"])
    xyz, rgb, mn, mx = eng.ColorPointCloudByMME(0)
    assert len(xyz) == ref["n_valid"], c["name"]
    assert _same(xyz, ref["xyz"]), c["name"]
    assert _same([mn, mx], [ref["min_abs"], ref["max_abs"]]), (c["name"], mn, mx)
    assert rgb.shape == ref["rgb"].shape
    exact = R.jet_exact_mask(ref["ne"])
    assert np.array_equal(_bits(rgb[exact]), _bits(ref["rgb"][exact])), c["name"]
    np.testing.assert_allclose(rgb, ref["rgb"], rtol=0, atol=1e-9, err_msg=c["name"])
    return ref


@pytest.mark.parametrize("c", RE, ids=[c["name"] for c in RE])
def test_render_entropy_equals_the_model(eng, c):
    _check_entropy(eng, c)


def test_render_entropy_range_extremes_in_the_second_trip(eng):
    _check_entropy(eng, E.re_body_case(E.RE_TAIL_N, tail=True))


def test_render_entropy_raw_abi(eng):
    c = E.re_body_case(257)
    ref = R.render_entropy(c["xyz"], c["ent"], c["valid"])
    m = ref["n_valid"]
    eng.upload(0, c["xyz"])
    nv, mn, mx = C.c_int64(-5), C.c_double(-5.0), C.c_double(-5.0)
    tail = (C.byref(nv), C.byref(mn), C.byref(mx))
    xyz, rgb = np.full((m, 3), -7.0), np.full((m, 3), -7.0)
    assert _rc(eng, "me_render_entropy", 0, None, None, 0, *tail) == ME_ERR_STATE  # no MME result yet
    eng.set_mme_result(0, c["ent"], c["valid"])
    assert _rc(eng, "me_render_entropy", 0, None, None, 0, *tail) == 0  # the sizing call
    assert (nv.value, mn.value, mx.value) == (m, ref["min_abs"], ref["max_abs"])
    assert _rc(eng, "me_render_entropy", 0, _dp(xyz), None, m, *tail) == ME_ERR_ARG
    assert _rc(eng, "me_render_entropy", 0, None, _dp(rgb), m, *tail) == ME_ERR_ARG
    nv.value = -5
    assert _rc(eng, "me_render_entropy", 0, _dp(xyz), _dp(rgb), m - 1, *tail) == ME_ERR_CAPACITY
    assert nv.value == m and (xyz == -7.0).all() and (rgb == -7.0).all()
    assert _rc(eng, "me_render_entropy", 0, _dp(xyz), _dp(rgb), m, *tail) == 0
    assert _same(xyz, ref["xyz"])
    np.testing.assert_allclose(rgb, ref["rgb"], rtol=0, atol=1e-9)
