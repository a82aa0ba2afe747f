"""The lifetime of every resident result: which event keeps it, which drops it.

Three tables, plain Python (no GPU at import):

  PRODUCERS   one entry per resident result: make(e, slot) runs the feature with fixed parameters, fetch(e, slot) returns a dict of
              numpy arrays in cloud order, `keyed` says whether the result belongs to one slot, to the pair, or to the context, and
              `needs` names every fact the documents let the result depend on, each with the sentence that says so.
  DISTURBERS  one entry per event that re-sorts a slot ("resort"), replaces its points ("points") or replaces an input of a result
              ("inputs"): act(e, slot), the facts it changes on the slot it acts on (`changes`) and on the other one
              (`changes_other`), and the results it writes afresh (`writes`, `writes_other`).
  EXPECT      (producer, disturber, "own" | "other") -> (KEEP | DROP | ROTATED | NEW, citation).  "own": the disturber acts on the
              producer's slot, "other": on the other slot.

EXPECT is filled from include/mapeval_hip.h ("H:" + the entry point whose comment is quoted) and DESIGN.md ("D:" + section), never
from the code: a result is dropped exactly when a fact it `needs` is among the facts the event `changes`.  NEW is the one value the
three of the issue cannot express: the disturber is itself a producer of this result (a second me_mme over a first), or carries it
over in a documented, changed form (normals travel through a selection and are averaged by a down-sample; a voxel table is rebuilt on
demand), so a successful fetch legitimately returns other bytes.  A NEW cell is held to this: the fetch equals the same fetch on a
fresh engine that ran the disturber WITHOUT the producer's make - a result the event made, with nothing of the earlier one in it -
and, after a point replacement, differs from the earlier one (a table about points no longer in the slot is stale however
repeatable).  The one producer whose make alters its own input (orient_normals flips the normals the next call starts from) is
compared with the earlier bytes alone.  In every other cell a successful fetch that is not bytewise equal to the earlier one is a
failure, whatever the table says.

Facts: "points" (the slot's coordinates), "order" (its sorted order: any index rebuild), "normals", "nn" (the 1-NN result with the
slot as the query), "lg" (its local-geometry result), "planes" (its plane labels), "mesh" (the resident mesh), "recon" (the last
reconstruction; the last two belong to the context, not to a slot).
"""
from __future__ import annotations

import math

import numpy as np

KEEP, DROP, ROTATED, NEW = "KEEP", "DROP", "ROTATED", "NEW"

N0, N1 = 3001, 2500   # points of slot 0 / slot 1
CELL = 0.1            # cell size of the uploads; the producers use radii that fit it, the re-sort disturbers 0.3
R_FIT, R_FAR = 0.1, 0.3
VOX = 0.25


# ------------------------------------------------------------------------------------------------------------------------ inputs
def cloud(n: int, seed: int) -> np.ndarray:
    """n points in the unit cube: half of them uniform, half a dense slab (2 mm thick) through z = 0.5."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3))
    m = n // 2
    p[:m, 2] = 0.5 + 0.002 * rng.standard_normal(m)
    return np.ascontiguousarray(p[rng.permutation(n)])


def normals(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = np.array([0.0, 0.0, 1.0]) + 0.3 * rng.standard_normal((n, 3))
    return np.ascontiguousarray(v / np.linalg.norm(v, axis=1)[:, None])


def mesh(seed: int = 0):
    from cloud_map_evaluation_amd import synth

    v, t = synth.heightfield_mesh(12, 12, 1.0 / 11.0, 0.05, seed=seed)
    v = v.copy()
    v[:, 2] += 0.5
    return np.ascontiguousarray(v), t


_CACHE: dict = {}


def data(key, fn, *a):
    if key not in _CACHE:
        _CACHE[key] = fn(*a)
    return _CACHE[key]


def points(slot: int) -> np.ndarray:
    return data(("pts", slot), cloud, (N0, N1)[slot], 11 + slot)


def new_points(slot: int) -> np.ndarray:
    return data(("new", slot), cloud, (N0, N1)[slot], 21 + slot)


def nrm(slot: int, which: int = 0) -> np.ndarray:
    return data(("nrm", slot, which), normals, (N0, N1)[slot], 31 + slot + 10 * which)


def transform() -> np.ndarray:
    a = math.radians(35.0)
    T = np.eye(4)
    T[:3, :3] = [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = (0.25, -0.5, 0.125)
    return T


def base(e, cell: float = CELL):
    """What every cell starts from: both clouds at the cell size, normals on both, the mesh."""
    for s in (0, 1):
        e.upload(s, points(s), cell_size=cell)
        e.set_normals(s, nrm(s))
    e.mesh_upload(*data("mesh0", mesh, 0))


_SCRATCH = []  # a second engine that receives select_kept_into's output (the mask's only read-out); closed by close_scratch()


def scratch():
    from cloud_map_evaluation_amd.engine import Engine

    if not _SCRATCH:
        _SCRATCH.append(Engine(0))
    return _SCRATCH[0]


def close_scratch():
    while _SCRATCH:
        _SCRATCH.pop().close()


# --------------------------------------------------------------------------------------------------------------------- producers
def _mk_nn1(e, s):
    e.nn1(s, 1 - s, fetch=False)


def _ft_nn1(e, s):
    idx, d2 = e.nn_fetch(s)
    return {"idx": idx, "d2": d2}


def _mk_mme(e, s):
    e.mme(s, R_FIT, 5, per_point=False)


def _ft_mme(e, s):
    ent, val = e.mme_fetch(s)
    return {"entropy": ent, "valid": val}


def _mk_lg(e, s):
    e.local_geometry(s, R_FIT, 5)


def _ft_lg(e, s):
    eig, k, v = e.local_geometry_fetch(s)
    return {"eig": eig, "k": k, "valid": v}


def _mk_surface(e, s):
    e.nn1(s, 1 - s, fetch=False)
    e.nn_surface_error(s, plane_thresholds=(0.05,), angle_thresholds_deg=(20.0,))


def _ft_surface(e, s):
    d, c = e.nn_surface_fetch(s)
    return {"plane_d": d, "cos_n": c}


def _mk_m3c2(e, s):
    e.m3c2(s, 0.05, 0.08)  # R = sqrt(0.05^2 + 0.08^2) = 0.0943: the 0.1 cell lies in [R, 1.5 R], no rebuild


def _ft_m3c2(e, s):
    return e.m3c2_fetch(s)


def _mk_mesh(e, s):
    e.mesh_distance(s)


def _ft_mesh(e, s):
    return e.mesh_distance_fetch(s)


def _mk_normals(e, s):
    e.set_normals(s, nrm(s))


def _ft_normals(e, s):
    return {"normals": e.get_normals(s)}


def _mk_cov(e, s):
    e.gicp_covariances(s, 1e-3)


def _ft_cov(e, s):
    return {"cov": e.get_covariances(s)}


def _mk_fpfh(e, s):
    for t in (s, 1 - s):
        e.fpfh(t, 0.15, 20, 10, fetch=False)


def _ft_fpfh(e, s):
    # (the features have no fetch of their own: their 1-NN in feature space is a function of every feature of both slots)
    corr, n = e.fpfh_match(s, 1 - s, mutual=False)
    return {"corr": corr}


def _mk_outlier(e, s):
    e.radius_outlier(s, 5, R_FIT)


def _ft_outlier(e, s):
    d = scratch()
    e.select_kept_into(s, d, 0)
    return {"kept": d.download(0)}


def _mk_cluster(e, s):
    e.cluster_dbscan(s, R_FIT, 5)


def _ft_cluster(e, s):
    sizes = e.cluster_sizes(s)
    keep = e.cluster_keep(s, 2, 0, fetch=True)[1]
    return {"sizes": sizes, "keep": keep}


_PLANE_KW = dict(distance_threshold=0.01, num_iterations=200, max_planes=2, min_inliers=50, seed=1)


def _mk_planes(e, s):
    e.segment_planes(s, **_PLANE_KW)


def _ft_planes(e, s):
    planes, labels = e.plane_fetch(s)
    return {"labels": labels, "plane": np.array([p["plane"] for p in planes], np.float64).reshape(-1, 4),
            "count": np.array([p["count"] for p in planes], np.int64)}


def _mk_mom(e, s):
    e.local_geometry(s, R_FIT, 5)
    e.segment_planes(s, **_PLANE_KW)
    e.mom(s, min_axis_points=100)


def _ft_mom(e, s):
    return {"axis": e.mom_fetch(s)}


def _mk_orient(e, s):
    e.orient_normals(s, k=8)


def _ft_orient(e, s):
    return e.orient_fetch(s)


def _mk_voxel(e, s):
    e.voxel_build(s, VOX)


def _ft_voxel(e, s):
    keys, n, mu, sg, en = e.voxel_gaussians(s, VOX)
    return {"keys": keys, "n": n, "mu": mu, "sigma": sg, "entropy": en}


def _mk_recon(e, s):
    e.reconstruct(s, 0.05, radius=R_FIT, min_k=4, fetch=False)  # R = 0.1: the 0.1 cell fits, no rebuild


def _ft_recon(e, s):
    return e.reconstruct_nodes()


_POINTS = "the cloud changed (upload, down-sample, transform, perturbation, selection)"
_CLOUD_ORDER = "held in cloud order: an index rebuild of the same points does not touch it"

# name -> dict(make, fetch, keyed, order, engine = the Engine methods used, needs = {(side, fact): citation}, keep = citation of KEEP)
PRODUCERS = {
    "nn1": dict(make=_mk_nn1, fetch=_ft_nn1, keyed="pair", order="sorted", engine=("nn1", "nn_fetch"),
                needs={("own", "points"): "H:me_perturb_cloud 'NN ... state invalidated ... the other slot's NN result invalidated' (the upload-time reset)",
                       ("other", "points"): "H:me_perturb_cloud 'the other slot's NN result invalidated' (the upload-time reset)",
                       ("own", "order"): "H:me_radius_normals 'may rebuild the slot's index ..., which discards the 1-NN result of the slot'",
                       ("other", "order"): "H:me_radius_normals '... and of its twin, the other slot (it searched in this one)'; H:me_m3c2 'DISCARDS the resident 1-NN results of both slots'",
                       ("own", "nn"): "H:me_nn_fetch 'the last nn1(query_slot, ..)': a new search or me_set_nn_result replaces it"},
                keep="H:me_orient_normals STATE / H:me_knn_search STATE: 1-NN results stay when neither slot's points nor index change"),
    "mme": dict(make=_mk_mme, fetch=_ft_mme, keyed="slot", order="sorted", engine=("mme", "mme_fetch"),
                needs={("own", "points"): "H:me_perturb_cloud 'NN, MME, voxel state invalidated'; H:me_set_mme_result 'me_transform_cloud discards the slot's MME result'",
                       ("own", "order"): "H:me_knn_search STATE 'what that rebuild discards (... that slot's MME, local-geometry and M3C2 results)'"},
                keep="H:me_knn_search STATE 'that slot's MME': only the slot's own rebuild discards it"),
    "local_geometry": dict(make=_mk_lg, fetch=_ft_lg, keyed="slot", order="sorted", engine=("local_geometry", "local_geometry_fetch"),
                           needs={("own", "points"): "H:me_local_geometry_fetch 'no current result - " + _POINTS + "'",
                                  ("own", "order"): "H:me_local_geometry_fetch '... or another stage rebuilt the slot's grid at a different cell'"},
                           keep="H:me_m3c2 'the re-indexed slot's local-geometry result': only the slot's own rebuild discards it"),
    "surface": dict(make=_mk_surface, fetch=_ft_surface, keyed="pair", order="sorted", engine=("nn_surface_error", "nn_surface_fetch"),
                    needs={(sd, f): "H:me_nn_surface_fetch 'it is discarded with the 1-NN result'; H:me_m3c2 'me_nn_surface_error's result included'"
                           for sd, f in (("own", "points"), ("other", "points"), ("own", "order"), ("other", "order"), ("own", "nn"))},
                    keep="H:me_nn_surface_fetch: discarded with the 1-NN result and with nothing else (new normals: H:me_orient_normals STATE 'everything else ... stays')"),
    "m3c2": dict(make=_mk_m3c2, fetch=_ft_m3c2, keyed="pair", order="sorted", engine=("m3c2", "m3c2_fetch"),
                 needs={("own", "points"): "H:me_m3c2_fetch 'discarded when either slot's points change'",
                        ("other", "points"): "H:me_m3c2_fetch 'discarded when either slot's points change'",
                        ("own", "order"): "H:me_m3c2_fetch '... or the query slot is re-indexed'"},
                 keep="H:me_m3c2_fetch names the query slot's re-index only (H:me_reconstruct corrected to agree); H:me_orient_normals STATE lists M3C2 among what stays"),
    "mesh_distance": dict(make=_mk_mesh, fetch=_ft_mesh, keyed="slot", order="sorted", engine=("mesh_distance", "mesh_distance_fetch"),
                          needs={("own", "points"): "H:me_mesh_distance_fetch 'discarded when the slot's points change'",
                                 ("own", "order"): "H:me_mesh_distance_fetch '... or the slot is re-indexed'",
                                 ("ctx", "mesh"): "H:me_mesh_upload 'a second upload replaces it, me_mesh_clear drops it; both discard the mesh-distance results of both slots'"},
                          keep="H:me_mesh_distance_fetch 'It survives me_nn1 and me_mme'"),
    "normals": dict(make=_mk_normals, fetch=_ft_normals, keyed="slot", order="cloud", engine=("set_normals", "get_normals"),
                    needs={("own", "points"): "H:me_perturb_cloud 'normals and covariances dropped' (the upload-time reset)"},
                    keep="H:me_m3c2 'Normals are kept in cloud order and survive'; H:me_reconstruct 'points and normals stay'"),
    "covariances": dict(make=_mk_cov, fetch=_ft_cov, keyed="slot", order="cloud", engine=("gicp_covariances", "get_covariances"),
                        needs={("own", "points"): "H:me_perturb_cloud 'normals and covariances dropped'; H:me_outlier_select_into 'covariances ... of dst are dropped'",
                               ("own", "normals"): "H:me_radius_normals 'covariances on the slot are dropped, as me_set_normals drops them'; H:me_orient_normals STATE"},
                        keep="H:me_knn_search STATE lists covariances among what stays; " + _CLOUD_ORDER),
    "fpfh": dict(make=_mk_fpfh, fetch=_ft_fpfh, keyed="pair", order="cloud", engine=("fpfh", "fpfh_match"),
                 needs={(sd, f): "H:me_fpfh 'an upload, down-sample, perturbation, transform or new normals drops them'; H:me_outlier_select_into; H:me_orient_normals STATE"
                        for sd in ("own", "other") for f in ("points", "normals")},
                 keep="H:me_fpfh 'The features stay on the device with the slot'; " + _CLOUD_ORDER),
    "outlier_mask": dict(make=_mk_outlier, fetch=_ft_outlier, keyed="slot", order="cloud", engine=("radius_outlier", "select_kept_into", "download"),
                         needs={("own", "points"): "H:outlier removal 'a uint8 keep-mask on the slot, held until the " + _POINTS + "'"},
                         keep="H:outlier removal 'held until the cloud changes'; " + _CLOUD_ORDER),
    "cluster": dict(make=_mk_cluster, fetch=_ft_cluster, keyed="slot", order="cloud", engine=("cluster_dbscan", "cluster_sizes", "cluster_keep"),
                    needs={("own", "points"): "H:clustering 'Labels and sizes stay with the slot until the " + _POINTS + "'"},
                    keep="H:clustering 'stay with the slot until the cloud changes'; " + _CLOUD_ORDER),
    "planes": dict(make=_mk_planes, fetch=_ft_planes, keyed="slot", order="cloud", engine=("segment_planes", "plane_fetch"),
                   needs={("own", "points"): "H:me_segment_planes 'Labels and records stay on the slot until the " + _POINTS + "'"},
                   keep="H:me_segment_planes 'stay on the slot until the cloud changes'; H:me_mom 'me_local_geometry discards only what depends on the sorted order'"),
    "mom": dict(make=_mk_mom, fetch=_ft_mom, keyed="slot", order="cloud", engine=("local_geometry", "segment_planes", "mom", "mom_fetch"),
                needs={("own", "points"): "H:me_mom_fetch 'dropped with the labels and with the eigenvalues (a changed cloud ...)'",
                       ("own", "order"): "H:me_mom_fetch 'dropped ... with the eigenvalues' + H:me_local_geometry_fetch 'another stage rebuilt the slot's grid'; H:me_m3c2 '(me_local_geometry_fetch, me_mom)'",
                       ("own", "lg"): "H:me_mom_fetch 'a later me_segment_planes or me_local_geometry'",
                       ("own", "planes"): "H:me_mom_fetch 'a later me_segment_planes or me_local_geometry'"},
                keep="H:me_mom_fetch: dropped with the slot's labels and eigenvalues and with nothing else"),
    "orient": dict(make=_mk_orient, fetch=_ft_orient, keyed="slot", order="cloud", engine=("orient_normals", "orient_fetch"),
                   make_alters_inputs=True,  # (make flips the slot's normals: a second orientation starts from other normals than a first)
                   needs={("own", "points"): "H:me_orient_normals STATE 'until the slot's normals or points are next replaced (an upload, a device-side producer, a transform ...)'",
                          ("own", "normals"): "H:me_orient_normals STATE '... any of the normal estimators, the set-normals call'"},
                   keep="H:me_orient_normals STATE 'stay fetchable until the slot's normals or points are next replaced'; " + _CLOUD_ORDER),
    "voxel": dict(make=_mk_voxel, fetch=_ft_voxel, keyed="slot", order="key", engine=("voxel_build", "voxel_gaussians"), rebuilt_on_demand=True,
                  needs={},
                  keep="H:me_knn_search STATE lists voxel tables among what stays; the table is in ascending key order, a function of the points alone"),
    "reconstruct": dict(make=_mk_recon, fetch=_ft_recon, keyed="context", order="lattice", engine=("reconstruct", "reconstruct_nodes"),
                        needs={("ctx", "mesh_clear"): "H:surface reconstruction 'held on the primary context ... until the next call of either producer or until the mesh clear call'"},
                        keep="H:surface reconstruction 'held ... until the next call of either producer or until the mesh clear call': cloud events do not touch it"),
}


# -------------------------------------------------------------------------------------------------------------------- disturbers
def _d_mme(e, s):
    e.mme(s, R_FAR, 5, per_point=False)


def _d_lg(e, s):
    e.local_geometry(s, R_FAR, 5)


def _d_rn_far(e, s):
    e.radius_normals(s, R_FAR, 5)


def _d_ro(e, s):
    e.radius_outlier(s, 5, R_FAR)


def _d_dbscan(e, s):
    e.cluster_dbscan(s, R_FAR, 5)


def _d_m3c2(e, s):
    e.m3c2(s, 0.2, 0.2, core_mask=(np.arange(e.size(s)) % 16 == 0))  # R = 0.283; a sixteenth of the core points keeps it quick


def _d_recon(e, s):
    e.reconstruct(s, 0.1, radius=R_FAR, min_k=4, band=0, fetch=False)


def _d_suite(e, s):
    from cloud_map_evaluation_amd.engine import Param

    e.run_suite(Param(icp_max_distance_=1.0, nn_radius_=R_FAR, vmd_voxel_size_=VOX))


def _d_upload(e, s):
    e.upload(s, new_points(s), cell_size=CELL)


def _d_transform(e, s):
    e.transform_cloud(s, transform())


def _d_vds(e, s):
    e.voxel_downsample(s, 0.05)


def _d_perturb(e, s):
    e.perturb(s, s, noise_std=0.01, seed=3)


def _d_select(e, s):
    e.radius_outlier(s, 5, R_FIT)  # (the radius fits the cell: the mask is written without a rebuild)
    e.select_kept_into(s)


def _d_ds_into(e, s):
    e.downsample_into(1 - s, e, s, 0.05)


def _d_sample(e, s):
    e.mesh_sample(s, 2000, seed=5)


def _d_set_normals(e, s):
    e.set_normals(s, nrm(s, 1))


def _d_est_normals(e, s):
    e.estimate_normals(s, 10, fetch=False)


def _d_rn_fit(e, s):
    e.radius_normals(s, R_FIT, 5)


def _d_orient(e, s):
    e.orient_normals(s, k=6, direction=(0.0, 0.0, -1.0))


def _d_mesh_upload(e, s):
    e.mesh_upload(*data("mesh1", mesh, 1))


def _d_mesh_clear(e, s):
    e.mesh_clear()


def _d_nn1(e, s):
    e.nn1(s, 1 - s, fetch=False)


def _d_set_nn(e, s):
    e.set_nn_result(s, 1 - s, np.full(e.size(s), 0.25))


_RESORT = "the radius does not fit the 0.1 cell (cell < r or cell > 1.5 r): the slot is rebuilt at the radius - "
_REPLACED = ("points", "order", "normals", "nn", "lg", "planes")  # an upload-time reset: everything about the slot goes
# name -> dict(act, group, engine, changes / changes_other = facts changed on the acted / the other slot, ctx = context facts,
#              writes / writes_other = results written afresh for the acted / the other slot, cite)
DISTURBERS = {
    # ---- the same points, re-sorted
    "mme": dict(act=_d_mme, group="resort", engine=("mme",), changes=("order",), writes=("mme",),
                cite=_RESORT + "H:me_upload_cloud 'rebuilt lazily by me_mme'"),
    "local_geometry": dict(act=_d_lg, group="resort", engine=("local_geometry",), changes=("order", "lg"), writes=("local_geometry",),
                           cite=_RESORT + "H:local geometry 'The slot's radius grid is rebuilt at `radius` when its cell differs'"),
    "radius_normals": dict(act=_d_rn_far, group="resort", engine=("radius_normals",), changes=("order", "lg", "normals"),
                           writes=("local_geometry", "normals"),
                           cite=_RESORT + "H:me_radius_normals ORDER OF USE; 'The call ALSO stores the slot's local-geometry result'; the normals are replaced"),
    "radius_outlier": dict(act=_d_ro, group="resort", engine=("radius_outlier",), changes=("order",), writes=("outlier_mask",),
                           cite=_RESORT + "H:me_radius_outlier 'The slot's radius grid is rebuilt at the radius when its cell differs'"),
    "cluster_dbscan": dict(act=_d_dbscan, group="resort", engine=("cluster_dbscan",), changes=("order",), writes=("cluster",),
                           cite=_RESORT + "H:clustering 'The slot's radius grid is rebuilt at eps when its cell differs'"),
    "m3c2": dict(act=_d_m3c2, group="resort", engine=("m3c2",), changes=("order",), changes_other=("order",), writes=("m3c2",), both=True,
                 cite=_RESORT + "H:me_m3c2 INDEX AND ORDER OF USE 'Both slots need an index whose cell edge is >= R ... re-indexed at R'"),
    "reconstruct": dict(act=_d_recon, group="resort", engine=("reconstruct",), changes=("order",), ctx=("recon",), writes=("reconstruct",),
                        cite=_RESORT + "H:me_reconstruct 'a rebuild re-sorts the slot'"),
    "run_suite": dict(act=_d_suite, group="resort", engine=("run_suite",), changes=("order", "nn"), changes_other=("order", "nn"),
                      writes=("mme", "nn1"), writes_other=("mme", "nn1"), both=True,
                      cite=_RESORT + "H:me_run_suite 'An index that is missing or does not fit nn_radius is rebuilt'; it runs both MMEs and both searches"),
    # ---- new points
    "upload": dict(act=_d_upload, group="points", engine=("upload",), changes=_REPLACED, cite="H:me_upload_cloud: the slot holds another cloud"),
    "transform_cloud": dict(act=_d_transform, group="points", engine=("transform_cloud",), changes=("points", "order", "nn", "lg", "planes"),
                            rotates=("normals", "covariances"),
                            cite="H:me_transform_cloud 'the index is rebuilt'; H:me_radius_normals 'they follow me_transform_cloud (n <- R n)'; D:4.5 rotate_attributes"),
    "voxel_downsample": dict(act=_d_vds, group="points", engine=("voxel_downsample",), changes=_REPLACED, writes=("normals",),
                             cite="H:me_voxel_downsample 'in place ... The index is rebuilt'; H:me_fpfh 'normals ... averaged by a down-sample'"),
    "perturb": dict(act=_d_perturb, group="points", engine=("perturb",), changes=_REPLACED,
                    cite="H:me_perturb_cloud 'dst gets the upload-time reset ... (in place works)'"),
    "select_kept_into": dict(act=_d_select, group="points", engine=("radius_outlier", "select_kept_into"), changes=_REPLACED, writes=("normals",),
                             cite="H:me_outlier_select_into 'in place ... Normals travel with their points; covariances, FPFH features, NN and MME results of dst are dropped'"),
    "downsample_into": dict(act=_d_ds_into, group="points", engine=("downsample_into",), changes=_REPLACED,
                            cite="H:me_voxel_downsample_into 'dst gets the upload-time reset (no normals, features, NN, MME or voxel state)'; 'src is untouched'"),
    "mesh_sample": dict(act=_d_sample, group="points", engine=("mesh_sample",), changes=_REPLACED,
                        cite="H:me_mesh_sample 'become the cloud of dst_slot, as an upload would leave it'"),
    # ---- new inputs
    "set_normals": dict(act=_d_set_normals, group="inputs", engine=("set_normals",), changes=("normals",), writes=("normals",),
                        cite="H:me_radius_normals 'as me_set_normals drops them'; H:me_orient_normals STATE 'the set-normals call'"),
    "estimate_normals": dict(act=_d_est_normals, group="inputs", engine=("estimate_normals",), changes=("normals",), writes=("normals",),
                             cite="H:me_orient_normals STATE 'any of the normal estimators'; H:me_knn_search STATE: the k-NN walk re-indexes no slot"),
    "radius_normals_fit": dict(act=_d_rn_fit, group="inputs", engine=("radius_normals",), changes=("normals", "lg"), writes=("normals", "local_geometry"),
                               cite="H:me_radius_normals at a radius that fits the cell: new normals and a new local-geometry result, no rebuild"),
    "orient_normals": dict(act=_d_orient, group="inputs", engine=("orient_normals",), changes=("normals",), writes=("normals", "orient"),
                           cite="H:me_orient_normals STATE 'The normals are replaced in place ... covariances and FPFH features on the slot are dropped. Everything else ... stays'"),
    "mesh_upload": dict(act=_d_mesh_upload, group="inputs", engine=("mesh_upload",), ctx=("mesh",),
                        cite="H:me_mesh_upload 'a second upload replaces it ... discard the mesh-distance results of both slots'"),
    "mesh_clear": dict(act=_d_mesh_clear, group="inputs", engine=("mesh_clear",), ctx=("mesh", "mesh_clear"),
                       cite="H:me_mesh_upload 'me_mesh_clear drops it'; H:surface reconstruction 'until the mesh clear call'"),
    "nn1": dict(act=_d_nn1, group="inputs", engine=("nn1",), changes=("nn",), writes=("nn1",),
                cite="H:me_nn_surface_error 'The call leaves the 1-NN result untouched' - a new search does not: me_nn_surface_fetch 'discarded with the 1-NN result'"),
    "set_nn_result": dict(act=_d_set_nn, group="inputs", engine=("set_nn_result",), changes=("nn",), writes=("nn1",),
                          cite="H:me_nn_error_distribution 'the current 1-NN result (me_nn1, me_set_nn_result or the suite)'"),
}

SIDES = ("own", "other")


def _expect(pname: str, dname: str, side: str):
    P, D = PRODUCERS[pname], DISTURBERS[dname]
    own = D.get("changes", ()) if side == "own" else D.get("changes_other", ())
    other = D.get("changes_other", ()) if side == "own" else D.get("changes", ())
    written = D.get("writes", ()) if side == "own" else D.get("writes_other", ())
    if P["keyed"] == "context":  # one result per context, whichever slot the event names
        written = tuple(D.get("writes", ())) + tuple(D.get("writes_other", ()))
    if pname in written:
        return NEW, D["cite"] + " - the disturber writes this result itself"
    if side == "own" and pname in D.get("rotates", ()):
        return ROTATED, D["cite"]
    hits = [c for (sd, f), c in P["needs"].items()
            if (sd == "own" and f in own) or (sd == "other" and f in other) or (sd == "ctx" and f in D.get("ctx", ()))]
    if hits:
        return DROP, hits[0] + " <- " + D["cite"]
    if P.get("rebuilt_on_demand") and "points" in own:
        return NEW, "H:me_voxel_gaussians builds the table of the slot's current points when it holds none: " + D["cite"]
    return KEEP, P["keep"]


EXPECT = {(p, d, s): _expect(p, d, s) for p in PRODUCERS for d in DISTURBERS for s in SIDES}

# What the documents promise to KEEP at the least (the floor test_lifetime_table_cpu.py holds the table to): the cloud-order results
# under every re-sort of their own slot, and every slot-keyed result under any re-sort of the OTHER slot.  Two groups are outside it,
# each by a sentence of the header: the pair-keyed 1-NN results (a rebuild of either slot discards them: H:me_radius_normals ORDER OF
# USE) and me_mom's axis bytes, which are in cloud order but derived from the sorted-order eigenvalues (H:me_mom_fetch).
RESORT = tuple(d for d, D in DISTURBERS.items() if D["group"] == "resort")
CLOUD_ORDER = tuple(p for p, P in PRODUCERS.items() if P["order"] == "cloud" and p != "mom")
_ON_NORMALS = ("normals", "covariances", "fpfh", "orient")  # (a re-sort that also replaces the normals is outside the floor for these)
KEEP_FLOOR = {(p, d, "own") for p in CLOUD_ORDER for d in RESORT if p not in DISTURBERS[d].get("writes", ())
              and not (p in _ON_NORMALS and "normals" in DISTURBERS[d].get("changes", ()))}
KEEP_FLOOR |= {(p, d, "other") for p, P in PRODUCERS.items() if P["keyed"] == "slot" for d in RESORT if not DISTURBERS[d].get("both")}
KEEP_FLOOR |= {("fpfh", d, sd) for d in RESORT for sd in SIDES if "normals" not in DISTURBERS[d].get("changes", ())}


# ----------------------------------------------------------------------------------------- the two frames really differ (CPU)
def cell_ids(p: np.ndarray, cell_size: float) -> np.ndarray:
    """cloud_build_index's frame: cell_h = cell_size (1 + 2^-20), origin = floor(bbox_lo / cell_h) cell_h, cell =
    floor((p - origin) / cell_h); returned as one integer per point (x major)."""
    cell_h = cell_size * (1.0 + 2.0 ** -20)
    origin = np.floor(p.min(axis=0) / cell_h) * cell_h
    c = np.floor((p - origin) / cell_h).astype(np.int64)
    return (c[:, 0] * (1 << 21) + c[:, 1]) * (1 << 21) + c[:, 2]


def order_isomorphic(a: np.ndarray, b: np.ndarray) -> bool:
    """True iff the two per-point id sequences are order-isomorphic: a[i] < a[j] <=> b[i] < b[j] for all i, j (equal dense ranks).
    This is a statement about the radius-cell ids in x-major order and nothing more: the library sorts on Hilbert keys of finer
    codes, which this module does not model.  It is a plausibility check on the inputs - the two cell sizes put the points into
    differently ordered cells, so there is no reason for the two permutations to coincide - not a proof that they differ."""
    return np.array_equal(np.unique(a, return_inverse=True)[1], np.unique(b, return_inverse=True)[1])


def render() -> str:
    """The whole EXPECT table as text (DESIGN.md 4.21 carries it; test_lifetime_table_cpu.py keeps the two equal): one row per
    producer, one column per disturber, two letters per cell = own, other; K keep, D drop, R rotated, N new."""
    ds = list(DISTURBERS)
    rows = ["columns: " + " ".join(f"{i + 1}={d}" for i, d in enumerate(ds))]
    rows.append(" " * 15 + " ".join(f"{i + 1:<2d}" for i in range(len(ds))))
    for p in PRODUCERS:
        rows.append(p.ljust(15) + " ".join(EXPECT[(p, d, "own")][0][0] + EXPECT[(p, d, "other")][0][0] for d in ds))
    return "\n".join(rows)
