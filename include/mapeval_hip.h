/*
 * mapeval_hip.h — C ABI of libmapeval_hip.so: MapEval's metric hot path on AMD MI355X (gfx950).
 *
 * The reference (JokerJohn/Cloud_Map_Evaluation) has no plugin / FFI layer: its seam is the set of MapEval member
 * calls made by MapEval::process() (map_eval/src/map_eval.cpp:52-85).  Each entry point below replaces one of
 * those calls (or the Open3D / VoxelCalculator operator it loops over) with ONE batched device call; the
 * reference file:line it stands in for is cited per function.  Plain pointers and sizes only — no C++ or torch
 * types cross this boundary.  INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *   - clouds are AoS fp64 `double[N][3]`, exactly open3d::geometry::PointCloud::points_.data() (map_eval.h:45);
 *     host pointers unless the function name ends in _device.
 *   - the caller owns every host buffer; the library owns all device memory inside me_ctx.
 *   - every call is synchronous on return and returns ME_OK (0) or a negative ME_ERR_*; me_last_error() has text.
 *   - nullable outputs may be NULL (skips the D2H copy).
 *   - one me_ctx = one GPU = one host thread at a time (MapEval::process is single-threaded, map_eval.cpp:4).
 *   - results follow the reference's arithmetic, quirks included (squared-vs-unsquared gate :1219, triple
 *     division of sigma voxel_calculator.cpp:48/102/120, Cholesky-trace "W2" :136-138, k>=10 / k>=5 MME gates).
 *     Inlier / valid / voxel point counts are bit-exact; floating-point sums agree to ~1e-12 relative
 *     (summation order differs, as it already does between two runs of the TBB/OpenMP reference).
 */
#ifndef MAPEVAL_HIP_H
#define MAPEVAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ME_OK 0
#define ME_ERR_ARG (-1)      /* bad argument (null pointer, bad slot, n out of range, ...)          */
#define ME_ERR_HIP (-2)      /* a HIP runtime call failed (no device, OOM, ...)                     */
#define ME_ERR_STATE (-3)    /* call order violated (cloud not uploaded, search not run, ...)       */
#define ME_ERR_CAPACITY (-4) /* caller-provided output capacity too small (count still returned)    */

#define ME_SLOT_EST 0 /* map_3d_  (map_eval.h:322) */
#define ME_SLOT_GT 1  /* gt_3d_   (map_eval.h:322) */

#define ME_GATE_LE_UNSQUARED 0 /* keep iff d2 <= gate        — calculateMetricsWithInitialMatrix, map_eval.cpp:1219 (sic) */
#define ME_GATE_LT_SQUARED 1   /* keep iff d2 <  gate*gate   — Open3D EvaluateRegistration / ICP, map_eval.cpp:1168        */

typedef struct me_ctx me_ctx;

/* Raw (shard-local, all-reduce-able) sums of one direction of the AC/COM/CD pass.
 * Every field is a plain sum over the query points this context owns, so partials from several GPUs add. */
typedef struct me_nn_partial {
    int64_t n_query;     /* queries processed (shard size)                                  */
    int64_t n_corr;      /* correspondences that passed the gate  (points_set.size(), :1076) */
    int64_t n_inl[5];    /* number_vec   (map_eval.cpp:1102,1107,...)                        */
    double sum_d[5];     /* mean_vec before /C  (:1100)                                      */
    double sum_d2[5];    /* rmse_vec before /C  (:1101)                                      */
    double sum_sqrt_all; /* sum of sqrt(d2) over ALL queries, ungated (computeChamferDistance :1416) */
} me_nn_partial;

/* Finished result block of getDiffRegResultWithCorrespondence (map_eval.cpp:1140-1144):
 * the five Vector5d pushed into est_gt_results / gt_est_results, plus the CD term. */
typedef struct me_nn_stats_out {
    int64_t n_src;       /* source.points_.size() (whole cloud)                              */
    int64_t n_corr;      /* C                                                                */
    double mean[5];      /* result[0] */
    double rmse[5];      /* result[1]  -> "RMSE/AC:"  (map_eval.cpp:439)                     */
    double fitness[5];   /* result[2]  -> "Comp:"     (map_eval.cpp:445)                     */
    double sigma[5];     /* result[3] */
    double number[5];    /* result[4] */
    double mean_nn_dist; /* sum_sqrt_all / n_src : one half of computeChamferDistance (:1429) */
} me_nn_stats_out;

/* ---- lifetime ---------------------------------------------------------------------------------------------- */
/* device: HIP device ordinal (one context per GPU).  flags: 0, or an OR of the ME_FLAG_* below.  NULL on failure.
 * The library reads nothing from the environment: every behaviour switch is a flag here or a compile-time constant. */
me_ctx *me_create(int device, int flags);
/* ME_FLAG_BORROW_DEVICE_INPUT: me_upload_cloud_device / me_upload_slab_device without a transform (T NULL or the identity) read the
 * caller's device buffer WHERE IT LIES instead of copying it: the caller keeps it valid and unchanged until the slot's next upload
 * (or me_destroy).  Saves one 48-byte-per-point pass per cloud; calls that modify the cloud in place (me_transform_cloud,
 * me_voxel_downsample) switch to a private copy first.  No reference counterpart (Open3D owns its points_). */
#define ME_FLAG_BORROW_DEVICE_INPUT 1
/* ME_FLAG_MORTON_ORDER: sort the points along the Z (Morton) curve instead of the Hilbert curve.  An implementation detail of the index
 * — counts identical, fp results equal to rounding (tests/test_gpu_order.py) — kept as a test / measurement switch. */
#define ME_FLAG_MORTON_ORDER 2
void me_destroy(me_ctx *ctx);
const char *me_last_error(me_ctx *ctx); /* ctx may be NULL: returns the last me_create error */
int me_version(void);

/* A second LANE on the same clouds: a context that shares both cloud slots with `ctx` (uploads, indexes, NN / MME / voxel
 * results are common) but owns its stream, scratch memory and timers.  Two host threads may then drive the two
 * contexts concurrently, e.g. indexing the ground truth (HBM-bound) under the MME pass of the map (VALU-bound).
 * Rules: never let both lanes upload / re-index / transform the same slot, or write the same product of a slot (its
 * NN result, MME, voxel table), at the same time; reading a slot's index while the other lane builds the OTHER slot is
 * fine.  The twin is owned by `ctx` (me_destroy(ctx) frees it; me_destroy(twin) is a no-op).  No reference counterpart. */
me_ctx *me_twin(me_ctx *ctx);

/* Multi-GPU slab sharding (no reference counterpart; the reference is single-process).  After this call every
 * per-point pass (NN, MME) only processes the `rank`-th of `world` equal slabs of the sorted (space-filling-curve) query order,
 * and the voxel passes only own voxels whose key index falls in the rank's slab; partial sums are returned for
 * the caller to all-reduce (RCCL).  Default (0,1) = whole job. */
int me_set_shard(me_ctx *ctx, int rank, int world);

/* Multi-GPU SPATIAL slab (no reference counterpart).  After this call me_upload_cloud* keeps only the points with
 * lo - halo <= p[axis] < hi + halo (after the transform); points with lo <= p[axis] < hi are OWNED by this context —
 * they are the queries of every per-point pass and the only contributors to the voxel partials — the rest are halo,
 * visible as reference points / neighbours only.  Every rank therefore sorts and indexes ~1/world of each cloud.
 * MME is exact when halo >= nn_radius.  1-NN is exact for every query whose best distance is below its distance to
 * the slab's outer faces; the others are returned by me_nn_unresolved for the cross-rank step (me_nn_points on every
 * rank, min-reduce, me_nn_patch).
 * Per-point outputs in slab mode (round 3; what the distributed host needs for map_entropy.pcd / raw_rendered_dis_map.pcd,
 * map_eval.cpp:485-495, 686-736): the entropies / valid arrays of me_mme and the idx / d2 arrays of me_nn1 / me_nn_fetch have
 * one entry per point this context HOLDS of the slot (me_cloud_size: owned + halo), in the order me_slab_points reports;
 * halo points read entropy 0 / valid 0 / d2 -1 / idx -1; idx is an index into the points held of the reference slot and is
 * the global neighbour only where the query did not go through the cross-rank step (d2 is global after me_nn_patch).
 * axis < 0 switches slab mode off.  Must be called before the uploads it applies to. */
int me_set_slab(me_ctx *ctx, int axis, double lo, double hi, double halo);

/* Slab mode, 1-NN cross-rank step.  me_nn_unresolved: the owned queries of the last me_nn1(query_slot, ..) whose
 * result is not yet provably global; xyz_device (capacity x 3, device memory) receives their coordinates, *count
 * their number (ME_ERR_CAPACITY if it exceeds capacity; xyz_device may be NULL to query the count); d2_device
 * (optional, capacity doubles) receives their current best squared distances, the bound the other ranks have to beat. */
int me_nn_unresolved(me_ctx *ctx, int query_slot, double *xyz_device, double *d2_device, int64_t capacity, int64_t *count);
/* Exact squared distance from each of m arbitrary points (device, m x 3) to the nearest point this context holds of
 * ref_slot (owned + halo) -> d2_device[m]. */
int me_nn_points(me_ctx *ctx, int ref_slot, const double *xyz_device, int64_t m, double *d2_device);
/* Same with an upper bound per point: on entry d2_inout_device[i] bounds the answer (+inf = none), on exit it holds
 * min(bound, nearest squared distance here).  A rank whose points are all farther prunes at the root, which is what
 * makes the cross-rank step cheap: the querying rank passes the distance it already has.  A NEGATIVE bound marks a slot that
 * needs no answer (the padding of a fixed-capacity message, a rank's own queries): it comes back unchanged after one step. */
int me_nn_points_bounded(me_ctx *ctx, int ref_slot, const double *xyz_device, int64_t m, double *d2_inout_device);
/* me_nn_points_bounded for queries whose OWNER has already searched everything in a band of one axis: covered_device[2 i],
 * covered_device[2 i + 1] = [lo, hi) along `axis` — the owner's slab + halo, which holds every point of the cloud in that band
 * (me_halo_pack_device) — and d2_inout_device[i] = the nearest squared distance found there.  The caller thereby guarantees that no
 * point inside the band is closer than the bound; this rank then only has to look at the part of its tree OUTSIDE the band.  Same
 * result as me_nn_points_bounded — min(bound, nearest squared distance here) — for a fraction of the walk: without it a neighbour
 * disproves a far outlier (a ball of metres reaching across the face) cell by cell inside the strip both ranks hold
 * (the computeChamferDistance / getDiffRegResult searches have no distance limit, map_eval.cpp:1398-1431, :1100-1110). */
int me_nn_points_covered(me_ctx *ctx, int ref_slot, const double *xyz_device, int64_t m, double *d2_inout_device, int axis,
                         const double *covered_device);
/* The cross-rank step above as three calls on ONE fixed-capacity message per rank (round 5) — what the ranks all-gather and min-reduce:
 *   row 0                          [open queries map -> gt, open queries gt -> map, n_local_est, n_local_gt]
 *   rows 1 .. capacity             the open queries of the last me_nn1(ME_SLOT_EST, ME_SLOT_GT): x, y, z, bound (best squared distance so far)
 *   rows 1 + capacity .. 2 capacity  the same for me_nn1(ME_SLOT_GT, ME_SLOT_EST); unused rows carry the bound -1
 * me_nn_cross_message  writes this rank's message (1 + 2 capacity rows x 4 doubles, device memory); counts[2] = its open queries per
 *                      direction (more than `capacity`: the message carries the first `capacity`, the caller falls back to exactly
 *                      sized messages through me_nn_unresolved / me_nn_points_covered / me_nn_patch).
 * me_nn_cross_answer   the all-gathered messages of all ranks (world x (1 + 2 capacity) x 4) -> d2_device (world x (1 + 2 capacity)):
 *                      every slot of another rank = min(its bound, the nearest squared distance among the points held here, looking only
 *                      OUTSIDE the band [cuts[k] - halo, cuts[k + 1] + halo) of `axis` its owner k has searched completely — as
 *                      me_nn_points_covered); own slots and padding keep their bound, every rank's header slot is written as 0.  dir_mask: bit 0 / 1 = answer the map -> gt /
 *                      gt -> map block (a direction nobody else has open queries in is copied through).  cuts: host, world + 1 values.
 * me_nn_cross_patch    after the all-reduce MIN of d2_device over the ranks: this rank's block patches its open queries (me_nn_patch for
 *                      both directions at once). */
int me_nn_cross_message(me_ctx *ctx, double *msg_device, int64_t capacity, int64_t n_local_est, int64_t n_local_gt, int64_t counts[2]);
int me_nn_cross_answer(me_ctx *ctx, const double *gathered_device, int world, int64_t capacity, int own_rank, int dir_mask, int axis,
                       const double *cuts, double halo, double *d2_device);
int me_nn_cross_patch(me_ctx *ctx, const double *d2_reduced_device, int64_t capacity, int own_rank);
/* Overwrites the squared distances of the unresolved queries (same order as me_nn_unresolved returned them) with the
 * globally min-reduced values d2_device[count]. */
int me_nn_patch(me_ctx *ctx, int query_slot, const double *d2_device, int64_t count);
/* The per-point result of the last me_nn1(query_slot, ..) as it stands now (after me_nn_patch in slab mode): idx / d2 as
 * me_nn1 returns them (either may be NULL). */
int me_nn_fetch(me_ctx *ctx, int query_slot, int32_t *idx, double *d2);
/* Slab mode: the points this context holds of `slot`, in the order of its per-point outputs: orig_index[i] = the point's
 * position in the array that was uploaded (identity after me_upload_slab_device), owned[i] = 1 for the slab's own points,
 * 0 for halo.  Either array may be NULL; *count = me_cloud_size.  ME_ERR_CAPACITY when capacity < count. */
int me_slab_points(me_ctx *ctx, int slot, int64_t *orig_index, uint8_t *owned, int64_t capacity, int64_t *count);
/* Hand a context per-point results that were computed elsewhere (by the ranks of a distributed run, put together with
 * me_slab_points): afterwards me_render_entropy(slot) / me_render_distance(query_slot, ..) colour the WHOLE cloud held by
 * this context exactly as after me_mme / me_nn1 (map_entropy.pcd, raw_rendered_dis_map.pcd; map_eval.cpp:485-495, 686-736).
 * Arrays are host memory in cloud order, one entry per point of the slot. */
int me_set_mme_result(me_ctx *ctx, int slot, const double *entropies, const uint8_t *valid);
int me_set_nn_result(me_ctx *ctx, int query_slot, int ref_slot, const double *d2);

/* Slab mode, voxel partials: Gaussians of the OWNED points only, RAW second moments (M2 = sum (p-mu)(p-mu)^T, no
 * division), ascending key order; partials of the same voxel from different ranks merge with Chan's formula. */
int me_voxel_partials(me_ctx *ctx, int slot, double voxel_size, int32_t *keys /*V x 3*/, int32_t *npts /*V*/,
                      double *mu /*V x 3*/, double *m2 /*V x 9*/, int64_t *n_voxels);

/* Multi-GPU with DISTRIBUTED INPUT (no reference counterpart): every rank starts with 1/world of each cloud.
 *   me_transform_points_device   *cloud = cloud->Transform(T) (map_eval.cpp:1206) on a raw device buffer, in place — applied to
 *                                a rank's part of the estimated map BEFORE the exchange, so that slab membership is decided
 *                                on the exact transformed coordinate.
 *   me_halo_pack_device          the send side of the one-shot halo exchange.  cuts[world + 1] (host, ascending, cuts[0] = -inf,
 *                                cuts[world] = +inf) are the slab faces along `axis`; point p goes to EVERY rank k with
 *                                cuts[k] - halo <= p[axis] < cuts[k+1] + halo (the filter me_set_slab applies on the
 *                                receiving side).  out_device (capacity x 3) receives the points destination-major, in input
 *                                order inside a destination (deterministic); counts[world] the segment sizes — exactly the
 *                                send buffer and split sizes of one all_to_all.  out_device == NULL: counts only.
 *   me_voxel_partial_rows_device me_voxel_partials as rows [kx, ky, kz, n, mu(3), M2(9)] (16 doubles) in a device buffer:
 *                                what the all-gather of the voxel partials carries (rows with n == 0 are padding).
 *   me_voxel_merge_device        Chan's parallel update of the gathered rows of all ranks -> the slot's voxel table exactly as
 *                                VoxelCalculator::buildVoxelMap leaves it (voxel_calculator.cpp:21-56: M2/(n-1)^2 for n > 10);
 *                                when both slots hold a merged table of the same voxel size, me_awd_scs runs on them.
 *   me_upload_slab_device        me_upload_cloud_device for points that ARE this rank's slab + halo already (what the exchange
 *                                delivered, transform applied): me_set_slab's filter pass is skipped, ownership still follows
 *                                the slab. */
int me_transform_points_device(me_ctx *ctx, double *xyz_device, int64_t n, const double *T_rowmajor4x4);
int me_upload_slab_device(me_ctx *ctx, int slot, const double *xyz_device, int64_t n, double cell_size);
int me_halo_pack_device(me_ctx *ctx, const double *xyz_device, int64_t n, int axis, const double *cuts, int world, double halo,
                        double *out_device, int64_t capacity, int64_t *counts);
/* me_halo_pack_device that also packs, in the same order, tag_base + the input index of every copied point into tags_device
 * (capacity entries; may be NULL): the receiver of the exchange then knows which point of the WHOLE cloud an entry of its slab is
 * (the C++ host's per-point outputs: map_entropy.pcd, raw_rendered_dis_map.pcd, map_eval.cpp:485-495, 686-736). */
int me_halo_pack_tagged_device(me_ctx *ctx, const double *xyz_device, int64_t n, int axis, const double *cuts, int world, double halo,
                               double *out_device, int64_t *tags_device, int64_t tag_base, int64_t capacity, int64_t *counts);
/* voxel_size > 0: every index build of this context (and of its twin) from now on also emits the voxel run records of
 * VoxelCalculator::buildVoxelMap for that voxel size (voxel_calculator.cpp:21-56) while it gathers the sorted cloud; a later
 * me_voxel_gaussians / me_voxel_partials / me_voxel_partial_rows_device / me_awd_scs with the SAME size then has no pass over the cloud
 * left (a sort and a reduction of ~n / 60 records).  Results as without the hint (keys and populations exact, sums to 1e-9 of their
 * scale).  0: off (the default).  me_run_suite_from does this by itself for the duration of the call. */
int me_set_voxel_hint(me_ctx *ctx, double voxel_size);
/* The lean exchange (no reference counterpart; dist.py `lattice_plan`): the marginal histograms of a rank's part of a cloud on an
 * ABSOLUTE power-of-two lattice.  Bin i of axis a counts the finite coordinates with floor(x_a / w) == origin_bin[a] + i,
 * w = 2^(e0 + *level); *level is the smallest one for which every axis of this buffer fits ME_LATTICE_BINS bins.  neg_inf[a]
 * counts the coordinates that are -inf (me_halo_pack_device hands those to rank 0; NaN and +inf satisfy no slab's test).
 * hist_device: 3 x ME_LATTICE_BINS uint32, axis-major.  With the histograms of every rank's parts (one all-gather) each rank computes
 * the slab cuts AT BIN EDGES, a halo of whole bins and the exact size of every message of the halo exchange — x / w, floor and
 * (whole number) * w are exact in fp64, so me_halo_pack_device's comparisons against such cuts decide exactly what the bins say. */
#define ME_LATTICE_BINS 4096
int me_lattice_histograms_device(me_ctx *ctx, const double *xyz_device, int64_t n, int e0, int32_t *level, int64_t origin_bin[3],
                                 int64_t neg_inf[3], uint32_t *hist_device);
/* me_lattice_histograms_device for a rank's `clouds` (1 or 2) pieces at once, written as the rows of its gather message:
 * msg_device = clouds x (8 + 3 ME_LATTICE_BINS) int64, row = [level, origin_bin x y z, n, neg_inf x y z | the counts, axis-major] —
 * what me_lattice_plan_device reads.  Two launches per piece, one host read and one stream synchronisation for both. */
int me_lattice_messages_device(me_ctx *ctx, const double *xyz_a_device, int64_t n_a, const double *xyz_b_device, int64_t n_b, int clouds, int e0,
                               int64_t *msg_device);
/* The plan of the lean exchange from the gathered messages of all ranks: msgs_device = world x clouds rows (rank-major; the LAST cloud is
 * the ground truth, whose extent picks the slab axis) of 8 + 3 ME_LATTICE_BINS int64: [level, origin_bin x y z, n, neg_inf x y z |
 * me_lattice_histograms_device's counts, axis-major].  out (host, 4 + clouds + world - 1 + world * clouds * world int64):
 * [axis, level of the combined window, its first bin on that axis, halo in bins, points per cloud, the cut edges c_1 .. c_{world-1}
 * (bins from the window's first), then counts[source rank][cloud][destination rank]] — cut k = (first bin + c_k) * 2^(e0 + level),
 * halo = (halo in bins) * 2^(e0 + level).  Four small kernels; the same arithmetic, number for number, as dist.lattice_plan. */
int me_lattice_plan_device(me_ctx *ctx, const int64_t *msgs_device, int world, int clouds, double halo, int e0, int64_t *out);
int me_voxel_partial_rows_device(me_ctx *ctx, int slot, double voxel_size, double *rows_device, int64_t capacity, int64_t *n_rows);
int me_voxel_merge_device(me_ctx *ctx, int slot, double voxel_size, const double *rows_device, int64_t n_rows);

/* ---- clouds ------------------------------------------------------------------------------------------------ */
/* Replaces: *map_3d_ = map_3d_->Transform(initial_matrix) (map_eval.cpp:1206) + every KDTreeFlann::SetGeometry
 * (map_eval.cpp:1214,1227,1401-1402,1449,1551,1619): uploads the cloud, applies T (row-major 4x4, NULL = none;
 * homogeneous divide as Open3D), sorts it along a space-filling curve and builds the search index ONCE.
 * cell_size: edge of the radius-search grid cell (pass nn_radius; <= 0 = automatic, rebuilt lazily by me_mme).
 * Limits: more than 2^21 cells per axis -> ME_ERR_ARG "cell size too small for the cloud extent".  A cloud whose 1-NN octree
 * would need more than 17 levels (dense patches more than ~2^17 1-NN cells apart) is indexed WITHOUT the octree: the radius passes
 * (me_mme, me_local_geometry, ...) work; the calls that walk the octree — me_nn1, me_nn_points*, me_estimate_normals, me_fpfh,
 * me_statistical_outlier — return ME_ERR_ARG "octree deeper than the level table". */
int me_upload_cloud(me_ctx *ctx, int slot, const double *xyz_host, int64_t n, const double *T_rowmajor4x4,
                    double cell_size);
int me_upload_cloud_device(me_ctx *ctx, int slot, const double *xyz_device, int64_t n,
                           const double *T_rowmajor4x4, double cell_size);
/* open3d::geometry::PointCloud::VoxelDownSample (map_eval.cpp:38-39) on the cloud already on the device, in place:
 * voxel index = floor((p - (min_bound - voxel_size/2)) / voxel_size), one output point per occupied voxel = the mean of
 * its points accumulated in cloud order (bit-identical to the CPU arithmetic).  Output order: ascending voxel index
 * (Open3D: hash-map iteration order).  The index is rebuilt; *n_out = points kept.   */
int me_voxel_downsample(me_ctx *ctx, int slot, double voxel_size, int64_t *n_out);
/* *cloud = cloud->Transform(T) (map_eval.cpp:1206, :1392) on the cloud already on the device (row-major 4x4); the index
 * is rebuilt.  Lets MME run on the map as loaded and AC/COM/CD/AWD on the transformed map, as the reference does. */
int me_transform_cloud(me_ctx *ctx, int slot, const double *T_rowmajor4x4);

/* ---- simulation mode: evaluate_noised_gt (map_eval_main.cpp:177-183, map_eval.h:79,87) -------------------------------------- */
/* The estimated map as a perturbed copy of a resident cloud.  Stages, in this order, each switchable:
 *   1. addLocalDeformation  (map_eval.cpp:1808-1829): d = |p - c| as Eigen's norm(); if d < R: p += (p - c) / d * s * w,
 *      w = 0.5 (1 + cos(pi d / R)); a point at d == 0 stays (normalize() leaves a zero vector).  No randomness.
 *   2. addNonUniformDensity (:1757-1784) on the deformed point: keep iff u < sparse_ratio where
 *      sin(x / region_size pi) sin(y / region_size pi) > 0, u < dense_ratio elsewhere; survivors keep the source order.
 *   3. addGaussianNoise     (:1745-1755): + N(0, noise_std^2) per coordinate of every survivor.
 *   4. addSparseOutliers    (:1786-1806): m = (int64)(n_kept outlier_ratio) outliers appended after the survivors; outlier j =
 *      point b = min(n_kept - 1, (int64)(u n_kept)) of the noised, compacted cloud + N(0, outlier_range^2) per axis (the clamp is
 *      a guard: the reference reads one past the end if its draw rounds to 1.0; with u < 1 below the product stays < n_kept).
 * Randomness: Philox4x64-10 (Random123) with key (seed, 0) — the reference's mt19937 is seeded from std::random_device, so no run of
 * it can be reproduced; here every block is a pure function of (seed, counter):
 *   density of source point i  counter (i, 1, 0, 0)  w0 -> u
 *   noise of source point i    counter (i, 2, 0, 0)  Box-Muller (w0, w1) -> x, y; (w2, w3) -> z (its second normal unused)
 *   outlier j                  counter (j, 3, 0, 0)  w0 -> u of the base index; Box-Muller (w1, w2) -> x, y
 *                              counter (j, 3, 1, 0)  Box-Muller (w0, w1) -> z
 * u = (w >> 11) 2^-53 in [0, 1); Box-Muller (a, b): u1 = ((a >> 11) + 1) 2^-53 in (0, 1], u2 = u(b),
 * n = sqrt(-2 ln u1) cos(2 pi u2), and sin(2 pi u2) for the pair's second.  i is the index in the source's order: a surviving
 * point gets the same noise whatever the density stage dropped, and nothing depends on the launch shape.
 * dst gets the upload-time reset (index rebuilt on the source's cell size; NN, MME, voxel state invalidated; normals and
 * covariances dropped; the other slot's NN result invalidated); src is left untouched unless dst == src (in place works).
 * *n_out = points in dst.  ME_ERR_ARG: p NULL, slab or shard mode, noise_std < 0 or non-finite, a ratio outside [0, 1],
 * outlier_range < 0 or non-finite, a non-finite deform_strength or deform_center while the deform stage is on (deform_radius =
 * +inf is legal: w = 1, every point is pushed by deform_strength along its direction; a NaN deform_radius or region_size
 * switches its stage off), an output of 2^31 points or more, or no survivor.  ME_ERR_STATE: src not uploaded, or uploaded but
 * empty (a me_mesh_scan without a hit).  A refused call leaves dst as it was.  Device timer "perturb". */
typedef struct me_perturb_params {
    double noise_std;                    /* addGaussianNoise noise_std_dev (map_eval.cpp:1746)            (0 = off)    */
    double sparse_ratio, dense_ratio;    /* addNonUniformDensity keep probabilities (:1758-1759)                       */
    double region_size;                  /*   its region_size (:1760)                                       (<= 0 = off) */
    double outlier_ratio, outlier_range; /* addSparseOutliers (:1787-1788)                                  (ratio 0 = off) */
    double deform_radius, deform_strength, deform_center[3]; /* addLocalDeformation (:1809-1811)    (radius <= 0 or strength 0 = off) */
    uint64_t seed;                       /* Philox key word 0 (no reference counterpart: std::random_device)            */
} me_perturb_params;
int me_perturb_cloud(me_ctx *ctx, int dst_slot, int src_slot, const me_perturb_params *p, int64_t *n_out);

/* ---- coarse global registration: the initial pose (the reference's FAQ "How to obtain initial pose?": by hand in CloudCompare) --- */
/* Open3D's compute_fpfh_feature + registration_ransac_based_on_feature_matching, on the device.
 *
 * me_voxel_downsample_into: me_voxel_downsample of src_ctx's src_slot written into dst_ctx's dst_slot; src is untouched.  The
 * result (points, order, index) is bit-identical to uploading src's points into dst with src's cell size and calling
 * me_voxel_downsample there.  dst gets the upload-time reset (no normals, features, NN, MME or voxel state).  dst_ctx may be
 * src_ctx (another slot); its stream waits for src_ctx's pending work.  ME_ERR_ARG: different devices, the same (context, slot),
 * slab or shard mode, voxel_size <= 0.  Device timer "downsample" of dst_ctx.
 *
 * me_fpfh: Fast Point Feature Histograms (Open3D ComputeFPFHFeature) of a resident cloud, N x 33.
 *   normals: those of the slot (me_set_normals / me_estimate_normals / averaged by a down-sample) are used as they are; a slot
 *            without normals gets me_estimate_normals(normal_knn) first (1..40).
 *   neighbours: Open3D's KDTreeSearchParamHybrid(radius, max_nn) — the max_nn nearest points (the exact k-NN walk of
 *            me_estimate_normals, ascending by (d2, index)) with d2 < radius^2, the query itself removed by index.  1 <= max_nn <= 40:
 *            Open3D's tutorial value of 100 is clipped to 40 (the k-NN walk keeps its list in LDS).
 *   pair feature of (p1, n1, p2, n2): d = p2 - p1, L = sqrt((dx dx + dy dy) + dz dz), L == 0 -> (0, 0, 0); a1 = n1.d / L,
 *            a2 = n2.d / L; if |a1| < |a2| the roles swap (n2, n1, -d) and f2 = -a2, else f2 = a1 (Open3D's acos(|a1|) > acos(|a2|)
 *            without the library call); v = d x n1', |v| == 0 -> (0, 0, 0), v /= |v|; w = n1' x v; f1 = v.n2';
 *            f0 = atan2(w.n2', n1'.n2').  Dots are (x x' + y y') + z z'.
 *   SPFH of a point with m >= 1 neighbours: each adds 100 / m to the bins floor(11 (f0 + pi) / (2 pi)), 11 + floor(11 (f1 + 1) / 2),
 *            22 + floor(11 (f2 + 1) / 2), each index clamped to [0, 10]; m = 0: all zeros.
 *   FPFH: sum over the neighbours in list order of SPFH(j) / d2 (d2 == 0 skipped: Open3D weighs by the SQUARED distance), each
 *            11-bin block scaled by 100 / block sum when that sum is nonzero, then + SPFH(i).
 * The features stay on the device with the slot; an upload, down-sample, perturbation, transform or new normals drops them.
 * features: N x 33 host array in the caller's (cloud) order, nullable.  Device timer "fpfh" (its normal estimation: "normals").
 *
 * me_fpfh_match: exact 1-NN in the 33-dimensional feature space, both directions: squared distance = a sequential fp64 sum over the
 * dimensions in index order (no contraction), ties to the smallest index.  corr[i] (n_src entries, host, nullable) = the reference
 * point matched to source point i, or -1; mutual = 1 keeps i -> j only when j -> i (Open3D's mutual_filter).  *n_corr = entries
 * != -1.  Both slots need me_fpfh features (ME_ERR_STATE).  Device timer "fpfh_match".
 *
 * me_global_register: RANSAC over the correspondences (i, corr[i]) in ascending i, on the device.  Hypothesis h < max_iterations
 * is a pure function of (seed, h): Philox4x64-10 counter (h, 4, 0, 0), key (seed, 0) -> w0, w1, w2; sample k_j = mulhi64(w_j,
 * n_corr) (the high word of w_j n_corr).  It is INVALID when two samples coincide; when an edge fails the two-sided length check
 * (|s_a - s_b| < edge_ratio |t_a - t_b| or |t_a - t_b| < edge_ratio |s_a - s_b|, Open3D's CorrespondenceCheckerBasedOnEdgeLength);
 * when the source triangle is degenerate: |e01 x e02|^2 <= 1e-12 |e01|^2 |e02|^2 (sine of its angle at s0 <= 1e-6); or when, after
 * the fit, a sampled pair is farther than max_corr_dist (d2 > eps^2, CorrespondenceCheckerBasedOnDistance).  The fit is Horn's
 * method of csrc/me_horn.hpp on the three pairs.  The valid hypotheses are scored (in batches, hypothesis order kept): the count of
 * correspondences with |R s + t - q|^2 < eps^2, fp64, ((R_r0 x + R_r1 y) + R_r2 z) + t_r, ((dx dx + dy dy) + dz dz).  The top
 * validate_top by (score desc, h asc) are re-scored on the whole source cloud (every point moved, 1-NN in ref_slot as me_nn_points,
 * inlier iff d2 < eps^2): fitness = inliers / N_src, inlier_rmse = sqrt(sum d2 / inliers) (0 without inliers), as Open3D evaluates
 * a RANSAC hypothesis.  The winner is the best by (fitness desc, rmse asc, h asc); T_out (row-major 4x4) maps the source's current
 * coordinates to ref_slot's frame; the source slot is not moved.  No confidence early stop: every hypothesis is drawn.
 * Features are computed with p->fpfh on a slot that has none.  scores (max_iterations entries, host, nullable): the correspondence
 * inliers of hypothesis h, -1 = invalid.  ME_ERR_STATE: fewer than 3 correspondences, or no valid hypothesis (with a message).
 * ME_ERR_ARG: bad parameters (max_corr_dist <= 0, edge_ratio outside (0, 1], max_iterations < 1, validate_top < 1), src == ref,
 * slab or shard mode.  Device timers "ransac" (sampling, fit, scoring), "ransac_validate" (the re-scoring without its 1-NN search,
 * which counts to "nn1"), and "fpfh" / "fpfh_match" of its own feature work. */
int me_voxel_downsample_into(me_ctx *src_ctx, int src_slot, me_ctx *dst_ctx, int dst_slot, double voxel_size, int64_t *n_out);
typedef struct me_fpfh_params {
    double radius;   /* KDTreeSearchParamHybrid radius                                       */
    int max_nn;      /*   its max_nn, 1..40                                                   */
    int normal_knn;  /* k of the normal estimation of a slot without normals, 1..40          */
} me_fpfh_params;
int me_fpfh(me_ctx *ctx, int slot, const me_fpfh_params *p, double *features);
int me_fpfh_match(me_ctx *ctx, int src_slot, int ref_slot, int mutual, int32_t *corr, int64_t *n_corr);
typedef struct me_globreg_params {
    me_fpfh_params fpfh;        /* computed on both slots when absent                                    */
    double max_corr_dist;       /* epsilon: inlier iff d2 < epsilon^2 (strict, the library's convention)  */
    double edge_ratio;          /* 0.9, CorrespondenceCheckerBasedOnEdgeLength                           */
    int64_t max_iterations;     /* hypotheses drawn; no confidence early stop                            */
    int validate_top;           /* K hypotheses re-scored on the whole cloud (default 64)                */
    int mutual;                 /* feature-match mutual filter                                           */
    uint64_t seed;              /* Philox key word 0                                                     */
} me_globreg_params;
typedef struct me_globreg_info {
    int64_t n_corr, n_valid_hypotheses, best_hypothesis, best_corr_inliers;
    double fitness, inlier_rmse; /* of the chosen T against ref_slot, 1-NN, gate d2 < epsilon^2              */
} me_globreg_info;
int me_global_register(me_ctx *ctx, int src_slot, int ref_slot, const me_globreg_params *p, double T_out[16], me_globreg_info *info,
                       int64_t *scores);

/* ---- outlier removal: Open3D 0.15's PointCloud::RemoveStatisticalOutlier / RemoveRadiusOutlier on a resident cloud -------------- */
/* (DESIGN.md section 4.8).  Single GPU only: slab or shard mode is ME_ERR_ARG.  Every per-point host output (N entries, nullable)
 * is in the slot's cloud order, the order of me_download_cloud.  Each call leaves a uint8 keep-mask on the slot, held until the
 * cloud changes (upload, down-sample, transform, perturbation, selection); me_outlier_select_into applies it.
 *
 * me_statistical_outlier (k = nb_neighbors in [1, 40], std_ratio > 0, else ME_ERR_ARG): the neighbours of point i are its k nearest
 * points of the same cloud, itself included (at d2 = 0), all n points when n < k; d2 = ((dx*dx + dy*dy) + dz*dz) in fp64.  Ties at
 * the k-th distance need no rule: only the multiset of the k smallest d2 is used.  avg_dist[i] = the sum of sqrt(d2_j) in ascending d2
 * order, starting from 0, divided by the neighbour count.  mean = (sum of avg_i > 0) / n — Open3D divides by every point —,
 * std_dev = sqrt(sum over avg_i > 0 of (avg_i - mean)^2 / (n - 1)), threshold = mean + std_ratio std_dev; both sums in a fixed
 * order (bit-identical from run to run).  keep[i] = avg_i > 0 && avg_i < threshold.  So k = 1 keeps nothing, nor does n = 1 (the
 * threshold is NaN), and a point whose neighbours all coincide with it is dropped.  info->n_fallback = the points the exact
 * octree walk settled (the grid pass could not).  Device timer "outlier".
 *
 * me_radius_outlier (nb_points >= 0, radius > 0): counts[i] = the points j with d2 < radius^2 (strict, the library's radius
 * convention), i itself included; keep[i] = counts[i] > nb_points.  The slot's radius grid is rebuilt at the radius when its cell
 * differs, as me_mme does.  info: mean = std_dev = 0, threshold = nb_points, n_fallback = 0.  Device timer "outlier".
 *
 * me_outlier_select_into: the points of src_slot whose mask entry is 1, in cloud order, written into dst_ctx's dst_slot — in place
 * when (dst_ctx, dst_slot) is (src_ctx, src_slot); otherwise src is untouched and dst_ctx (same device) waits for src_ctx's pending
 * work.  Normals travel with their points; covariances, FPFH features, NN and MME results of dst are dropped and its index is
 * rebuilt (src's cell size), as after me_voxel_downsample.  ME_ERR_STATE: src has no mask, or the mask keeps no point.  *n_out = the
 * points kept.  Device timer "outlier_select" of dst_ctx. */
typedef struct me_outlier_info {
    int64_t n_in, n_kept, n_fallback;
    double mean, std_dev, threshold; /* statistical as defined above; radius: 0, 0, nb_points */
} me_outlier_info;
int me_statistical_outlier(me_ctx *ctx, int slot, int nb_neighbors, double std_ratio, double *avg_dist, uint8_t *keep,
                           me_outlier_info *info);
int me_radius_outlier(me_ctx *ctx, int slot, int nb_points, double radius, int32_t *counts, uint8_t *keep, me_outlier_info *info);
int me_outlier_select_into(me_ctx *src_ctx, int src_slot, me_ctx *dst_ctx, int dst_slot, int64_t *n_out);

/* ---- clustering: Open3D 0.15's PointCloud::ClusterDBSCAN on a resident cloud, and a cluster-size filter ------------------------ */
/* (DESIGN.md section 4.9).  Single GPU only: slab or shard mode is ME_ERR_ARG.  Every per-point host output (N entries, nullable)
 * is in the slot's cloud order, the order of me_download_cloud.  Labels and sizes stay with the slot until the cloud changes (upload,
 * down-sample, transform, perturbation, selection).  The slot's radius grid is rebuilt at eps when its cell differs, as
 * me_radius_outlier does.  Device timer "cluster".
 *
 * me_cluster_dbscan (eps > 0 finite, min_points >= 1, else ME_ERR_ARG).  The result is a function of the cloud alone:
 *   1. d2 = ((dx*dx + dy*dy) + dz*dz) in fp64, no FMA.  j is a neighbour of i iff d2 < eps*eps (strict, the library's radius
 *      convention).  counts[i] = the number of neighbours of i, i itself included.
 *   2. i is a core point iff counts[i] >= min_points.
 *   3. Two core points are in the same cluster iff a chain of core points connects them, consecutive ones being neighbours.
 *   4. Clusters are numbered 0 .. n_clusters - 1 in ascending order of their smallest core point index (cloud order).
 *   5. A non-core point with at least one core neighbour is a border point; its label is the smallest cluster id among its core
 *      neighbours' clusters.
 *   6. Every other point is noise, label -1.
 * info: n_core + n_border + n_noise = n_in; largest = the largest cluster's size (0 without clusters).
 *
 * me_cluster_sizes: sizes[c] = the points labelled c (core and border), c < *n_clusters.  sizes NULL: only the count.
 * ME_ERR_CAPACITY: capacity < *n_clusters (the count is still written).  ME_ERR_STATE: no current labels.
 *
 * me_cluster_keep (min_cluster_size >= 1, keep_largest >= 0, else ME_ERR_ARG; ME_ERR_STATE without current labels):
 * keep[i] = label[i] >= 0 && size[label[i]] >= min_cluster_size && (keep_largest == 0 || rank[label[i]] < keep_largest), where rank
 * orders the clusters by descending size, ties by ascending id.  It writes the slot's outlier keep-mask: me_outlier_select_into
 * applies it.  info: n_in, n_kept, threshold = min_cluster_size, the other fields 0. */
typedef struct me_cluster_info {
    int64_t n_in, n_clusters, n_core, n_border, n_noise, largest;
} me_cluster_info;
int me_cluster_dbscan(me_ctx *ctx, int slot, double eps, int min_points, int32_t *labels, int32_t *counts, me_cluster_info *info);
int me_cluster_sizes(me_ctx *ctx, int slot, int64_t *sizes, int64_t capacity, int64_t *n_clusters);
int me_cluster_keep(me_ctx *ctx, int slot, int64_t min_cluster_size, int64_t keep_largest, uint8_t *keep, me_outlier_info *info);

/* ---- local geometry: mean plane variance (MPV) and the eigenvalue shape features of every radius neighbourhood --------------- */
/* (DESIGN.md section 4.10).  MPV is MME's no-reference companion (Razlaw et al. 2015; Kornilova and Ferrer 2021): the mean, over the
 * valid points, of the smallest eigenvalue of the neighbourhood covariance.  Single GPU only: slab or shard mode is ME_ERR_ARG.
 * The slot's radius grid is rebuilt at `radius` when its cell differs, as me_mme does.  Device timer "local_geom".
 *
 * me_local_geometry (radius finite and > 0, min_k >= 2, else ME_ERR_ARG).  Per point i:
 *   1. j is a neighbour iff d2 = ((dx*dx + dy*dy) + dz*dz) < radius*radius (fp64, no FMA, strict: the set me_mme uses); the query
 *      itself is removed once, its coincident duplicates stay.  k_i = the neighbours left.
 *   2. k_i >= min_k: C = (sum(d d^T) - sum(d) sum(d)^T / k) / (k - 1) with d = p_j - p_i (moments about the query: no term
 *      exceeds radius^2, so each eigenvalue is within 8 k 2^-53 radius^2 of the exact one), eigenvalues by cyclic Jacobi, clamped at
 *      0 from below, ordered l1 >= l2 >= l3.
 *   3. The point is valid iff k_i >= min_k and l1 > 0; an invalid point stores l1 = l2 = l3 = 0.
 * out: n, n_valid and, over the valid points, the sums of l3 (MPV = sum_l3 / n_valid), linearity (l1 - l2) / l1, planarity
 * (l2 - l3) / l1, sphericity l3 / l1, surface variation l3 / (l1 + l2 + l3), and k.  The sums are formed from per-block partials in
 * block order: bit-identical from run to run.
 *
 * me_local_geometry_fetch: the per-point arrays of the slot's last me_local_geometry in cloud order (N entries each, nullable):
 * eig = N x 3 (l1, l2, l3), k, valid.  ME_ERR_STATE: no current result — the cloud changed (upload, down-sample, transform,
 * perturbation, selection) or another stage rebuilt the slot's grid at a different cell. */
typedef struct me_local_geom_out {
    int64_t n, n_valid;
    double sum_l3, sum_linearity, sum_planarity, sum_sphericity, sum_surface_variation;
    int64_t sum_k;
} me_local_geom_out;
int me_local_geometry(me_ctx *ctx, int slot, double radius, int min_k, me_local_geom_out *out);
int me_local_geometry_fetch(me_ctx *ctx, int slot, double *eig, int32_t *k, uint8_t *valid);

/* ---- radius-search normals: the eigenVECTOR of the same covariance ------------------------------------------------------------- */
/* (DESIGN.md section 4.14).  me_estimate_normals is k-NN (Open3D's default): its neighbourhood in metres changes with the density,
 * which is wrong for a metric.  me_radius_normals takes the neighbourhood of me_local_geometry — a fixed radius — in the same
 * kernel pass.  Single GPU only: slab or shard mode is ME_ERR_ARG.  Device timer "radius_normals".
 *
 * me_radius_normals (radius finite and > 0, min_k >= 2, out non-NULL, else ME_ERR_ARG; viewpoint = 3 finite doubles or NULL).
 *   1. Neighbour set, moments about the query, covariance, cyclic Jacobi, clamp and ordering: steps 1 - 3 of me_local_geometry,
 *      the same arithmetic.  The call ALSO stores the slot's local-geometry result (eigenvalues, k, validity; a new serial),
 *      bit-identical to what me_local_geometry(slot, radius, min_k) stores: me_local_geometry_fetch and me_mom work after either.
 *   2. The normal of a valid point: the column of Jacobi's V that belongs to the smallest eigenvalue BEFORE the clamp; among equal
 *      eigenvalues the column with the LOWEST index (d[0], d[1], d[2] in Jacobi's own order: b = 0; d[1] < d[b] -> 1; d[2] < d[b]
 *      -> 2).  The column is scaled once to unit length, n / sqrt((nx*nx + ny*ny) + nz*nz): the accumulated rotations leave it
 *      within some 1e-15 of unit length, the scaling within 3 ulp.
 *   3. Sign.  viewpoint == NULL: as Jacobi yields it — a pure function of the cloud, identical from run to run and from a fresh
 *      context.  Otherwise, with v = viewpoint - p_i component by component, n is negated iff ((nx*vx + ny*vy) + nz*vz) < 0.
 *   4. An invalid point (k_i < min_k, or l1 == 0) gets (0, 0, 0); with invalid_z != 0 it gets (0, 0, 1), what me_estimate_normals
 *      writes where a normal is undefined and what the ICP / GICP consumers expect.
 * The normals go into the slot's normals (cloud order), as me_set_normals / me_estimate_normals put theirs: they follow
 * me_transform_cloud (n <- R n), me_get_normals, me_icp_lsq_sums and me_gicp_covariances; covariances on the slot are dropped, as
 * me_set_normals drops them.  out: n, n_valid, sum_k (over the valid points).
 * ORDER OF USE: like me_local_geometry the call may rebuild the slot's index at the radius level, which discards the 1-NN result
 * of the slot and of its twin, the other slot (it searched in this one) — estimate the normals first, then call me_nn1. */
typedef struct me_radius_normals_out {
    int64_t n, n_valid, sum_k;
} me_radius_normals_out;
int me_radius_normals(me_ctx *ctx, int slot, double radius, int min_k, const double *viewpoint, int invalid_z, me_radius_normals_out *out);

/* ---- plane segmentation: RANSAC plane fit and multi-plane extraction on a resident cloud ---------------------------------------- */
/* (DESIGN.md section 4.11).  The model is Open3D's PointCloud::SegmentPlane(distance_threshold, 3, num_iterations), applied
 * repeatedly to what is left; the deviations are listed in DESIGN.md section 5.  Single GPU only: slab or shard mode is ME_ERR_ARG.
 * No index is needed.  Device timers "plane_score" (the scoring kernel) and "plane" (everything else).
 *
 * me_segment_planes.  Parameters: distance_threshold t finite and > 0, 1 <= num_iterations H <= 2^24, 1 <= max_planes P <= 64,
 * min_inliers >= 3, refit 0 or 1, else ME_ERR_ARG.  The result is a pure function of (cloud, parameters, seed).  Round r = 0, 1, ...
 * works on the REMAINING points — those without a label yet, m of them, in ascending cloud index (the order of me_download_cloud):
 *   1. Hypothesis h < H of round r: Philox4x64-10 counter (h, 5, r, 0), key (seed, 0) -> w0, w1, w2 (counter word 1 = 5 names this
 *      call); k_j = mulhi64(w_j, m); the sample p_j is the k_j-th remaining point.  The hypothesis is INVALID when two k_j coincide
 *      or when |e01 x e02|^2 <= 1e-12 |e01|^2 |e02|^2, e01 = p1 - p0, e02 = p2 - p0 (cross / dot as in me_global_register:
 *      dot(u, v) = (u0 v0 + u1 v1) + u2 v2, the test is dot(cr, cr) <= (1e-12 * dot(e01, e01)) * dot(e02, e02)).
 *   2. Plane of a valid hypothesis: cr = e01 x e02, L = sqrt(dot(cr, cr)), n = cr / L component by component; n is negated when
 *      c < 0, or c == 0 && b < 0, or c == b == 0 && a < 0; d = -((a x0 + b y0) + c z0).  fp64, no contraction.
 *   3. Score: s_i = ((a x_i + b y_i) + c z_i) + d for every remaining point; i is an inlier iff |s_i| < t (strict, the library's
 *      convention); score[h] = the number of inliers, an exact integer; -1 for an invalid hypothesis.
 *   4. Winner: the largest score, ties to the smallest h.  The round ENDS the extraction, producing no plane, when m < 3 (nothing is
 *      drawn: every score of the round is -1), when no hypothesis is valid, or when the best score is < min_inliers.
 *   5. The winner's inliers get label r and leave the remaining set.
 *   6. Returned plane.  refit = 0: the winner's (a, b, c, d).  refit = 1: the least-squares plane of the inliers — moments about
 *      o = the winner's p0, M1 = sum(p - o), M2 = sum (p - o)(p - o)^T (per-block partials combined in block order: bit-identical
 *      from run to run), C = (M2 - M1 M1^T / k) / k, the normal = the eigenvector of the smallest eigenvalue by cyclic Jacobi, the
 *      sign rule of step 2, d = -dot(n, o + M1 / k).  When the two smallest eigenvalues are equal to working precision,
 *      l2 - l3 <= 8 k 2^-53 D^2 with D = the largest |p - o|, the hypothesis plane is returned and refit_degenerate is set.
 *      The labels are NOT recomputed after the refit (upstream's order).
 *   7. Record of plane r: count, the winning h and its score (= count), the plane, rms = sqrt(sum s^2 / count), mean_abs and max_abs
 *      of the inliers' residuals against the RETURNED plane (sums in fixed block order), refit_degenerate.
 *   8. The extraction stops after P planes or at the first round that ends it.  n_planes >= 0 is a result, not an error: a cloud of
 *      collinear points returns ME_OK with n_planes = 0.
 * Host outputs (nullable): planes[max_planes] (the first n_planes are written), labels[N] in cloud order (-1 = no plane),
 * scores[max_planes x num_iterations] (row r = the scores of round r; rows of rounds that were never started hold -1).
 * info: n_in, n_planes, n_labelled, n_valid_hypotheses (summed over the rounds), rounds = the rounds started (the one that ended the
 * extraction included).  Labels and records stay on the slot until the cloud changes (upload, down-sample, transform, perturbation,
 * selection), as the cluster labels do.
 *
 * me_plane_fetch: the records and labels of the slot's last me_segment_planes (both nullable; *n_planes is always written).
 * ME_ERR_STATE: no current labels.  ME_ERR_CAPACITY: capacity < *n_planes (the count is still written).
 *
 * me_plane_keep (plane = -1 or 0 <= plane < n_planes, invert 0 or 1, else ME_ERR_ARG; ME_ERR_STATE without current labels):
 * keep[i] = (plane >= 0 ? label[i] == plane : label[i] >= 0) != invert.  It writes the slot's outlier keep-mask:
 * me_outlier_select_into applies it.  Ground removal is (plane 0, invert 1), keeping only planar structure (-1, 0).
 * info: n_in, n_kept, threshold = plane, the other fields 0. */
typedef struct me_plane_params {
    double distance_threshold;
    int64_t num_iterations;
    int32_t max_planes;
    int32_t refit;
    int64_t min_inliers;
    uint64_t seed; /* Philox key word 0 */
} me_plane_params;
typedef struct me_plane_record {
    int64_t count, h, score;
    double plane[4]; /* a, b, c, d: a x + b y + c z + d = 0, |(a, b, c)| = 1 */
    double rms, mean_abs, max_abs;
    int32_t refit_degenerate, reserved;
} me_plane_record;
typedef struct me_plane_info {
    int64_t n_in, n_planes, n_labelled, n_valid_hypotheses, rounds;
} me_plane_info;
int me_segment_planes(me_ctx *ctx, int slot, const me_plane_params *p, me_plane_record *planes, int32_t *labels, int64_t *scores,
                      me_plane_info *info);
int me_plane_fetch(me_ctx *ctx, int slot, me_plane_record *planes, int64_t capacity, int64_t *n_planes, int32_t *labels);
int me_plane_keep(me_ctx *ctx, int slot, int plane, int invert, uint8_t *keep, me_outlier_info *info);

/* ---- MOM: plane variance on mutually orthogonal planes, aggregated by exact medians ---------------------------------------------- */
/* (DESIGN.md section 4.12).  The mutually orthogonal metric of Kornilova and Ferrer 2021: the smallest covariance eigenvalue l3 of
 * me_local_geometry, taken only on the points of planes (me_segment_planes) whose directions are mutually orthogonal, and aggregated
 * per axis by the median.  Three pieces: a grouped exact order statistic on the device, the choice of the axes on the host, and the
 * metric on a resident cloud.
 *
 * me_group_order_stats (1 <= n_groups <= 64 and n >= 0, else ME_ERR_ARG; host pointers, values / group of n entries).  group[i] in
 * [-1, n_groups), -1 = the entry is ignored; values finite and >= 0 (-0.0 counts as +0.0).  Anything else is ME_ERR_ARG, detected on
 * the device and reported after the call (`out` is then unspecified).  The selection key of an entry is the bit pattern of v + 0.0
 * read as an unsigned 64-bit integer: on non-negative doubles its order is the numeric order.  Per group g, over its entries:
 *   count           their number
 *   sum             per-block partials (tiles of 2048 entries; inside a tile a fixed tree) combined in block order, 256 chunks, then one
 *                   block: no floating-point atomics, bit-identical from run to run
 *   min, max        the smallest and the largest entry
 *   lower, upper    sorted[(count - 1) / 2] and sorted[count / 2]: the two middle elements (the same one for an odd count)
 * count, min, max, lower and upper are EXACT — elements of the input, found by a radix select over the keys (eight passes of eight
 * bits, integer histograms: independent of any order).  The median is (lower + upper) / 2, formed by the caller in exactly this
 * form.  A group without an entry has every field 0.  Device timer "group_select".
 *
 * me_mom_select_axes: pure host arithmetic, no context (like me_nn_finalize).  0 <= cos_orthogonal < cos_parallel <= 1,
 * min_axis_points >= 1, 0 <= n_planes <= 64, planes / p / axes non-NULL (planes and dir_of_plane may be NULL when n_planes = 0), else
 * ME_ERR_ARG.  With dot(u, v) = (u0 v0 + u1 v1) + u2 v2 (fp64, no contraction), n_r = planes[r].plane[0..2], c_r = planes[r].count:
 *   1. Directions.  r ascending: plane r joins the SMALLEST existing direction g with |dot(n_r, rep_g)| >= cos_parallel, rep_g = the
 *      normal of the plane that founded g; otherwise it founds a new direction.  dir_of_plane[r] = g; W_g = the sum of its c_r.
 *   2. A direction is eligible iff W_g >= min_axis_points.
 *   3. g and h are orthogonal iff |dot(rep_g, rep_h)| <= cos_orthogonal.  Both thresholds are inclusive.
 *   4. The largest s in {3, 2, 1} with an eligible, pairwise orthogonal s-subset; among those subsets the largest min W, then the
 *      largest sum W, then the lexicographically smallest ascending tuple.  n_axes = s (0 without an eligible direction); the axes in
 *      ascending g, each with its direction, the number of its planes, W and rep.  Unused axis entries are zero.
 * The thresholds are cosines, so that no trigonometry has to agree between languages.
 *
 * me_mom (parameters as above, else ME_ERR_ARG; single GPU only: slab or shard mode is ME_ERR_ARG).  ME_ERR_STATE unless the slot
 * holds both a current me_local_geometry result and current me_segment_planes labels; the two stages may run in either order
 * (me_segment_planes builds no index, me_local_geometry discards only what depends on the sorted order).  The axes are chosen from
 * the slot's plane records as me_mom_select_axes does.  Point i is USED by axis a iff its label is >= 0, the direction of its plane
 * is axis a, and its local-geometry validity byte is set; it then contributes its l3 to the group a of me_group_order_stats.  Per
 * axis: direction, n_planes, rep, n_points = W (the labelled points of the direction), n_valid = the used points, sum_l3, min, max,
 * lower, upper and median = (lower + upper) / 2 of their l3.  mom_median = the sum of the medians in axis order (map_metrics'
 * definition), mom_mean = the sum of sum_l3 / n_valid; an axis without a used point contributes 0 to both and says so by
 * n_valid = 0.  n_axes = 0 is a result (ME_OK, both metrics 0), not an error.  Device timers "mom" and "group_select".
 *
 * me_mom_fetch: axis[N] in cloud order, the axis that used the point, -1 = not used.  ME_ERR_STATE without a current me_mom result:
 * it is dropped with the labels and with the eigenvalues (a changed cloud, a later me_segment_planes or me_local_geometry). */
typedef struct me_group_stats {
    int64_t count;
    double sum, min, max, lower, upper;
} me_group_stats;
typedef struct me_mom_params {
    double cos_parallel;     /* planes whose normals have |dot| >= this share a direction */
    double cos_orthogonal;   /* directions whose representatives have |dot| <= this are orthogonal */
    int64_t min_axis_points; /* labelled points a direction needs to be eligible */
} me_mom_params;
typedef struct me_mom_axis_choice {
    int32_t direction, n_planes;
    int64_t weight; /* W */
    double rep[3];
} me_mom_axis_choice;
typedef struct me_mom_axes {
    int32_t n_axes, n_directions;
    me_mom_axis_choice axis[3];
} me_mom_axes;
typedef struct me_mom_axis {
    int32_t direction, n_planes;
    double rep[3];
    int64_t n_points, n_valid;
    double sum_l3, min, max, lower, upper, median;
} me_mom_axis;
typedef struct me_mom_out {
    int32_t n_axes, n_directions;
    me_mom_axis axis[3];
    double mom_median, mom_mean;
} me_mom_out;
int me_group_order_stats(me_ctx *ctx, const double *values, const int32_t *group, int64_t n, int32_t n_groups, me_group_stats *out);
int me_mom_select_axes(const me_plane_record *planes, int32_t n_planes, const me_mom_params *p, int32_t *dir_of_plane, me_mom_axes *axes);
int me_mom(me_ctx *ctx, int slot, const me_mom_params *p, me_mom_out *out);
int me_mom_fetch(me_ctx *ctx, int slot, int8_t *axis);

/* ---- Error distribution: exact quantiles, Hausdorff distance, F-score counts, error histogram --------------------------------------- */
/* (DESIGN.md section 4.13).  Everything the library reported about a direction's 1-NN distances was a mean: the truncated RMSE of
 * AC, the mean of CD (computeChamferDistance, map_eval.cpp:1398-1431), one count ratio per threshold; the reference's own attempt at
 * more, f1_vec (map_eval.cpp:1245-1253), mixes a ratio with metres and is reproduced as it is.  These calls add the shape of the
 * error.  Every quantity they return except the two sums is an element of the input or an integer count.
 *
 * me_rank_select (host pointers; n >= 0, 0 <= n_ranks <= ME_RANK_MAX, else ME_ERR_ARG).  The entries USED are those with use[i] != 0
 * (use == NULL: all).  Used values are finite and >= 0 (-0.0 counts as +0.0); the selection key is the bit pattern of v + 0.0, as
 * for me_group_order_stats.  ranks[j] are 0-based, may be unsorted and may repeat, each in [0, count).  A bad value or rank is
 * ME_ERR_ARG, detected on the device and reported after the call (`out` is then unspecified).
 *   count           the used entries
 *   sum             per-block partials (a fixed grid of at most 1024 blocks; a thread adds its entries in order, a block by a fixed
 *                   tree) combined in block order: no floating-point atomics, bit-identical from run to run
 *   min, max        the smallest and the largest used entry
 *   value[j]        sorted_used[ranks[j]]; 0 for j >= n_ranks
 * count, min, max and value[] are EXACT: a most-significant-digit radix select over the keys, eight passes of eight bits, integer
 * histograms only, all ranks at once (ranks that share a prefix share a histogram).  After a pass in which at most 1/8 of the
 * entries read carried a live prefix (and the list had at least 32768 entries), those entries are copied, in order, to a compact list
 * which the later passes read instead.  count == 0 (then n_ranks must be 0): every field 0.  Device timer "rank_select";
 * me_timer_get "rank_select_compactions" / "rank_select_list": compactions done by the context's last select / entries its last
 * pass read.
 *
 * me_sqrt_threshold(t): the largest double x whose correctly rounded sqrt is <= t (-1 unless t >= 0).  Host arithmetic.  "d <= t"
 * is decided everywhere as d2 <= me_sqrt_threshold(t), so that no count depends on how a device rounds sqrt.
 *
 * me_nn_error_distribution: the current 1-NN result of query_slot (me_nn1, me_set_nn_result or the suite; ME_ERR_STATE without
 * one).  Single GPU only (slab or shard mode: ME_ERR_ARG); any parameter out of range is ME_ERR_ARG.  The USED set: every entry with
 * d2 >= 0 that passes the gate (gate / gate_mode as me_nn_stats; gate < 0: every query, CD's population).
 *   n_query, n_used   entries with d2 >= 0; the used ones
 *   sum_d, sum_d2     sums over the used set (sqrt on the device), block-order sums as above
 *   min_d, max_d      host sqrt of the exact smallest / largest used d2; max_d is the one-sided Hausdorff distance
 *   argmax            ORIGINAL index of the used query with the largest d2, ties -> smallest index; -1 when n_used == 0
 *   rank[j]           min(n_used - 1, max(0, (int64) ceil(prob[j] * (double) n_used) - 1)): the nearest-rank definition, one fp64
 *                     multiplication; quantile_d2[j] = the used d2 of that rank (exact, by the select above on nn_d2 in place),
 *                     quantile_d[j] = its host sqrt — sqrt is monotone, so it is that order statistic of the distances.
 *                     n_used == 0: ranks -1, values 0
 *   n_within[k]       used entries with d2 <= me_sqrt_threshold(tau[k])
 *   hist[j]           with E_j = me_sqrt_threshold((double) j * bin_width), j = 1 .. n_bins, and E_0 = -inf: the used entries with
 *                     E_j < d2 <= E_{j+1}, j = 0 .. n_bins - 1; n_overflow those with d2 > E_{n_bins}.  The cumulative sums of hist
 *                     are the empirical CDF of the distances at the edges j * bin_width under the rule "d <= t"
 * The call leaves the slot's 1-NN result untouched.  Device timers "errdist" and "rank_select".
 *
 * me_fscore_finalize: pure host arithmetic, no context (like me_nn_finalize).  prf = {P, R, F}: P = n_within_est / n_est,
 * R = n_within_gt / n_gt (a zero denominator gives 0 for that ratio), F = 2 P R / (P + R) when P + R > 0, else 0. */
#define ME_RANK_MAX 16
#define ME_ERRDIST_MAX_THRESHOLDS 8
#define ME_ERRDIST_MAX_BINS 4096
typedef struct me_rank_stats {
    int64_t count;
    double sum, min, max;
    double value[ME_RANK_MAX];
} me_rank_stats;
typedef struct me_errdist_params {
    double gate;
    int32_t gate_mode; /* as me_nn_stats; gate < 0: every query */
    int32_t n_quantiles;
    double prob[ME_RANK_MAX]; /* each in [0, 1] */
    int32_t n_thresholds;
    double tau[ME_ERRDIST_MAX_THRESHOLDS]; /* each >= 0 */
    int32_t n_bins; /* 0: no histogram */
    double bin_width; /* > 0 when n_bins > 0 */
} me_errdist_params;
typedef struct me_errdist_out {
    int64_t n_query, n_used;
    double sum_d, sum_d2, min_d, max_d;
    int64_t argmax;
    int64_t rank[ME_RANK_MAX];
    double quantile_d[ME_RANK_MAX], quantile_d2[ME_RANK_MAX];
    int64_t n_within[ME_ERRDIST_MAX_THRESHOLDS];
    int64_t n_overflow;
} me_errdist_out;
int me_rank_select(me_ctx *ctx, const double *values, const uint8_t *use, int64_t n, const int64_t *ranks, int32_t n_ranks, me_rank_stats *out);
double me_sqrt_threshold(double t);
int me_nn_error_distribution(me_ctx *ctx, int query_slot, const me_errdist_params *p, me_errdist_out *out, int64_t *hist);
void me_fscore_finalize(int64_t n_within_est, int64_t n_est, int64_t n_within_gt, int64_t n_gt, double prf[3]);

/* ---- Normal-aware map error over the resident 1-NN pairs: point-to-plane distance and normal consistency ------------------------- */
/* (DESIGN.md section 4.14).  The distances of getDiffRegResultWithCorrespondence (map_eval.cpp:1069-1145) and of
 * computeChamferDistance (map_eval.cpp:1398-1431) are nearest-POINT distances: on a surface sampled at spacing s a map point lying
 * on the surface still sits about s / 3 from its nearest sample.  These calls refine that quantity with the reference cloud's
 * normals (me_set_normals, me_estimate_normals or me_radius_normals): the distance to the neighbour's local plane, the tangential
 * remainder, and the agreement of the two normals.  Single GPU only (slab or shard mode: ME_ERR_ARG).
 *
 * me_nn_surface_error: the current 1-NN result of query_slot (ME_ERR_STATE without one); the reference slot must have normals
 * (ME_ERR_STATE), the query's are optional.  gate / gate_mode as me_nn_stats (gate < 0: every query); 0 <= n_thresholds <=
 * ME_ERRDIST_MAX_THRESHOLDS, every tau finite and >= 0; 0 <= n_angles <= ME_SURFACE_MAX_ANGLES, every cos_min in [0, 1]; else
 * ME_ERR_ARG.  Normals are used AS STORED, not re-normalised, and must be finite.
 *   The pair (i, j = nn_idx[i]) is USED iff d2_i >= 0, it passes the gate, j names a reference point (a result placed by
 *   me_set_nn_result has no neighbour indices: none of its pairs is used) and the reference normal n = normals_ref[j] is not the
 *   zero vector.  It is NORMAL-USED iff moreover the query has normals and m = normals_query[i] is not the zero vector.
 *   Per used pair, with d = p_i - g_j component by component (fp64, no FMA):
 *     e  = fabs((nx*dx + ny*dy) + nz*dz)          the point-to-plane distance
 *     t2 = fmax(d2 - e*e, 0)                      the squared tangential remainder
 *     c  = fabs((mx*nx + my*ny) + mz*nz)          (normal-used pairs) the normal consistency
 *   n_query           entries with d2 >= 0;  n_used, n_normal_used: the used / normal-used pairs
 *   sum_e, sum_e2, sum_t2   over the used pairs;  sum_c over the normal-used ones.  Per-block partials (a fixed grid of at most 1024
 *                     blocks; a thread adds its entries in order, a block by a fixed tree) combined in block order: no floating-point
 *                     atomics, bit-identical from run to run
 *   max_e, argmax     the largest e and the ORIGINAL index of its query, ties -> smallest index; 0 and -1 when n_used == 0
 *   n_within[k], sum_e2_within[k]   the used pairs with e <= tau[k] and the sum of their e*e
 *   n_angle[k]        the normal-used pairs with c >= cos_min[k].  The caller passes the COSINE: no count depends on a device cos
 * n_used == 0: every sum and count but n_query is 0.  The call leaves the 1-NN result untouched.  Device timer "surface".
 *
 * me_nn_surface_fetch: e (plane_d) and c (cos_n) of the slot's last me_nn_surface_error in cloud order (N entries each, nullable),
 * -1.0 where the pair was not used (cos_n: not normal-used).  ME_ERR_STATE without a current result: it is discarded with the 1-NN
 * result.  Exact quantiles of e: me_rank_select on plane_d with use = (plane_d >= 0). */
#define ME_SURFACE_MAX_ANGLES 8
typedef struct me_surface_params {
    double gate;
    int32_t gate_mode; /* as me_nn_stats; gate < 0: every query */
    int32_t n_thresholds;
    double tau[ME_ERRDIST_MAX_THRESHOLDS]; /* each finite and >= 0 */
    int32_t n_angles;
    int32_t reserved;
    double cos_min[ME_SURFACE_MAX_ANGLES]; /* each in [0, 1] */
} me_surface_params;
typedef struct me_surface_out {
    int64_t n_query, n_used, n_normal_used;
    double sum_e, sum_e2, sum_t2, sum_c, max_e;
    int64_t argmax;
    int64_t n_within[ME_ERRDIST_MAX_THRESHOLDS];
    double sum_e2_within[ME_ERRDIST_MAX_THRESHOLDS];
    int64_t n_angle[ME_SURFACE_MAX_ANGLES];
} me_surface_out;
int me_nn_surface_error(me_ctx *ctx, int query_slot, const me_surface_params *p, me_surface_out *out);
int me_nn_surface_fetch(me_ctx *ctx, int query_slot, double *plane_d, double *cos_n);

/* ---- M3C2: the signed cloud-to-cloud distance along the query cloud's normals, with a level of detection -------------------------- */
/* (Lague, Brodu, Leroux 2013).  Every 1-NN figure compares one point with one sample and has no sign.  M3C2
 * averages BOTH clouds inside a cylinder around each core point's normal and reports the signed offset of the two averages and
 * whether it can be told from roughness and density.  Single GPU only (slab or shard mode: ME_ERR_ARG).  Device timer "m3c2".
 *
 * me_m3c2.  The core points are the points of query_slot ("own" cloud), thinned by core_mask (host, uint8[N], cloud order, != 0 =
 * core point; NULL = every point); the other slot is the compared cloud ("other").  The query slot's resident normals are used AS
 * STORED (me_set_normals, me_estimate_normals or me_radius_normals; not re-normalised; must be finite).  Parameters:
 * projection_radius rp (half of M3C2's d) and max_depth L (the cylinder's half-length) finite and > 0, min_points >= 2, reg_error
 * finite and >= 0, p and out non-NULL, else ME_ERR_ARG.  ME_ERR_STATE: either slot holds no cloud, or the query slot has no normals.
 *   Membership.  For the core point q with stored normal N = (nx, ny, nz) and a candidate p of either cloud (fp64, no FMA):
 *       dx = px-qx, dy = py-qy, dz = pz-qz
 *       d2 = (dx*dx + dy*dy) + dz*dz
 *       t  = (nx*dx + ny*dy) + nz*dz
 *       inside  <=>  fabs(t) < L  &&  d2 - t*t < rp*rp
 *     Both tests are strict (the library's radius convention).  The core point counts in its own cloud's cylinder (t = 0, as in
 *     M3C2); coincident duplicates count as often as they occur.  A zero normal gives t = 0 for every candidate: the counts are those
 *     of the ball of radius rp, and the point is invalid.
 *   Per cloud c in {own, other}: n_c = the points inside; S_c = sum t, Q_c = sum t*t, added per core point in the order the
 *     candidates are streamed — moments about the core point, so that no term exceeds L^2 —; mean_c = S_c / n_c,
 *     var_c = max((Q_c - S_c*S_c/n_c) / (n_c - 1), 0).
 *   A core point is VALID iff its normal is not the zero vector, n_own >= min_points and n_other >= min_points.  On a valid one
 *       dist        = mean_other - mean_own        (positive: the other cloud lies further along +N)
 *       lod         = 1.96 * (sqrt(var_own/n_own + var_other/n_other) + reg_error)
 *       significant = fabs(dist) > lod
 *     Error bounds against exactly summed moments of the same t: |dist| within (n_own + n_other) 2^-53 L, each var_c within
 *     (3 n_c + 10) 2^-53 L^2 (<= 8 n_c 2^-53 L^2).
 *   An invalid core point stores dist = lod = var_own = var_other = 0 and flags 0 but KEEPS its two counts (they say why it is
 *   invalid); a masked-out point stores zeros throughout and enters no total.
 *   out: n_core (the core points), n_no_normal (core points with a zero normal), n_valid, n_significant; over the VALID points
 *     sum_dist, sum_abs_dist, sum_dist2, sum_lod, sum_n_own, sum_n_other, and max_abs_dist with argmax = the ORIGINAL index of its
 *     core point, ties -> smallest index (0 and -1 when n_valid == 0).  Per-block partials (a fixed grid of at most 1024 blocks; a
 *     thread adds its entries in order, a block by a fixed tree) combined in block order: no floating-point atomics, bit-identical
 *     from run to run on the same index.
 * INDEX AND ORDER OF USE.  Both slots need an index whose cell edge is >= R = sqrt(L*L + rp*rp), the radius of the cylinder's
 * bounding ball; a slot whose cell is smaller than R or larger than 1.5 R is re-indexed at R (me_local_geometry's rule; the cell size
 * asked for at the upload is remembered).  That DISCARDS the resident 1-NN results of both slots (me_nn1 and everything read from
 * it, me_nn_surface_error's result included) and the re-indexed slot's local-geometry result (me_local_geometry_fetch, me_mom).
 * Normals are kept in cloud order and survive.  So: normals first, then me_m3c2, then me_nn1 and what depends on it.
 * COST.  The search visits the ball of radius R, not the cylinder: the work per core point grows like (R / spacing)^2.  Thin the core
 * points with core_mask when L is long or the clouds are dense.
 *
 * me_m3c2_fetch: the per-point arrays of the slot's last me_m3c2 in cloud order (N entries each, all nullable); flags bit 0 = valid,
 * bit 1 = significant.  ME_ERR_STATE without a current result: it is discarded when either slot's points change (upload,
 * down-sample, transform, perturbation, selection) or the query slot is re-indexed. */
typedef struct me_m3c2_params {
    double projection_radius; /* rp, finite and > 0 */
    double max_depth;         /* L, finite and > 0 */
    double reg_error;         /* finite and >= 0 */
    int32_t min_points;       /* >= 2 */
    int32_t reserved;
} me_m3c2_params;
typedef struct me_m3c2_out {
    int64_t n_core, n_no_normal, n_valid, n_significant;
    double sum_dist, sum_abs_dist, sum_dist2, sum_lod;
    int64_t sum_n_own, sum_n_other;
    double max_abs_dist;
    int64_t argmax;
} me_m3c2_out;
int me_m3c2(me_ctx *ctx, int query_slot, const me_m3c2_params *p, const uint8_t *core_mask, me_m3c2_out *out);
int me_m3c2_fetch(me_ctx *ctx, int query_slot, double *dist, double *lod, double *var_own, double *var_other, int32_t *n_own,
                  int32_t *n_other, uint8_t *flags);

/* ---- cloud-to-mesh distance against a ground-truth triangle mesh, and an area-uniform sample of that mesh ---------------------------- */
/*   Stands in for the reference's mesh branch (map_eval.cpp:194-205, 509-523, renderDistanceOnMesh 738-775),
 * which measures against a Poisson mesh of the ground truth, and plays the role of computePointCloudDistance (map_eval.cpp:568-584)
 * with an exact point-to-triangle distance against a mesh the CALLER supplies (CloudCompare's cloud-to-mesh distance); me_mesh_sample
 * is Open3D's TriangleMesh::SamplePointsUniformly with a stated generator.  Single GPU only (slab or shard mode: ME_ERR_ARG).
 *
 * me_mesh_upload: vertices = host fp64 xyz [n_vertices][3], triangles = host int32 [n_triangles][3], T = nullable row-major 4x4 applied
 *   as me_upload_cloud applies it.  The mesh lives in the primary context beside the two clouds (a twin sees it), survives cloud uploads
 *   and re-indexing; a second upload replaces it, me_mesh_clear drops it; both discard the mesh-distance results of both slots.
 *   ME_ERR_ARG: n_triangles < 1, an index outside [0, n_vertices), a non-finite coordinate of a REFERENCED vertex (unreferenced
 *   vertices are ignored).  A triangle is DEGENERATE iff n = (B - A) x (C - A), each component u1*v2 - u2*v1 in fp64 without
 *   contraction, is exactly the zero vector; it is kept and searched as its three segments; its area is 0.
 *   area(t) = 0.5 * sqrt((nx*nx + ny*ny) + nz*nz); the cumulative table is the sequential fp64 sum in the caller's order, formed on the
 *   host (numpy.cumsum reproduces it bit for bit).  Index: an implicit 8-ary tree of axis-aligned fp64 boxes over the triangles sorted
 *   by the Morton code of their centroid (leaves = 8 consecutive triangles); device timer "mesh_index" covers the build's own kernels,
 *   the radix sort between them reports under the library's "sort" timer as in every index build (scopes do not nest).
 * me_mesh_info: counts, bounding box of the referenced vertices, total area, tree depth (levels, leaves included).  ME_ERR_STATE: no mesh.
 *
 * me_mesh_distance: for every point p of query_slot the closest point c of the mesh.  Per triangle ONE fixed sequence of fp64
 *   operations (no FMA), dot(u, v) = (u0*v0 + u1*v1) + u2*v2, clamp01(x) = fmin(fmax(x, 0), 1) (a NaN quotient gives 0):
 *       ab = B-A  ac = C-A   d1 = dot(ab, p-A) d2 = dot(ac, p-A)   d3 = dot(ab, p-B) d4 = dot(ac, p-B)   d5 = dot(ab, p-C) d6 = dot(ac, p-C)
 *       d1 <= 0 && d2 <= 0                               -> vertex A (region 4)
 *       d3 >= 0 && d4 <= d3                              -> vertex B (5)
 *       d1*d4 - d3*d2 <= 0 && d1 >= 0 && d3 <= 0         -> edge AB (1)   c = A + clamp01(d1 / (d1 - d3)) * ab
 *       d6 >= 0 && d5 <= d6                              -> vertex C (6)
 *       d5*d2 - d1*d6 <= 0 && d2 >= 0 && d6 <= 0         -> edge CA (3)   c = A + clamp01(d2 / (d2 - d6)) * ac
 *       d3*d6 - d5*d4 <= 0 && d4-d3 >= 0 && d5-d6 >= 0   -> edge BC (2)   c = B + clamp01((d4-d3) / ((d4-d3) + (d5-d6))) * (C-B)
 *       else                                             -> face (0)      va = d3*d6 - d5*d4, vb = d5*d2 - d1*d6, vc = d1*d4 - d3*d2,
 *                                                           den = (va + vb) + vc, s = clamp01(vb / den), t = fmin(fmax(vc / den, 0), 1 - s),
 *                                                           c = (A + s*ab) + t*ac
 *   the first line that holds decides; d2(p, t) = ((dx*dx + dy*dy) + dz*dz) with d = p - c.  A degenerate triangle: the segments AB, BC,
 *   CA in this order, a later one only when strictly nearer; per segment P0 P1: e = P1-P0, l = dot(e, e), t = dot(e, p-P0); t <= 0 -> P0
 *   (its vertex code), t >= l -> P1, else c = P0 + (t / l) * e (the edge's code).
 *   Per query: the minimal d2; the triangle = the smallest caller index among the bitwise-minimal d2; that triangle's region and c.
 *   The search is unbounded and exact in this arithmetic (the tree only prunes what cannot win or tie).  Device timer "mesh_dist".
 *   SIGN.  Only in the face region: s = dot(p - c, n) / sqrt(dot(n, n)), n = (B-A) x (C-A) by the triangle's winding.  At an edge or a
 *   vertex a single face normal can name the wrong side of a non-convex mesh: signed_d is NaN there and such points enter neither
 *   sum_signed nor sum_abs_signed.  The sign at edges and vertices is me_mesh_signed_distance's (pseudo-normals, below); this call and
 *   its fetch are unchanged by it.
 *   GATE.  A point is MATCHED iff d2 <= max_distance * max_distance (+inf: every point); only matched points enter the totals.
 *   n_within[k] counts the matched points with d2 <= thresholds[k] * thresholds[k].  max_d = the largest matched d = sqrt(d2), argmax its
 *   cloud-order index (ties -> the smaller index; -1 without a matched point).  n_face, sum_signed, sum_abs_signed over the matched points
 *   whose region is the face.  Sums: per-block partials by a fixed tree, combined in block order; identical from run to run.
 *   ME_ERR_STATE: no mesh, or no cloud in the slot.  ME_ERR_ARG: bad slot, max_distance negative or NaN, a negative or non-finite
 *   threshold, n_thresholds outside [0, 8], slab or shard mode.
 * me_mesh_distance_fetch: the per-point arrays in cloud order, every pointer nullable: d2[N], tri[N] (caller's triangle index),
 *   region[N], closest[N][3], signed_d[N] (NaN outside the face region).  ME_ERR_STATE without a current result: it is discarded when the
 *   slot's points change or the slot is re-indexed, and by me_mesh_upload / me_mesh_clear.  It survives me_nn1 and me_mme.
 *
 * me_mesh_sample: n_points area-uniform samples of the mesh become the cloud of dst_slot, as an upload would leave it (the cell size
 *   of the other slot's upload, so that the two grids align).  Sample i: (w0, w1, w2, w3) = Philox4x64-10(counter (i, 0, 0, 0), key
 *   (seed, 0)); u01(w) = (w >> 11) * 2^-53; u = u01(w0) * total_area; the triangle is the first index whose cumulative area exceeds u
 *   (a zero-area triangle is never chosen); r1 = sqrt(u01(w1)), r2 = u01(w2); wa = 1 - r1, wb = r1 * (1 - r2), wc = r1 * r2;
 *   point = (wa*A + wb*B) + wc*C per coordinate.  ME_ERR_ARG: n_points < 1, a total area that is not positive and finite. */
#define ME_MESH_MAX_THRESHOLDS 8
typedef struct me_mesh_params {
    double max_distance; /* >= 0, +inf allowed */
    int64_t n_thresholds;
    double thresholds[ME_MESH_MAX_THRESHOLDS];
} me_mesh_params;
typedef struct me_mesh_out {
    int64_t n_query, n_matched, n_face;
    double sum_d, sum_d2, max_d;
    int64_t argmax;
    int64_t n_within[ME_MESH_MAX_THRESHOLDS];
    double sum_signed, sum_abs_signed;
} me_mesh_out;
typedef struct me_mesh_info_out {
    int64_t n_vertices, n_triangles, n_degenerate, depth;
    double bbox_lo[3], bbox_hi[3];
    double area;
} me_mesh_info_out;
int me_mesh_upload(me_ctx *ctx, const double *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, const double *T);
int me_mesh_clear(me_ctx *ctx);
int me_mesh_info(me_ctx *ctx, me_mesh_info_out *out);
int me_mesh_distance(me_ctx *ctx, int query_slot, const me_mesh_params *p, me_mesh_out *out);
int me_mesh_distance_fetch(me_ctx *ctx, int query_slot, double *d2, int32_t *tri, uint8_t *region, double *closest, double *signed_d);
int me_mesh_sample(me_ctx *ctx, int dst_slot, int64_t n_points, uint64_t seed);

/* ---- signed cloud-to-mesh distance everywhere: mesh connectivity, pseudo-normals at edges and vertices, the sign pass ------------------ */
/*   Baerentzen and Aanaes (2005): for a closed, orientable, manifold mesh the sign of dot(p - c, N) is that of
 * the side p lies on when N is chosen by the feature the closest point c lies on: the face normal in a face, the sum of the two incident
 * face normals on an edge, the angle-weighted sum of the incident face normals at a vertex.  me_mesh_upload (and me_reconstruct_install,
 * which is one) keeps the caller's int32 [n_triangles][3] index array on the device, 12 B per triangle.  VERTEX IDENTITY IS THE
 * CALLER'S INDEX: two indices with equal coordinates are two vertices (weld triangle soup first).  Everything below is formed from the
 * resident corners (after the upload's T) in fp64 without contraction, dot(u, v) = (u0*v0 + u1*v1) + u2*v2.  Single GPU only.
 *
 * me_mesh_topology: built on the device on first use and kept with the mesh; me_mesh_upload, me_mesh_clear and me_reconstruct_install
 *   drop it.  Needs 3 * n_triangles < 2^32 (ME_ERR_ARG otherwise).  ME_ERR_STATE: no mesh.
 *   FACE.  n = (B-A) x (C-A), each component u1*v2 - u2*v1; len = sqrt((nx*nx + ny*ny) + nz*nz); n^ = n / len per component.  A
 *     degenerate triangle (n exactly zero, as the upload flags it) has no n^ and contributes nothing to any sum.
 *   CORNER ANGLES.  ang_A = atan2(len, dot(B-A, C-A)), ang_B = atan2(len, dot(C-B, A-B)), ang_C = atan2(len, dot(A-C, B-C)).
 *   EDGE {lo, hi} (undirected, by vertex index).  N_e = sum of n^ over the incident non-degenerate triangles in ascending caller triangle
 *     index, a left-to-right fp64 sum.  m counts ALL incident triangles, degenerate ones included, except a triangle that names the same
 *     vertex twice: such a triangle has no edges.  Flags: BOUNDARY m == 1; NONMANIFOLD m > 2; INCONSISTENT m == 2 and both triangles
 *     traverse the edge in the same direction; ZERO N_e is exactly the zero vector or no incident triangle is non-degenerate.
 *   VERTEX v.  N_v = sum of ang * n^ (each term ang * n^x, ang * n^y, ang * n^z) over the incident non-degenerate (triangle, corner) pairs
 *     in ascending triangle index, then corner; a left-to-right sum.  Flags: ZERO as for edges; TAINTED any edge of an incident triangle
 *     that ends in v carries BOUNDARY, NONMANIFOLD or INCONSISTENT.  A vertex no triangle names: zero normal, ZERO.
 *   The 3T edge records (key lo, hi) and the 3T corner records (key v) are emitted in triangle order and sorted by the library's stable
 *   radix sort ("sort" timer); one lane walks each run of equal keys serially.  Device timer "mesh_topology" covers the build's kernels.
 *   me_mesh_topo_out: n_edges (unique), the edges per flag, n_zero_vertices (every vertex that carries ZERO, unreferenced ones included),
 *   n_tainted_vertices, n_unreferenced_vertices, closed (no boundary edge), oriented_manifold (none of the three edge flags anywhere).
 * me_mesh_topology_fetch: every pointer nullable.  vertex_normal [n_vertices][3], vertex_flags [n_vertices], edge_normal
 *   [n_triangles][3][3] and edge_flags [n_triangles][3] per (triangle, local edge AB BC CA); a triangle without edges: zeros and ZERO.
 *
 * me_mesh_signed_distance: needs the slot's current me_mesh_distance result (ME_ERR_STATE otherwise, and without a mesh); builds the
 *   topology if it is absent.  Per point, from the resident (d2, triangle, region, c): N = n (NOT normalised) of the winning triangle
 *   for region 0, N_e of that triangle's edge for regions 1-3, N_v of that corner for regions 4-6; g = dot(p - c, N), p - c per component.
 *       d2 == 0                        -> signed_d = +0.0, flag ON
 *       the winning triangle is degenerate, or the feature carries ZERO -> NaN, flag UNSIGNED
 *       g > 0 -> +sqrt(d2)    g < 0 -> -sqrt(d2)    else (g == 0 or NaN) -> NaN, flag UNSIGNED
 *   UNRELIABLE: the feature carries BOUNDARY, NONMANIFOLD, INCONSISTENT or TAINTED (the theorem's preconditions fail there).  The
 *   magnitude is the same sqrt(d2) in every region; across a shared edge N is the same vector whichever tied triangle won.
 *   signed_d > 0 outside, as in me_mesh_distance.  Per-point values exist for every point; the TOTALS are over the MATCHED points,
 *   d2 <= max_distance * max_distance (+inf: every point): n_signed = n_inside (signed_d < 0) + n_outside (> 0) + n_on; n_unsigned;
 *   n_unreliable; n_by_region face / edge / vertex; sum_signed, sum_abs_signed, sum_signed2 = sum of signed_d * signed_d, over the signed
 *   points; min_signed / argmin (the deepest inside point) and max_signed / argmax over the signed points, ties -> the smaller cloud
 *   index, -1 (and 0.0) without one.  Sums as in me_mesh_distance: fixed tree, identical from run to run.  Device timer "mesh_sign".
 *   ME_ERR_ARG: bad slot, NULL, max_distance negative or NaN, slab or shard mode.
 * me_mesh_signed_fetch: signed_d[N] and flags[N] in cloud order, both nullable.  The result is discarded with the mesh-distance result
 *   (a changed cloud, a new index, me_mesh_upload, me_mesh_clear, me_reconstruct_install) and by a new me_mesh_distance on the slot. */
#define ME_MESH_TOPO_BOUNDARY 1
#define ME_MESH_TOPO_NONMANIFOLD 2
#define ME_MESH_TOPO_INCONSISTENT 4
#define ME_MESH_TOPO_ZERO 8
#define ME_MESH_TOPO_TAINTED 16
#define ME_MESH_SIGN_ON 1
#define ME_MESH_SIGN_UNSIGNED 2
#define ME_MESH_SIGN_UNRELIABLE 4
typedef struct me_mesh_topo_out {
    int64_t n_edges, n_boundary_edges, n_nonmanifold_edges, n_inconsistent_edges, n_zero_edges;
    int64_t n_zero_vertices, n_tainted_vertices, n_unreferenced_vertices;
    int64_t closed, oriented_manifold;
} me_mesh_topo_out;
typedef struct me_mesh_sign_params {
    double max_distance; /* >= 0, +inf allowed */
} me_mesh_sign_params;
typedef struct me_mesh_sign_out {
    int64_t n_query, n_matched, n_signed, n_inside, n_outside, n_on, n_unsigned, n_unreliable;
    int64_t n_by_region[3];
    double sum_signed, sum_abs_signed, sum_signed2;
    double min_signed;
    int64_t argmin;
    double max_signed;
    int64_t argmax;
} me_mesh_sign_out;
int me_mesh_topology(me_ctx *ctx, me_mesh_topo_out *out);
int me_mesh_topology_fetch(me_ctx *ctx, double *vertex_normal, uint8_t *vertex_flags, double *edge_normal, uint8_t *edge_flags);
int me_mesh_signed_distance(me_ctx *ctx, int query_slot, const me_mesh_sign_params *p, me_mesh_sign_out *out);
int me_mesh_signed_fetch(me_ctx *ctx, int query_slot, double *signed_d, uint8_t *flags);

/* ---- rays against the resident mesh: closest hit, any hit, a simulated range sensor, observability of a cloud's points --------------- */
/* (DESIGN.md section 4.25.  No reference counterpart: the reference has no ray.)  All against the resident mesh of the primary context
 * (a twin sees it); ME_ERR_STATE without one.  fp64, single GPU only (slab or shard mode: ME_ERR_ARG).
 *
 * The ray-triangle routine is the watertight test of Woop, Benthin and Wald (2013) as ONE fixed sequence of fp64 operations, none
 * contracted.  Per ray (o, d), INVALID (hits nothing) unless every component of o and d is finite and d is not the zero vector:
 *   kz = argmax |d[k]| (ties: lowest k); kx = (kz+1)%3; ky = (kz+2)%3; if d[kz] < 0: swap(kx, ky)
 *   Sx = d[kx]/d[kz]   Sy = d[ky]/d[kz]   Sz = 1/d[kz]   dd = (d0*d0 + d1*d1) + d2*d2
 * Per triangle (A, B, C) in the caller's winding; a triangle flagged degenerate at upload never hits:
 *   grazing gate: u = B - A, v = C - A, n = (u1*v2 - u2*v1, u2*v0 - u0*v2, u0*v1 - u1*v0), c = (n0*d0 + n1*d1) + n2*d2,
 *     nn = (n0*n0 + n1*n1) + n2*n2; a miss if c*c < 0x1p-40 * (nn * dd)        (an incidence within ~1e-6 rad of the plane)
 *   A' = A - o per component (likewise B', C');  Ax = A'[kx] - Sx*A'[kz]   Ay = A'[ky] - Sy*A'[kz]   (same for B, C)
 *   U = Cx*By - Cy*Bx   V = Ax*Cy - Ay*Cx   W = Bx*Ay - By*Ax
 *   a miss if (U < 0 || V < 0 || W < 0) && (U > 0 || V > 0 || W > 0);  det = (U + V) + W;  a miss if det == 0
 *   T = (U*(Sz*A'[kz]) + V*(Sz*B'[kz])) + W*(Sz*C'[kz]);  t = T / det;  a hit iff t_min <= t && t <= t_max
 *   u = V / det (weight of B), v = W / det (weight of C), BACKFACE iff det < 0.  The point is o + t d: t is in units of |d|.
 * The edge functions are exactly antisymmetric (Qx*Py - Qy*Px of edge P->Q is the exact negative of the neighbour's): a ray across
 * the shared edge of two consistently wound triangles hits at least one of them, unless the grazing gate drops it.
 * Closest hit: the lexicographic minimum of (t, caller's triangle index) over the hits.  Any hit: whether a hit exists.  Neither depends
 * on the order of the walk: the tree culls a box only when no triangle inside it can be a computed hit in the interval.
 * (Stated limit of that cull, DESIGN.md 4.25 "Pruning": a triangle whose smallest altitude is below 2^-29 of its lateral distance from the
 * ray may be a hit of an exhaustive loop over the routine, far off the ray, and be culled.)
 *
 * me_mesh_raycast: origins / dirs = host fp64 [n_rays][3], 0 <= t_min (finite) <= t_max (+inf allowed), mode ME_RAY_CLOSEST or
 *   ME_RAY_ANY.  Every per-ray output is nullable, caller's order: t (+inf on a miss), tri (caller's index, -1 on a miss), u, v, flags
 *   (ME_RAY_HIT, ME_RAY_BACKFACE, ME_RAY_INVALID).  ME_RAY_ANY reports ME_RAY_HIT / ME_RAY_INVALID only: t = +inf, tri = -1, u = v = 0
 *   (the triangle the walk met first is not a result).  Totals: n_rays, n_hit, n_backface, n_invalid, min_t / max_t over the hits
 *   (+inf / -inf without a hit and in mode ME_RAY_ANY).  Device timers "ray_cast" (closest) and "ray_occl" (any).
 *   ME_ERR_ARG: a NULL input, n_rays outside [1, 2^31), t_min negative or not finite, t_max < t_min or NaN, an unknown mode.
 *
 * me_mesh_scan: the simulated sensor; no trigonometry in the library.  poses = host [n_poses][16] row-major 4x4 sensor -> world, dirs =
 *   host [n_dirs][3] beams in the sensor frame; n_poses * n_dirs < 2^31.  Ray r = p * n_dirs + b: o = (P[3], P[7], P[11]),
 *   d_w[k] = (P[4k]*dx + P[4k+1]*dy) + P[4k+2]*dz, len = sqrt((d_w0*d_w0 + d_w1*d_w1) + d_w2*d_w2), the closest hit with t in
 *   [min_range / len, max_range / len].  With noise_std > 0 the hit parameter becomes t + (noise_std * z) / len, z =
 *   sqrt(-2 ln u1) cos(2 pi u2) of Philox4x64-10 at counter (r, 6, 0, 0), key (seed, 0), u1 = ((w0 >> 11) + 1) 2^-53, u2 =
 *   (w1 >> 11) 2^-53 (counter word 1 = 6 names this user; 0 me_mesh_sample, 1-3 me_perturb_cloud, 4 me_global_register,
 *   5 me_segment_planes); the range gate is on the hit, not on the noised value.  Point x[k] = o[k] + t * d_w[k].  The hits become the
 *   cloud of dst_slot IN RAY ORDER (a prefix sum of the hit flags; no atomic decides an order), as me_mesh_sample leaves a slot (the
 *   other slot's cell size).  No hit at all: dst_slot is left holding an empty cloud (me_cloud_size 0).  pose_hits = nullable
 *   int64[n_poses].  Device timer "scan".  ME_ERR_ARG: a NULL input, bad counts, min_range negative or not finite, max_range <
 *   min_range, noise_std negative or not finite.
 * me_mesh_scan_fetch: ray_id int64[N] of every point of the slot, cloud order (pose = ray / n_dirs).  ME_ERR_STATE once the slot's
 *   points are no longer that scan's.
 *
 * me_cloud_visibility: origins = host [n_origins][3], n_origins <= ME_VIS_MAX_ORIGINS.  Point p, origin o_j: d = p - o_j per
 *   component, len = sqrt((d0*d0 + d1*d1) + d2*d2).  p is IN RANGE of j iff min_range <= len <= max_range, and SEEN from j iff in range
 *   and (len <= tolerance, or no any-hit of the ray (o_j, d) with t in [0, (len - tolerance) / len]); a non-finite p or o_j sees nothing.
 *   Per point: n_seen (origins that see it) and first_seen (the smallest such j, -1: none); first_only = 1 stops at the first origin
 *   that sees the point (n_seen is 0 or 1, first_seen the same).  Totals: n_points, n_visible (n_seen > 0), n_in_range (of some
 *   origin), n_tests (segments cast; an integer sum).  The call writes the slot's keep mask (kept = visible) exactly as me_plane_keep
 *   does: me_outlier_select_into then copies the observable points anywhere.  Device timer "ray_occl".
 *   ME_ERR_STATE: no mesh, or no cloud in the slot.  ME_ERR_ARG: bad slot, n_origins outside [1, 65536], min_range negative or not
 *   finite, max_range < min_range, tolerance negative or not finite, first_only not 0 or 1.
 * me_cloud_visibility_fetch: n_seen[N], first_seen[N] in cloud order, both nullable.  The result is discarded when the slot's points
 *   change or the slot is re-indexed, and by me_mesh_upload / me_mesh_clear / me_reconstruct_install. */
#define ME_RAY_CLOSEST 0
#define ME_RAY_ANY 1
#define ME_RAY_HIT 1
#define ME_RAY_BACKFACE 2
#define ME_RAY_INVALID 4
#define ME_VIS_MAX_ORIGINS 65536
typedef struct me_ray_out {
    int64_t n_rays, n_hit, n_backface, n_invalid;
    double min_t, max_t;
} me_ray_out;
typedef struct me_scan_params {
    double min_range, max_range; /* metres along the beam; max_range = +inf: unbounded */
    double noise_std;            /* metres; 0 = off */
    uint64_t seed;               /* Philox key word 0 */
} me_scan_params;
typedef struct me_scan_out {
    int64_t n_rays, n_hit, n_backface;
} me_scan_out;
typedef struct me_vis_params {
    double min_range, max_range, tolerance; /* metres */
    int64_t first_only;
} me_vis_params;
typedef struct me_vis_out {
    int64_t n_points, n_visible, n_in_range, n_tests;
} me_vis_out;
int me_mesh_raycast(me_ctx *ctx, const double *origins, const double *dirs, int64_t n_rays, double t_min, double t_max, int mode, double *t,
                    int32_t *tri, double *u, double *v, uint8_t *flags, me_ray_out *out);
int me_mesh_scan(me_ctx *ctx, int dst_slot, const double *poses, int64_t n_poses, const double *dirs, int64_t n_dirs,
                 const me_scan_params *p, int64_t *pose_hits, me_scan_out *out);
int me_mesh_scan_fetch(me_ctx *ctx, int slot, int64_t *ray_id);
int me_cloud_visibility(me_ctx *ctx, int slot, const double *origins, int64_t n_origins, const me_vis_params *p, me_vis_out *out);
int me_cloud_visibility_fetch(me_ctx *ctx, int slot, int32_t *n_seen, int32_t *first_seen);

/* ---- surface reconstruction of a resident cloud into a triangle mesh ------------------------------------------------------------------ */
/*   Stands in for the reference's createMeshFromPCD (map_eval.cpp:777-826, called at :194-205), a Poisson
 * solve, with a LOCAL, deterministic reconstruction whose every number has a stated definition: an implicit-moving-least-squares
 * (IMLS) signed-distance field on a sparse voxel lattice, from the points of a slot and their resident normals, and its zero set by
 * marching tetrahedra.  tests/_recon_ref.py restates everything below.  All arithmetic is fp64 without contraction.  The result is
 * held on the primary context (a twin sees it), like the resident mesh, until the next call of either producer or until the mesh
 * clear call.  All five entry points are single GPU only (slab or shard mode: ME_ERR_ARG).
 * Consistent orientation of the normals is the CALLER's job: normals point outward.  The tools are a viewpoint for the radius normals
 * (enough for a star-shaped scene), the set-normals call, and the orientation call of the next section, which propagates one sign
 * across the k-NN graph of the cloud.  Hole filling, smoothing, the reference's density trimming and multi-GPU slabs are out of scope.
 *
 * PARAMETERS.  voxel h > 0, finite; radius R finite, R >= h; min_k >= 1; band in {0, 1, 2}.
 * LATTICE.  The cell of a point is floor(p / h) per axis (a division, getVoxelIndex's).  Node (i, j, k) sits at x = (double(i)*h,
 *   double(j)*h, double(k)*h).  OCCUPIED cells: the cells of the slot's points.  ACTIVE cells: the occupied cells and every cell within
 *   Chebyshev distance `band` of one.  NODES: the distinct corners of the active cells.  The active cells must span at most 2^21 - 1
 *   cells per axis (the 21-bit Morton frame) and |floor(p / h)| < 2^30, else ME_ERR_ARG.
 * FIELD at a node.  The slot's points p with d = x - p and d2 = (dx*dx + dy*dy) + dz*dz < R*R (strict; R*R formed once), skipping every
 *   point whose stored normal n is the zero vector or has a non-finite component (it contributes nothing and is not counted):
 *       q = 1 - d2 / (R*R)     w = (q*q) * (q*q)     s = (nx*dx + ny*dy) + nz*dz
 *   k = the count, W = sum w, S = sum w*s.  The node is VALID iff k >= min_k and W > 0, and then f = S / W (f = 0 otherwise).  The order
 *   of the two sums is the neighbourhood stream's and not part of the definition: with |n| <= 1, f is within (2k + 4) 2^-53 R of the
 *   exactly rounded sums' quotient; k and validity are exact.  A node is INSIDE iff f < 0 (0 and -0.0 are outside).
 * EXTRACTION.  A cell is extracted iff it is active and all 8 corners are valid.  It is cut into the 6 Kuhn tetrahedra around the
 *   diagonal (0,0,0)-(1,1,1): for each permutation (a, b, c) of the axes, in lexicographic order, v0 = corner 0, v1 = v0 + e_a,
 *   v2 = v1 + e_b, v3 = v2 + e_c (translation invariant; matches across cell faces).  Its edges are the 7 directions out of a node,
 *   dir 0 .. 6 = 100 010 001 110 101 011 111 (dx dy dz).  A VERTEX exists on the edge from origin node a to b = a + dir iff both ends
 *   are valid, exactly one is inside and at least one extracted cell contains the edge; per coordinate, from the ORIGIN whichever end
 *   is inside:   t = clamp01(fa / (fa - fb)) (t < 0 -> 0, t > 1 -> 1)     v = xa + t * (xb - xa)
 *   Triangles of a tetrahedron, tetrahedron-local corner indices ascending, E(x, y) = the vertex on the edge between corners x and y:
 *       one inside corner p, others q1 q2 q3:      (E(p,q1), E(p,q2), E(p,q3)); kept iff det[q1-p, q2-p, q3-p] > 0
 *       three inside, p the outside corner:        the same triangle from p;    kept iff det[q1-p, q2-p, q3-p] < 0
 *       two inside p q, two outside r s:           the quad E(p,r) E(p,s) E(q,s) E(q,r) as (0,1,2) (0,2,3); kept iff det[r-p, s-p, q-p] > 0
 *   "not kept" swaps the last two corners of each triangle.  The determinants are of integer lattice vectors, never of positions:
 *   (B-A) x (C-A) points from inside to outside, the sign convention of the mesh distance (signed_d > 0 outside).  A triangle whose
 *   corners coincide (t was 0 or 1) is kept; n_degenerate counts the triangles the mesh upload would call degenerate.
 * OUTPUT.  vertices double[V][3], vertex_edge int32[V][4] = (i, j, k, dir), triangles int32[T][3].  The order is the implementation's
 *   (vertices ascending by (Morton code of the origin node in the lattice frame, dir), triangles cell by cell in that Morton order,
 *   tetrahedron by tetrahedron) and a pure function of the input: two calls return identical bytes.  V or T >= 2^31: ME_ERR_ARG.
 *
 * me_reconstruct: field and extraction for the cloud of `slot`.  The slot's index is brought to a cell edge >= R by the M3C2 rule
 *   (kept if R (1 + 2^-20) <= cell <= 1.5 R (1 + 2^-20), else rebuilt at R): a rebuild re-sorts the slot and discards the 1-NN results
 *   of both slots and the slot's own MME, local-geometry (me_mom with it), M3C2 and mesh-distance results; points and normals stay, and so
 *   does the OTHER slot's M3C2 result, which is held in that slot's order about unchanged points (me_m3c2_fetch).
 *   ME_ERR_STATE: no cloud, or no normals on the slot.  ME_ERR_ARG: bad parameters.  A cloud that yields no extracted cell is not an
 *   error: zeros.  Device timers "recon_field" and "recon_extract"; the sorts of the lattice build report under "sort".
 * me_isosurface: the same extraction stage on a lattice field the caller supplies: node_ijk int32[n_nodes][3], f[n_nodes],
 *   valid uint8[n_nodes] (host).  A cell is extracted iff all 8 corners are present and valid.  ME_ERR_ARG: a duplicate node, a
 *   non-finite f on a valid node, nodes spanning more than 2^21 - 1 on an axis.  n_nodes = 0 or 1: an empty result.
 * me_reconstruct_fetch: the mesh; every pointer nullable.  ME_ERR_STATE without a reconstruction.
 * me_reconstruct_nodes_fetch: node_ijk int32[n_nodes][3] (Morton order of the lattice frame), f, k int32, valid uint8; every pointer
 *   nullable.  ME_ERR_STATE without one, and after me_isosurface (which keeps no node field).
 * me_reconstruct_install: the reconstruction becomes the resident mesh, exactly as me_mesh_upload of the fetched arrays (T = NULL).
 *   ME_ERR_STATE when there are no triangles. */
typedef struct me_recon_params {
    double voxel, radius;
    int32_t min_k, band;
} me_recon_params;
typedef struct me_recon_out {
    int64_t n_occupied_cells, n_active_cells, n_nodes, n_valid_nodes, n_cells_extracted, n_vertices, n_triangles, n_degenerate, sum_k;
} me_recon_out;
int me_reconstruct(me_ctx *ctx, int slot, const me_recon_params *p, me_recon_out *out);
int me_isosurface(me_ctx *ctx, const int32_t *node_ijk, const double *f, const uint8_t *valid, int64_t n_nodes, double voxel, me_recon_out *out);
int me_reconstruct_fetch(me_ctx *ctx, double *vertices, int32_t *vertex_edge, int32_t *triangles);
int me_reconstruct_nodes_fetch(me_ctx *ctx, int32_t *node_ijk, double *f, int32_t *k, uint8_t *valid);
int me_reconstruct_install(me_ctx *ctx);

/* ---- consistent normal orientation: one sign propagated over the k-NN graph of a resident cloud ---------------------------------------- */
/*   The construction of Hoppe et al. 1992, "Surface reconstruction from unorganized points", which Open3D
 * exposes as PointCloud::OrientNormalsConsistentTangentPlane(k, lambda, cos_alpha_tol): a minimum spanning tree of a neighbour graph
 * weighted by 1 - |n_i . n_j|, and the sign carried along the tree from a root.  The reconstruction, the signed mesh distance and M3C2
 * all consume the sign of the resident normals; a single viewpoint cannot give it on a scene that is not star-shaped.
 * DEVIATIONS from Open3D.  (a) The graph is the k-NN graph alone: Open3D adds the edges of a Delaunay triangulation / Euclidean minimum
 *   spanning tree so that its graph is connected.  Here every connected component of the k-NN graph is oriented on its own, from a root of
 *   its own, and n_components says how many there were.  (b) No lambda (edge penalty along the normal) and no cos_alpha_tol.  (c) Equal
 *   weights do not exist: the edges are in the strict total order of item 3, so the forest, and with it every output, is unique.
 *   (d) The root is the extreme point along a caller-given direction and is turned towards (or, inward, against) that direction; Open3D
 *   takes the point of largest z and turns it towards +z, which direction = (0, 0, 1), inward = 0 reproduces up to ties.
 * tests/_orient_ref.py restates everything below.  All arithmetic is fp64 without contraction.  N = the slot's points, in cloud order.
 *
 * 1. VALID POINTS.  A point is valid iff its resident normal is not (0, 0, 0) (each component compared with 0: -0.0 is 0).  An invalid
 *    point takes no part: it has no edges, keeps its normal, and gets component = -1, flipped = 0.
 * 2. GRAPH.  For every valid point i take the (k+1)-list of i in its own cloud, exactly the row of the k-NN search call with
 *    query_slot = ref_slot = slot and k + 1: ascending by (d2, original index), padded with -1.  The edges of i are the entries j of
 *    that list with j != i, j >= 0 and j valid.  An invalid neighbour is skipped and NOT replaced by the next nearest; where more than
 *    k + 1 points coincide, i may be missing from its own list and then has k + 1 edges.  The graph is undirected: the edge {i, j} exists
 *    if either end lists the other, and counts once in n_graph_edges.
 * 3. EDGE VALUE AND ORDER.  c_ij = (nx*mx + ny*my) + nz*mz on the normals n of i and m of j as resident; bitwise symmetric.  With
 *    lo < hi the original indices of its ends, edge a PRECEDES edge b iff |c_a| > |c_b|, or the two are equal and (lo, hi)_a is
 *    lexicographically smaller.  |c| is compared through its bit pattern as an unsigned integer, which for every non-NaN value is the
 *    numerical order (a NaN, from a non-finite normal, sorts before every number).  A strict total order.
 * 4. FOREST.  The minimum spanning forest of the graph under that order (the first edge is the cheapest): unique.
 *    n_tree_edges = n_valid - n_components.  Components are numbered 0 ... by ascending lowest original index of their members;
 *    largest_component is the largest member count.
 * 5. ROOT.  Per component the member that maximises (px*dx + py*dy) + pz*dz, d = direction as given (not normalised; -0.0 and +0.0
 *    are equal), among equal values the lowest original index.  The root is flipped iff ((nx*dx + ny*dy) + nz*dz < 0) != (inward != 0):
 *    with inward = 0 a product of exactly 0 (or NaN) leaves the root as it is, with inward set it counts as flipped.
 * 6. PROPAGATION.  Every other member is flipped iff flip(root) XOR (the number of tree edges with c < 0 on its path from the root is
 *    odd).  c == 0 (and -0.0) does not flip.  A flipped normal is negated exactly, component by component.  n_flipped counts them.
 * 7. n_inconsistent_edges = the graph edges, tree or not, with (c_ij < 0) XOR flipped_i XOR flipped_j: the edges that still join
 *    opposed normals afterwards.  0 on a smooth, well-sampled surface; a positive count says that k was too small for the sampling,
 *    that two sheets lie closer than the sample spacing, or that the normals are noisy.
 * STATE.  The normals are replaced in place, in cloud order, as the set-normals call would: covariances and FPFH features on the slot
 *   are dropped.  Everything else resident on both slots stays and stays fetchable (positions, index, 1-NN results, MME, local
 *   geometry, M3C2, labels, the resident mesh); the slot is not re-indexed, except in the one case the k-NN search documents below.
 *   component and flipped stay fetchable until the slot's normals or points are next replaced (an upload, a device-side producer, a
 *   transform, any of the normal estimators, the set-normals call).  Single GPU only.
 * ERRORS.  ME_ERR_ARG: bad slot; k outside [1, 39]; a non-finite or all-zero direction; p or out NULL; slab or shard mode.
 *   ME_ERR_STATE: no cloud on the slot, or no normals on it; the fetch without a current result.  ME_ERR_HIP: an allocation failed.
 * DETERMINISM.  Integer atomics (max, min, add) only; no result depends on the order in which they arrive: two calls, and two
 *   contexts, return identical bytes.  A second call on an oriented cloud with the same parameters reports n_flipped = 0.
 * MEMORY for the time of the call: 20 (k + 1) + 38 bytes per point (lists 4 (k + 1), edges 16 (k + 1)), released on return; 5 bytes per
 *   point stay for the fetch.  Device timers "orient_normals" (the whole call), "orient_walk" (the lists) and "orient_forest" (the rest);
 *   the timer-get call under the name "orient_rounds" returns the Boruvka rounds of the last call in *launches.
 *
 * me_orient_normals: the above for the cloud of `slot`.
 * me_orient_fetch: component int32[N], flipped uint8[N] (host, cloud order); either pointer nullable. */
typedef struct me_orient_params {
    double direction[3];
    int32_t k, inward;
} me_orient_params;
typedef struct me_orient_out {
    int64_t n, n_valid, n_components, largest_component, n_tree_edges, n_graph_edges, n_flipped, n_inconsistent_edges;
} me_orient_out;
int me_orient_normals(me_ctx *ctx, int slot, const me_orient_params *p, me_orient_out *out);
int me_orient_fetch(me_ctx *ctx, int slot, int32_t *component, uint8_t *flipped);

/* ---- neighbour lists between the resident clouds: KDTreeFlann::SearchKNN / SearchHybrid / SearchRadius for every point of a
 * cloud (the reference's loops over them: map_eval.cpp:1213-1218, 1448-1454, 1670) ---- */
/* The three searches below hand the neighbours themselves to the caller, for every point of query_slot among the points of
 * ref_slot.  Common to all three:
 *   SLOTS.  query_slot and ref_slot are each 0 or 1 and may be equal: a search of a cloud in itself, in which a query point is its
 *     own first neighbour with d2 = 0 (as in Open3D).  Single-GPU plain clouds only (no slab, no shard); both slots uploaded.
 *   DISTANCE.  d2 = (dx*dx + dy*dy) + dz*dz in fp64 without contraction: the expression of me_nn1 and of the CPU path, bit-identical.
 *   ORDER.  Every list is ascending by (d2, index of the reference point): equal distances resolve to the smaller index, between
 *     coincident and between equidistant points alike.  Results are identical from run to run.
 *   RADIUS.  Membership is strict, d2 < radius * radius, the product formed once on the host in fp64 (me_mme's convention).
 *   INDICES are original (upload-order) indices of the reference cloud, int32; row offsets and totals are int64.
 *   query_mask (nullable): uint8[N_query] in cloud order, non-zero = search this point.  A masked-out query gets an empty row
 *     (radius) or a row of padding and a count of 0 (k-NN, hybrid) and costs no search work.
 *   STATE.  The searches walk the reference cloud's octree, which every index carries at any cell size: no slot is re-indexed for k
 *     or for a radius, and everything resident on both slots (1-NN results, normals, covariances, MME, local geometry, M3C2, voxel
 *     tables, labels) stays as it is and stays fetchable.  The one exception is a slot whose points were replaced on the device and
 *     that has no index at the time of the call: it is indexed at the cell size asked for at its upload, exactly as the next
 *     me_nn1 would, with what that rebuild discards (the 1-NN results of both slots, that slot's MME, local-geometry and M3C2 results).
 *   ERRORS.  ME_ERR_ARG: bad slot, k / max_nn outside [1, 40], radius not finite or not > 0, idx without d2 or the reverse, slab or
 *     shard mode; ME_ERR_STATE: a slot that holds no cloud — never uploaded, or offered an empty cloud, which me_upload_cloud itself
 *     rejects with ME_ERR_ARG, so that no slot can hold zero points (the searches check the count all the same); ME_ERR_HIP: a
 *     device allocation failed (the lists take 12 bytes per entry on the device for the time of the call and are released on return).
 *
 * me_knn_search — SearchKNN(q, k): idx / d2 are N_query x k (host), padded with -1 / +inf where the reference cloud has fewer than
 *   k points.  1 <= k <= 40.
 * me_hybrid_search — SearchHybrid(q, radius, max_nn): the max_nn nearest among those with d2 < radius^2.  idx / d2 are N_query x
 *   max_nn, padded as above; counts[N_query] = entries used per row (nullable).  1 <= max_nn <= 40.
 * me_radius_search — SearchRadius(q, radius) as CSR: offsets[N_query + 1] (host, nullable), *total = offsets[N_query] (nullable).
 *   With idx == d2 == NULL only the counts are computed (the sizing call).  Otherwise capacity >= total is required — ME_ERR_ARG
 *   whose message names the needed total if not, and then NOTHING is written, *total and offsets included — and idx / d2 [total]
 *   receive the rows.  Rows of up to me_search_sort_tile() entries are sorted by one wavefront in LDS, longer ones by one workgroup
 *   in global memory: same order, more time per entry.  Memory: 12 bytes per entry plus 12 per query on the device. */
int me_knn_search(me_ctx *ctx, int query_slot, int ref_slot, int k, const uint8_t *query_mask, int32_t *idx, double *d2);
int me_hybrid_search(me_ctx *ctx, int query_slot, int ref_slot, double radius, int max_nn, const uint8_t *query_mask, int32_t *counts,
                     int32_t *idx, double *d2);
int me_radius_search(me_ctx *ctx, int query_slot, int ref_slot, double radius, const uint8_t *query_mask, int64_t *offsets, int32_t *idx,
                     double *d2, int64_t capacity, int64_t *total);
int me_search_sort_tile(void);

int64_t me_cloud_size(me_ctx *ctx, int slot);
/* transformed points back to the host (N x 3), original order — what map_3d_->points_ holds after :1206 */
int me_download_cloud(me_ctx *ctx, int slot, double *xyz_host);

/* ---- 1-NN: KDTreeFlann::SearchKNN(q, 1, idx, d2) over a whole cloud (map_eval.cpp:1218,1231,1415,1424,579) --- */
/* Searches every point of query_slot in ref_slot; results stay on the device for the me_nn_* calls below.
 * idx / d2 (query-cloud order, length N_query; nullable) receive the neighbour index in ref cloud order and the
 * SQUARED distance ((dx*dx + dy*dy) + dz*dz), bit-identical to the CPU path.  Ties -> smallest ref index, between coincident
 * and between equidistant reference points alike.  ME_ERR_ARG "octree deeper than the level table": see me_upload_cloud. */
int me_nn1(me_ctx *ctx, int query_slot, int ref_slot, int32_t *idx, double *d2);

/* getDiffRegResultWithCorrespondence / getDiffRegResult (map_eval.cpp:1069-1145, 828-897, 990-1067) on the
 * correspondences of the last me_nn1(query_slot, ...): gate (negative = none) + 5 thresholds.  One-shot,
 * single GPU. */
int me_nn_stats(me_ctx *ctx, int query_slot, double gate, int gate_mode, const double trunc[5],
                me_nn_stats_out *out);
/* The same, split for multi-GPU: raw partial sums -> (all-reduce) -> second pass for sigma -> finalize. */
int me_nn_partial_sums(me_ctx *ctx, int query_slot, double gate, int gate_mode, const double trunc[5],
                       me_nn_partial *out);
int me_nn_sigma_sums(me_ctx *ctx, int query_slot, double gate, int gate_mode, const double mean[5],
                     double sigma_num[5]);
void me_nn_finalize(const me_nn_partial *total, const double sigma_num[5], int64_t n_src_total,
                    me_nn_stats_out *out);

/* One point-to-point ICP correspondence + reduction step: what an iteration of Open3D's
 * RegistrationICP(.., TransformationEstimationPointToPoint) (called at map_eval.cpp:1369-1371) needs from the clouds.
 * Over the correspondences of the last me_nn1(query_slot, ref) with d2 < max_distance^2 (Open3D SearchHybrid semantics):
 * the count, sum p, sum q, sum p q^T (row-major, p = source, q = target; all RELATIVE TO `origin`) and sum d2
 * (fitness = n_corr / n_source, inlier_rmse = sqrt(sum_d2 / n_corr)).  The 3x3 Umeyama / Kabsch solve stays on the host;
 * me_transform_cloud applies the update. */
typedef struct me_icp_sums {
    int64_t n_corr;
    int64_t n_source;
    double origin[3];
    double sum_p[3];
    double sum_q[3];
    double sum_pq[9];
    double sum_d2;
} me_icp_sums;
int me_icp_p2p_sums(me_ctx *ctx, int query_slot, double max_distance, me_icp_sums *out);

/* registration_methods 1 (point-to-plane) and 2 (generalized ICP, the shipped config's default; map_eval.cpp:1373-1384):
 * Open3D RegistrationICP(.., TransformationEstimationPointToPlane) / RegistrationGeneralizedICP [upstream].  Per-point
 * attributes live on the device in the caller's point order and follow the cloud through me_transform_cloud
 * (n <- R n, C <- R C R^T, as PointCloud::Transform) and me_voxel_downsample (normals averaged per voxel).
 *   me_set_normals       normals that came with the cloud (PCD normal_x/y/z), N x 3.
 *   me_get_normals       the current normals, N x 3.
 *   me_estimate_normals  PointCloud::EstimateNormals(KDTreeSearchParamKNN(knn)) of a cloud WITHOUT normals: exact k-NN of
 *                        every point (itself included), utility::ComputeCovariance, FastEigen3x3; (0,0,1) where
 *                        undefined.  1 <= knn <= 40.  Optional outputs: normals N x 3, and the neighbours themselves,
 *                        knn_idx / knn_d2 N x knn ascending by (d2, index), -1 / +inf where the cloud has fewer points.
 *   me_gicp_covariances  InitializePointCloudForGeneralizedICP(epsilon): C = Rx diag(epsilon,1,1) Rx^T from the normals
 *                        (estimated with knn = 20 when the slot has none); optional output N x 9 row-major.
 *   me_icp_lsq_sums      one correspondence + reduction step over the pairs of the last me_nn1(query_slot, ref) with
 *                        d2 < max_distance^2: J^T J (6x6 row-major), J^T r, sum r^2 of utility::ComputeJTJandJTr and
 *                        sum d2 (fitness = n_corr / n_source, inlier_rmse = sqrt(sum_d2 / n_corr)).  The host solves
 *                        JTJ x = -JTr, converts x with TransformVector6dToMatrix4d and calls me_transform_cloud.
 *                        ME_ICP_POINT_TO_PLANE needs normals on the ref cloud, ME_ICP_GENERALIZED covariances on both. */
#define ME_ICP_POINT_TO_PLANE 1
#define ME_ICP_GENERALIZED 2
typedef struct me_icp_lsq {
    int64_t n_corr;
    int64_t n_source;
    double JTJ[36];
    double JTr[6];
    double r2;
    double sum_d2;
} me_icp_lsq;
int me_set_normals(me_ctx *ctx, int slot, const double *normals);
int me_get_normals(me_ctx *ctx, int slot, double *normals);
int me_estimate_normals(me_ctx *ctx, int slot, int knn, double *normals, int32_t *knn_idx, double *knn_d2);
int me_gicp_covariances(me_ctx *ctx, int slot, double epsilon, double *cov);
int me_get_covariances(me_ctx *ctx, int slot, double *cov); /* the current N x 9 covariances (after any transform) */
int me_icp_lsq_sums(me_ctx *ctx, int query_slot, int mode, double max_distance, me_icp_lsq *out);

/* The same step under a robust loss: Open3D's TransformationEstimationPointToPlane(kernel) and
 * TransformationEstimationForGeneralizedICP(epsilon, kernel) [upstream], the refinement that performICPRegistration
 * (map_eval.cpp:1366-1394) asks for when the map carries ghost points.  The weights restate RobustKernel.cpp [upstream]:
 *   L1 1 / |r|      Huber k / max(|r|, k)      Cauchy 1 / (1 + (r / k)^2)      GM k / (k + r^2)^2
 *   Tukey (1 - min(1, |r| / k)^2)^2
 * Each row contributes (J[a] w) J[b] and (J[a] w) r, as utility::ComputeJTJandJTr weights them; r2 stays the unweighted
 * sum r^2.  Point-to-plane has one row per correspondence (J, r of me_icp_lsq_sums).  Generalized ICP has three, the
 * rows of W [-skew(vs) | I] and of W d with W = (Ct + Cs)^(-1/2) from a Jacobi decomposition,
 * each with its own weight.  sum_w and sum_wr2 are the sums of w and of w r^2 over the rows; n_zero_weight counts the
 * rows with w == 0 (L1 at r == 0 is one: 0 here where upstream divides by zero); n_degenerate counts the generalized
 * correspondences whose Ct + Cs has an eigenvalue <= 0 or not finite: they stay in n_corr and sum_d2 only.
 * ME_ROBUST_L2 runs me_icp_lsq_sums itself (sum_w = rows, sum_wr2 = r2).  k is read by Huber, Cauchy, GM and Tukey and
 * must be finite and > 0 for them.  Point-to-point takes no kernel (as upstream).  Single GPU: slab or shard mode is ME_ERR_ARG for
 * every kernel id, ME_ROBUST_L2 included, although me_icp_lsq_sums itself serves a shard. */
#define ME_ROBUST_L2 0
#define ME_ROBUST_L1 1
#define ME_ROBUST_HUBER 2
#define ME_ROBUST_CAUCHY 3
#define ME_ROBUST_GM 4
#define ME_ROBUST_TUKEY 5
typedef struct me_icp_robust {
    int64_t n_corr, n_source, n_zero_weight, n_degenerate;
    double JTJ[36], JTr[6], r2, sum_d2, sum_w, sum_wr2;
} me_icp_robust;
int me_icp_lsq_sums_robust(me_ctx *ctx, int query_slot, int mode, double max_distance, int kernel, double k,
                           me_icp_robust *out);

/* Open3D GetInformationMatrixFromPointClouds(source, target, max_distance, T) [upstream] for the alignment that
 * performICPRegistration (map_eval.cpp:1366-1394) ends with: info = sum G^T G over the correspondences of the last
 * me_nn1(query_slot, ref) with d2 < max_distance^2, G = [-skew(t) | I] with t the TARGET point (6x6 row-major, rotation
 * first).  An eigenvalue near zero is a direction of the pose that the pair does not constrain.  Single GPU. */
int me_icp_information(me_ctx *ctx, int query_slot, double max_distance, double info[36], int64_t *n_corr);

/* renderDistanceOnPointCloud (map_eval.cpp:586-607; raw_rendered_dis_map.pcd / inlier_rendered_dis_map.pcd, :485-495) for
 * the queries of the last me_nn1(query_slot, ...): rgb[N][3] in the caller's cloud order = ColorMapJet(min(d2, dis) / dis)
 * (the SQUARED distance against the unsquared `dis`, as the reference does; it repeats a serial KD-tree pass for it,
 * computePointCloudDistance :568-584 — the numbers are those of me_nn1).  inlier[N] (optional) = the gate of me_nn_stats,
 * i.e. the rows of corresponding_cloud_est (:1086-1087): their colours are the inlier rendering. */
int me_render_distance(me_ctx *ctx, int query_slot, double dis, double gate, int gate_mode, double *rgb, uint8_t *inlier);

/* ColorPointCloudByMME(pointcloud, entropies) (map_eval.cpp:686-735; map_entropy.pcd / gt_entropy.pcd) from the last
 * me_mme(slot): the VALID points in cloud order with their Jet colour of the log-mapped normalised |entropy|; range =
 * (|max|, |min|) over the non-zero entropies (:696-699).  xyz = rgb = NULL: count and range only. */
int me_render_entropy(me_ctx *ctx, int slot, double *xyz, double *rgb, int64_t capacity, int64_t *n_valid, double *min_abs,
                      double *max_abs);

/* computeChamferDistance (map_eval.cpp:1398-1431): both directions, no gate.  Runs me_nn1 both ways. */
int me_chamfer(me_ctx *ctx, double *cd);

/* ---- MME: ComputeMeanMapEntropyUsingNormalTBB / UsingNormal / ComputeMeanMapEntropy
 *      (map_eval.cpp:1608-1737, 1538-1606, 1438-1535) ------------------------------------------------------------ */
/* min_k: 10 for the estimated cloud (:1675), 5 for the GT cloud (:1458).  entropies[N] (0.0 where invalid) and
 * valid[N] are in cloud order, nullable.  sum_H / n_valid are shard-local partial sums; the mean entropy is
 * sum_H / n_valid (0 when n_valid == 0, :1720-1724).
 * INDEX.  A slot whose cell edge is below radius (1 + 2^-20) or above 1.5 times that is re-indexed at `radius` (the rule every
 * radius pass shares); that discards what a re-sort of the slot discards: the 1-NN results of both slots and the slot's local-geometry,
 * M3C2 and mesh-distance results.  me_mme ADOPTS its radius as the cell size asked for on the slot (the lazy choice
 * me_upload_cloud's cell_size <= 0 leaves to it): every later rebuild of the slot's index that uses the requested cell
 * (me_transform_cloud, the device-side producers, a missing index) builds at `radius`.  So do me_run_suite, through its two me_mme
 * calls, and me_run_suite_from, which settles both slots' indexes at nn_radius before its lanes start: after either, nn_radius is the
 * cell size asked for on both slots.  The other radius passes - me_radius_outlier, me_cluster_dbscan, me_local_geometry,
 * me_radius_normals, me_m3c2 and me_reconstruct - borrow the index: they restore the cell size asked for before. */
int me_mme(me_ctx *ctx, int slot, double radius, int min_k, double *entropies, uint8_t *valid, double *sum_H,
           int64_t *n_valid);
/* The per-point arrays of the slot's LAST MME pass (me_mme, me_run_suite, me_run_suite_from), as me_mme returns them: what
 * est_entropies / valid_entropy_points / gt_entropies hold after computeMME (map_eval.cpp:149-189).  Either may be NULL. */
int me_mme_fetch(me_ctx *ctx, int slot, double *entropies, uint8_t *valid);

/* ---- voxel Gaussians: VoxelCalculator::buildVoxelMap + computeVoxelEntropy (voxel_calculator.cpp:21-56,97-113) */
/* Output rows are in ascending (ix,iy,iz) order.  sigma is AS STORED by the reference after buildVoxelMap, i.e.
 * M2/(n-1)^2 for n > 10 and raw M2 otherwise (row-major 3x3).  *n_voxels in: capacity, out: count
 * (ME_ERR_CAPACITY if too small; pass all-NULL arrays to query the count). */
int me_voxel_gaussians(me_ctx *ctx, int slot, double voxel_size, int32_t *keys /*V x 3*/, int32_t *npts /*V*/,
                       double *mu /*V x 3*/, double *sigma /*V x 9*/, double *entropy /*V*/, int64_t *n_voxels);

/* ---- per-voxel AC / COM / CD / MME on the AWD voxel lattice (no reference counterpart: the reference reports one scalar per map) -- */
/* Per-voxel breakdown of the last me_nn1(slot, other) statistics and the slot's last MME, on the voxel lattice of
 * VoxelCalculator::getVoxelIndex (voxel_calculator.cpp:241-245).  Rows in ascending (ix,iy,iz) order = the rows of
 * me_voxel_gaussians(slot, voxel_size).  nn[v] sums exactly what me_nn_partial_sums sums (map_eval.cpp:1069-1145, 1416),
 * over the points of voxel v (n_query = its point count).  sum_H / n_H: entropies of the valid points
 * (map_eval.cpp:1692-1697).  *have_mme = 0 (and zero columns) when the slot has no MME result.
 * *n_voxels in: capacity, out: count (all-NULL arrays: count only; ME_ERR_CAPACITY if too small).  Host pointers.
 * Points are binned by their CURRENT coordinates: after me_run_suite_from(T) or a registration transform that is the transformed
 * frame, the one AC and AWD are measured in.  Entropies stay with their points by point index, and MME runs on the map AS LOADED
 * (map_eval.cpp:56, before the transform at :1206): a point's entropy describes its neighbourhood before the transform.
 * me_transform_cloud discards the slot's MME result (me_run_suite_from carries it across its own transform); hand it back with
 * me_set_mme_result to keep the entropy columns after a registration.
 * Summed over all rows: the integer columns equal me_nn_partial_sums exactly, the doubles to rounding; sum n_H = the MME valid
 * count, sum sum_H = the MME sum.  Bit-identical from call to call.  ME_ERR_STATE: slot not uploaded, no me_nn1 with this slot as
 * the query since its last upload or transform, or slab / shard mode.  ME_ERR_ARG: voxel_size <= 0, or a voxel index outside
 * |floor(p / voxel_size)| < 2^20.  One pass over the sorted cloud plus a sort of ~n / 60 run records (device timer "voxel_metrics"). */
int me_voxel_metrics(me_ctx *ctx, int slot, double voxel_size, double gate, int gate_mode, const double trunc[5],
                     int32_t *keys /*V x 3*/, me_nn_partial *nn /*V*/, double *sum_H /*V*/, int64_t *n_H /*V*/,
                     int *have_mme, int64_t *n_voxels);

/* ---- per-voxel rigid deformation field from the resident 1-NN pairs (no reference counterpart: map_eval.cpp reports scalars only) -- */
/* (DESIGN.md section 4.22).  Which way, and by how much, has each voxel of the query cloud moved against the reference cloud: the pair
 * moments of the last me_nn1(query_slot, ..) per voxel of the lattice of me_voxel_gaussians(query_slot, voxel_size) (same keys, same
 * row order, a row for EVERY voxel of the query cloud), a rigid fit per voxel (Horn's closed form) and the share of the squared error
 * that fit explains.  Nothing resident is changed but the result itself.
 *   PAIRS   point i of the voxel is a pair iff d2_i >= 0, d2_i < max_distance^2 (strict: Open3D's SearchHybrid, as me_icp_p2p_sums;
 *           max_distance = +inf takes every d2 >= 0) and nn_idx_i names a reference point (a result placed by me_set_nn_result has
 *           no neighbour indices: none of its pairs is used).  p = the query point, q = the reference point, both in CURRENT
 *           coordinates; o = (double(k) * voxel_size + 0.5 * voxel_size) per axis, the voxel's centre; a = p - o, b = q - o.
 *   SUMS    23 doubles per voxel: sum a (3), sum b (3), sum a b^T (9, row-major), sum a a^T (6: xx, xy, xz, yy, yz, zz), sum |b|^2,
 *           sum d2 (the resident values).  Fixed-order sums, no floating-point atomics, added in the POINTS' OWN order (by voxel,
 *           inside a voxel by original point index): bit-identical from call to call and after any re-index of the same points.
 *   FIT     with n the voxel's pair count: abar = sum a / n, bbar = sum b / n, t0 = bbar - abar (the mean displacement);
 *           S = sum a b^T - (sum a)(sum b)^T / n, C = sum a a^T - (sum a)(sum a)^T / n.  ME_DEFORM_FIT: n >= min_pairs.
 *           ME_DEFORM_ROT_OK: FIT and the middle eigenvalue of C >= n * min_spread^2 (a collinear or single-point source has no
 *           rotation).  With ROT_OK R = horn_rotation(S), the least-squares rotation a - abar -> b - bbar, and u = bbar - R abar,
 *           the fit's displacement at the voxel centre; otherwise R = I and u = t0.  e0 = sum d2; e_t = max(0, sum d2 - n |t0|^2),
 *           what is left after the mean displacement; e_R = max(0, tr C + (sum |b|^2 - |sum b|^2 / n) - 2 sum_rc R_rc S_cr), the
 *           sum of |R (a - abar) - (b - bbar)|^2 over the pairs: what is left after the rigid fit, with ROT_OK, else e_R = e_t.  n = 0: t0 = u = 0, R = I, every residual 0.
 *   out     the totals over the rows in key order, added in the fixed order of the per-cloud totals.
 * me_voxel_deformation_fetch: the rows of the last me_voxel_deformation(query_slot, ..): every array may be NULL; *n_voxels in:
 * capacity, out: count (all-NULL arrays: count only; ME_ERR_CAPACITY if too small).  Host pointers.  e = [e0, e_t, e_R] per row.
 * The rows stay on the query cloud exactly as long as its 1-NN result: a new search (me_nn1, me_set_nn_result, the suite), an upload
 * or a transform of either slot, or an index rebuild of either slot discards them (ME_ERR_STATE from the fetch).
 * ME_ERR_STATE: slot not uploaded, no me_nn1 with this slot as the query since the last upload or transform of either slot, or slab
 * / shard mode.  ME_ERR_ARG: voxel_size <= 0, max_distance <= 0 or NaN, min_pairs < 3, min_spread < 0 or NaN, or a voxel index
 * outside |floor(p / voxel_size)| < 2^20.  A sort of n (key, position) pairs, one pass over the cloud and a sort of ~n / 60 run records (device timer
 * "voxel_deformation": the kernels; the sorts are under "sort").
 * LIMITATION: 1-NN pairs under-report motion tangential to a surface; on a single plane u is reliable along the normal only, and the
 * rigid share 1 - sum e_R / sum e0_fit is a lower bound of the drift share. */
#define ME_DEFORM_FIT 1
#define ME_DEFORM_ROT_OK 2
#define ME_DEFORM_SUMS 23
typedef struct {
    int64_t n_voxels, n_with_pairs, n_fit, n_rot; /* rows, rows with n > 0, with FIT, with ROT_OK */
    int64_t n_pairs;                              /* sum n = me_icp_p2p_sums(query_slot, max_distance).n_corr for a searched result */
    int64_t max_row;                              /* row of max_t0 (ties: the smallest row); -1 without a FIT row */
    int32_t max_key[3];                           /* its voxel key */
    int32_t pad_;
    double sum_n_t0, sum_n_t0sq;                  /* sum n |t0|, sum n |t0|^2 over all rows */
    double max_t0;                                /* the largest |t0| of a FIT row (0 without one) */
    double sum_e0, sum_e_t;                       /* over all rows */
    double sum_e0_fit, sum_e_R;                   /* over the FIT rows */
} me_deform_summary;
int me_voxel_deformation(me_ctx *ctx, int query_slot, double voxel_size, double max_distance, int min_pairs, double min_spread,
                         me_deform_summary *out);
int me_voxel_deformation_fetch(me_ctx *ctx, int query_slot, int32_t *keys /*V x 3*/, int64_t *n_pairs /*V*/, uint8_t *flags /*V*/,
                               double *sums /*V x 23*/, double *t0 /*V x 3*/, double *u /*V x 3*/, double *R /*V x 9*/,
                               double *e /*V x 3*/, int64_t *n_voxels);

/* ---- per-voxel distribution distances on the AWD lattice: point-set MMD, KL, Bhattacharyya and the textbook W2 (the reference
 *      declares computeKLDivergenceGaussian, computeGaussianKernel, computeGaussianBhattacharyya and computeMMD at
 *      voxel_calculator.hpp:71-79 and defines none of them) ---------------------------------------------------------------------- */
/* (DESIGN.md section 4.24).  AWD's W is close to the offset of two centroids wherever the reference's formula clamps the eigenvalues;
 * these columns compare the SHAPES of what the two clouds hold in a voxel.  Both resident clouds, single GPU.
 *   ROWS    exactly the voxels for which me_awd_scs(voxel_size, min_pts, ..) emits a row: the keys present in both clouds with both
 *           populations >= min_pts, ascending (ix, iy, iz), on the lattice of me_voxel_gaussians (floor(p / voxel_size), CURRENT
 *           coordinates).  n_pop[v] = the two populations (est, gt).
 *   POINTS  X = the map's points in the voxel, Y = the ground truth's, each in ascending ORIGINAL point index.  With max_points > 0
 *           and a population n > max_points only every s-th point of that list is used, starting at the first, s = ceil(n /
 *           max_points): ceil(n / s) points.  max_points = 0: all points.  n_used[v] = the used counts (n, m); the min_pts gate
 *           always looks at the full population.
 *   MMD     per bandwidth sigma_b, b < n_sigma: g_b = 1.0 / (2.0 * sigma_b * sigma_b) (host), d2 = ((dx dx) + (dy dy)) + (dz dz)
 *           from the coordinates as stored (no recentring, no FMA: the d2 of every other kernel), k_b(x, y) = exp(-(d2 * g_b)) in
 *           fp64.  ksum[v][b] = Sxx, Syy, Sxy with Sxx = sum_{i<j} k(x_i, x_j), Syy likewise, Sxy = sum_i sum_j k(x_i, y_j).
 *           mmd2[v][b] = u, b:  u = 2 Sxx / (n (n - 1)) + 2 Syy / (m (m - 1)) - 2 Sxy / (n m)   (the unbiased estimate),
 *                               b = (n + 2 Sxx) / n^2 + (m + 2 Syy) / m^2 - 2 Sxy / (n m)        (the biased one);
 *           mmd = sqrt(max(0, b)).  Fixed-order sums in the points' own order, no floating-point atomics: bit-identical from call
 *           to call and after any re-index of the same points (the sorted order of a cloud decides nothing).
 *   GAUSS   from both voxels' n, mu and sigma AS me_voxel_gaussians REPORTS THEM (min_pts >= 11, so sigma is M2 / (n - 1)^2): the
 *           sample covariance C = sigma * (n - 1) elementwise, its symmetric part, jacobi_sym, the eigenvalues raised to eig_floor:
 *           S~ = V diag(l~) V^T, ln det = sum ln l~.  d = mu_gt - mu_est.  gauss[v] =
 *             KL(est || gt) = 1/2 [tr(S~g^-1 S~e) + d^T S~g^-1 d - 3 + ln det S~g - ln det S~e],
 *             KL(gt || est), the same with the roles swapped,
 *             Bhattacharyya = 1/8 d^T S^-1 d + 1/2 [ln det S - 1/2 (ln det S~e + ln det S~g)], S = (S~e + S~g) / 2 decomposed the
 *               same way,
 *             W2 = sqrt(max(0, |d|^2 + tr S~e + tr S~g - 2 tr (S~e^1/2 S~g S~e^1/2)^1/2)), both square roots by jacobi_sym: the textbook
 *               2-Wasserstein distance, which the reference's W is not (SURVEY finding 2).
 *           A function of the two voxel tables alone: bit-identical from call to call, and across every re-sort, because a slot keeps
 *           its table until its points are replaced (a table built afresh under another sorted order sums in that order and may
 *           differ in the last bits, as me_voxel_gaussians' own output does).
 *   out     n_rows; n_rows_subsampled = rows with s > 1 on either side; n_pairs = sum over the rows of n (n - 1) / 2 + m (m - 1) / 2
 *           + n m; mean_mmd[b], mean_mmd2_u[b] (b < n_sigma, NaN past it) and mean_gauss[4], the means over the rows, added in the
 *           fixed order of the per-cloud totals; NaN with no rows, as AWD is.
 * Host pointers; every array and `out` may be NULL.  *n_rows in: capacity, out: count (ME_ERR_CAPACITY if an array is passed and the
 * capacity is too small).  All arrays and `out` NULL: the row count alone, no pass over the points; all arrays NULL with `out`: the
 * summary.  Nothing resident changes but the two slots' cached voxel tables, which are (re)built at voxel_size exactly as me_awd_scs
 * and me_voxel_gaussians build them; the 1-NN, MME and every other per-point result stay.
 * ME_ERR_ARG: voxel_size <= 0, min_pts < 11, n_sigma outside 1 .. 4, a sigma that is <= 0 or NaN, max_points < 0 or in 1 .. 10,
 * eig_floor <= 0 or NaN, or a voxel index outside |floor(p / voxel_size)| < 2^20.  ME_ERR_STATE: a slot not uploaded, or slab / shard
 * mode.  A refused call changes nothing.  Cost: a sort of (key, position) pairs per cloud and one exp per pair and bandwidth (device
 * timer "voxel_distances": the kernels; the sorts are under "sort"). */
typedef struct {
    double voxel_size;
    int32_t min_pts, n_sigma;
    double sigma[4];
    int64_t max_points;
    double eig_floor;
} me_voxdist_params;
typedef struct {
    int64_t n_rows, n_rows_subsampled, n_pairs;
    double mean_mmd[4], mean_mmd2_u[4], mean_gauss[4];
} me_voxdist_out;
int me_voxel_distances(me_ctx *ctx, const me_voxdist_params *p, int32_t *keys /*V x 3*/, int32_t *n_pop /*V x 2*/, int32_t *n_used /*V x 2*/,
                       double *ksum /*V x n_sigma x 3*/, double *mmd2 /*V x n_sigma x 2*/, double *gauss /*V x 4*/,
                       int64_t *n_rows /*in: capacity, out: count*/, me_voxdist_out *out);

/* ---- per-voxel point-set Wasserstein distances on the AWD lattice: sliced W2 and the debiased Sinkhorn divergence (no reference
 *      counterpart: AWD is called a Wasserstein distance and computes none between the points of a voxel).  DESIGN.md 4.26 --------
 * The rows, the gate, the points X (map) and Y (ground truth) of a row and the stride rule are those of me_voxel_distances, with
 * max_points in 11 .. 1024 (both used point sets of a row stay in one workgroup's LDS).  n = |X used|, m = |Y used|.
 *   SLICED  n_dir = L directions u_l (fp64 triples, used AS GIVEN: not normalised).  Per row and direction the projections
 *           p = ((x ux) + (y uy)) + (z uz) (no FMA, coordinates as stored) of both sides are sorted ascending (a_i, b_j) and
 *             W2^2_l = (sum w_ij ((a_i - b_j) (a_i - b_j))) / (n m),
 *           w_ij the INTEGER overlap of [i m, (i + 1) m) and [j n, (j + 1) n): the exact squared 2-Wasserstein distance of the two
 *           empirical measures on the line, n + m - gcd(n, m) terms.  ORDER: lane t of 256 takes i = t, t + 256, ... ascending, for each i
 *           the overlapping j ascending, one fp64 accumulator; the lanes fold by wave_sum (shuffle down 32 .. 1), the four waves as
 *           (s0 + s1) + (s2 + s3); then one division by (double) n * (double) m.  A function of n, m and the points alone.
 *           sliced[v] = sw2_sq (the sum over l ascending, divided by (double) L), sw2 = sqrt(sw2_sq), max_sw2_sq = the largest
 *           W2^2_l, and the index l that attains it as a double (the smallest on ties).  per_direction[v][l] = W2^2_l.
 *   SINKHORN  cost C_ij = ((dx dx) + (dy dy)) + (dz dz), weights 1 / n and 1 / m, n_eps = T iterations, iteration t at eps[t], no
 *           convergence test.  From f = g = 0, per iteration
 *             f_i <- -eps (M_i + log sum_j exp(t_ij - M_i)),  t_ij = lb + (g_j - C_ij) / eps,  M_i = max_j t_ij,  lb = -log((double) m),
 *           the sum in ascending j (two passes over j: the maximum, then the sum; t_ij is formed the same way in both, so the sum is
 *           >= 1), then g_j likewise from the new f with la = -log((double) n).  The symmetric problems (X, X) and (Y, Y) iterate
 *           f_i <- 0.5 (f_i + T(f)_i), every T(f)_i from the f of the iteration before.  OT(X, Y) = (sum f_i) / n + (sum g_j) / m,
 *           OT(X, X) = (sum f_i) / n + (sum f_i) / n; each sum: lane t takes t, t + 256, ... ascending, then the fold above.
 *           S = (OT(X, Y) - 0.5 OT(X, X)) - 0.5 OT(Y, Y).  marginal_err = sum_i | sum_j exp((la + lb) + ((f_i + g_j) - C_ij) / eps) - 1 / n |
 *           at eps[T - 1] with the final f and g (j ascending, the i as the sums above): the L1 distance of the plan's first marginal
 *           from 1 / n, which tells whether T was enough (the second marginal is exact after the g update).
 *           sinkhorn[v] = OT(X, Y), OT(X, X), OT(Y, Y), S, sqrt(max(0, S)), marginal_err.  potentials: the final f of the cross
 *           problem of all rows, row after row (sum of n_used[v][0] doubles), then the final g (sum of n_used[v][1]): out->n_used_est
 *           and out->n_used_gt are those sums, and a call with n_used alone (no solver runs) tells them beforehand.
 *   out     n_rows; n_rows_subsampled; n_pairs = sum n m; n_used_est, n_used_gt; mean_sw2 and mean_max_sw2 (of sqrt(max_sw2_sq)),
 *           mean_s, mean_sinkhorn, mean_marginal_err over the rows in the fixed order of the per-cloud totals; max_marginal_err and
 *           its row (-1 without rows).  NaN for a part that did not run (n_dir = 0 or n_eps = 0) and with no rows.
 * No floating-point atomics: bit-identical from call to call and after any re-index of the same points.  n_dir = 0 skips the sliced
 * part (sliced and per_direction are not written), n_eps = 0 the Sinkhorn part; the other part's bytes do not change.
 * Host pointers; every array and `out` may be NULL.  *n_rows in: capacity, out: count (ME_ERR_CAPACITY if an array is passed and the
 * capacity is too small).  All arrays and `out` NULL: the row count alone; only keys / n_pop / n_used: the rows, no solver.
 * ME_ERR_ARG: voxel_size <= 0, min_pts < 11, n_dir outside 0 .. 64, n_eps outside 0 .. 512, n_dir = n_eps = 0, directions NULL with
 * n_dir > 0, eps_schedule NULL with n_eps > 0 or not positive and non-increasing (NaN included), max_points outside 11 .. 1024, or a
 * voxel index out of range.  ME_ERR_STATE: a slot not uploaded, or slab / shard mode.  A refused call changes nothing.
 * Cost: one exp per pair, half-update and iteration (device timer "voxel_transport"). */
typedef struct {
    double voxel_size;
    int32_t min_pts, n_dir, n_eps, reserved;
    int64_t max_points;
} me_voxtrans_params;
typedef struct {
    int64_t n_rows, n_rows_subsampled, n_pairs, n_used_est, n_used_gt, max_marginal_row;
    double mean_sw2, mean_max_sw2, mean_s, mean_sinkhorn, mean_marginal_err, max_marginal_err;
} me_voxtrans_out;
int me_voxel_transport(me_ctx *ctx, const me_voxtrans_params *p, const double *directions /*n_dir x 3*/, const double *eps_schedule /*n_eps*/,
                       int32_t *keys /*V x 3*/, int32_t *n_pop /*V x 2*/, int32_t *n_used /*V x 2*/, double *sliced /*V x 4*/,
                       double *sinkhorn /*V x 6*/, double *per_direction /*V x n_dir*/, double *potentials /*n_used_est + n_used_gt*/,
                       int64_t *n_rows /*in: capacity, out: count*/, me_voxtrans_out *out);

/* ---- AWD + CDF + SCS: MapEval::calculateVMD (map_eval.cpp:240-390) with updateVoxelMap (voxel_calculator.cpp:
 *      142-172) and computeWassersteinDistanceGaussian (:115-140) ------------------------------------------------ */
/* rows: n x 27 doubles in the column order of voxel_errors.txt (map_eval.cpp:292-302), ascending key order;
 * w_sorted: ascending W (the CDF file's first column, :330-340); both nullable.  *n_rows in: capacity, out: count.
 * awd = mean W (NaN if no voxel qualifies, :324), scs as :347-389 (NaN if no voxel has a neighbour).
 * counts[3] = active / old / new voxel counts (voxel_calculator.cpp:170), nullable. */
int me_awd_scs(me_ctx *ctx, double voxel_size, int min_pts /*100, :280*/, int scs_radius /*5, :353*/,
               double *rows, double *w_sorted, int64_t *n_rows, double *awd, double *scs, int64_t counts[3]);

/* Batched VoxelCalculator::computeWassersteinDistanceGaussian(voxel1, voxel2) (voxel_calculator.hpp:69,
 * voxel_calculator.cpp:115-140) on caller-provided Gaussians: mu*[count][3], sigma*[count][9] (row-major, AS STORED
 * in VoxelInfo::sigma), n*[count] -> w[count].  Host pointers.  Lets the reference's own voxel_errors.txt be replayed
 * through the device kernel.  n <= 1: the identity stands in for the matrix, which is not read (:118, :126); otherwise
 * sigma / (n - 1), its symmetric part, eigenvalues raised to 1e-6.  W = sqrt(max(0, D)) with max(0, NaN) = 0 as std::max(0.0, NaN):
 * a NaN in mu or in a matrix that is read, or a Cholesky pivot that rounding made negative, gives W = 0, never NaN. */
int me_w2_batch(me_ctx *ctx, const double *mu1, const double *sigma1, const int32_t *n1, const double *mu2,
                const double *sigma2, const int32_t *n2, int64_t count, double *w);

/* SCS of a caller-provided sparse W table (map_eval.cpp:347-389): keys[n][3] voxel indices, w[n].  Host pointers.
 * scs_radius in [1, 10] (here and in me_awd_scs; the stencil's (2 r + 1)^3 doubles live in LDS, 74,088 bytes at 10; a launch the
 * device refuses is ME_ERR_HIP, never ME_OK).  n = 0, or no voxel with a neighbour: NaN.  ME_ERR_ARG: a voxel index outside
 * |index| < 2^20 - 16; a w that is negative or NaN (W is a distance; +0, -0 and large values are values like any other, and a
 * voxel whose neighbours are all 0 gives 0 / 0 = NaN as the reference does); a key listed twice (the reference's map holds one W per
 * voxel). */
int me_scs_table(me_ctx *ctx, const int32_t *keys, const double *w, int64_t n, int scs_radius, double *scs);

/* ---- whole suite in one call (what MapEval::process runs between load and save, map_eval.cpp:52-85) -------- */
typedef struct me_suite_params {
    double icp_max_distance; /* Param::icp_max_distance_ */
    int gate_mode;           /* ME_GATE_* */
    double trunc[5];         /* Param::trunc_dist_ */
    double nn_radius;        /* Param::nn_radius_ */
    double vmd_voxel_size;   /* Param::vmd_voxel_size_ */
    int evaluate_mme;        /* Param::evaluate_mme_ */
    int evaluate_gt_mme;     /* Param::evaluate_gt_mme_ */
    int min_pts;             /* 100 */
    int scs_radius;          /* 5 */
} me_suite_params;

typedef struct me_suite_out {
    me_nn_stats_out est_gt; /* est_gt_results */
    me_nn_stats_out gt_est; /* gt_est_results (intended (gt_i, map_nn) pairing; see DESIGN.md deviation #4) */
    double full_chamfer;    /* full_chamfer_dist */
    double mme_est, mme_gt; /* mme_est / mme_gt */
    int64_t mme_est_valid, mme_gt_valid;
    double awd, scs;        /* vmd / scs_overall */
    int64_t n_w_voxels;
    double stage_ms[8];     /* host wall clock per stage (each ends with a stream sync): [1] nn est->gt, [2] nn gt->est,
                             * [3] statistics, [4] mme est, [5] mme gt, [6] voxel Gaussians + AWD + CDF + SCS, [7] the whole call;
                             * [0]: me_run_suite_from only (upload + index) */
} me_suite_out;

int me_run_suite(me_ctx *ctx, const me_suite_params *p, me_suite_out *out);

/* The same pass STARTING FROM THE TWO RAW CLOUDS — one call for everything MapEval::process() does between VoxelDownSample
 * (map_eval.cpp:38-39) and the result writers: upload + index of both clouds, computeMME(map_3d_, gt_3d_) (:56) on the map AS
 * LOADED, *map_3d_ = map_3d_->Transform(T) (:1206; T row-major 4x4, NULL or the identity = none), both 1-NN directions with the
 * AC / COM / CD statistics (:76), voxel Gaussians, AWD, CDF, SCS (:85).  The caller stays single-threaded (as process() is, :4).
 *   est / gt           double[n][3] — host memory, or device memory with ME_SUITE_DEVICE_INPUT; both NULL = run on the clouds
 *                      already uploaded to the two slots (e.g. after me_voxel_downsample).  With resident clouds T is applied to
 *                      the resident map IN PLACE, as :1206 overwrites map_3d_: a second call with the same T != identity
 *                      transforms it again (and computes the MME on the already transformed map) — upload afresh, or pass the
 *                      identity, to evaluate the same pose twice.  An index that is missing or does not fit nn_radius is rebuilt
 *                      on nn_radius' lattice before the stages (and the second lane) start: the call from resident clouds returns
 *                      what the call from the raw clouds returns, bit for bit.
 *   ME_SUITE_OVERLAP   two lanes: the calling thread drives `ctx`, an internal thread drives me_twin(ctx) on its own low-priority
 *                      stream — the ground truth is uploaded / indexed and both voxel tables are built UNDER the map's VALU-bound
 *                      MME kernel, and each lane searches one 1-NN direction (schedule: csrc/me_suite.hip).  Same kernels on the
 *                      same data: every result is bit-identical to the call without the flag and to me_run_suite.
 * Afterwards the per-point products are on the device as after the separate calls: me_mme_fetch, me_nn_fetch,
 * me_render_entropy / me_render_distance, me_awd_scs(rows, w_sorted) (cached tables), me_download_cloud (the transformed map).
 * stage_ms: wall clock of the calling thread per stage — [0] upload + index (+ transform) of the map (without ME_SUITE_OVERLAP: of
 * both clouds), [1] 1-NN map -> ground truth + partial sums, [2] the other direction (with ME_SUITE_OVERLAP: the wait for the second
 * lane), [3] sigma passes, [4] MME map, [5] MME ground truth, [6] AWD + CDF + SCS (+ voxel tables without the second lane),
 * [7] the whole call. */
#define ME_SUITE_OVERLAP 1
#define ME_SUITE_DEVICE_INPUT 2
#define ME_SUITE_PIN_HOST_INPUT 4 /* host input: page-lock the caller's two buffers for the duration of the call (hipHostRegister;
                                   * ~2 ms per 1.2 GB where measured), so that pageable memory — a std::vector, Open3D's points_ —
                                   * crosses PCIe at the pinned rate (21 instead of 30 ms per 50 M points); already pinned: no-op */
int me_run_suite_from(me_ctx *ctx, const double *est, int64_t n_est, const double *gt, int64_t n_gt, const double *T_rowmajor4x4,
                      const me_suite_params *p, int flags, me_suite_out *out);

/* ---- instrumentation (bench.py roofline leg) ------------------------------------------------------------- */
/* Average device time (ms, HIP events on the context's stream) and launch count of a named kernel family since
 * the last me_timers_reset: "nn_grid", "nn1", "mme", "sort", "morton", "gather", "cells" (the cell tables), "octree", "nn_stats", "voxel", "voxel_metrics", "voxel_deformation", "w2", "scs", "slab_filter", "halo_pack", "perturb", "fpfh", "fpfh_match", "ransac", "ransac_validate", "plane", "plane_score", "mom", "group_select".  Enabled by me_timers_enable(1).
 * Counters (total_ms = 0, value in *launches): "mme_pairs" (accepted (query, neighbour) pairs of the MME launches: the useful work of
 * the VALU-bound kernel, bench.py's roofline.valu), "mme_refined" (queries whose thin neighbourhood — smallest covariance eigenvalue below ~1.8e-6 cell^2 — the MME pass
 * recomputed two-pass about the query itself; counted whether or not timers are on), "nn_queries" / "nn_fallback_queries" (1-NN queries, and those that needed the
 * octree pass), "nn1_opened" / "nn1_scans" / "nn1_points" / "nn1_max_opened" (octree walk: nodes opened, leaf cells and points
 * scanned, the longest chain of one query in the octet walk), "nn1_far" (walks handed over to the wave-per-query kernel). */
/* Debug: one cell table of an indexed slot as it lies on the device (which: 0 the radius grid, 1 the 1-NN grid).  *n_slots = size of the
 * open-addressing table, *n_cells = occupied cells; hkeys[n_slots] (empty = all ones), hvals[n_slots] (cell index; undefined in empty
 * slots), cell_start[n_cells + 1] (runs of the sorted points) and entries[n_slots] x 16 bytes {uint64 key; uint32 start; uint32 count}:
 * the record of the same slot that the per-round tables of the radius and 1-NN kernels probe.  Any array may be NULL (sizes only).
 * ME_ERR_STATE without an index. */
int me_cell_table_fetch(me_ctx *ctx, int slot, int which, int64_t *n_slots, int64_t *n_cells, uint64_t *hkeys, uint32_t *hvals,
                        uint32_t *cell_start, void *entries);
int me_timers_enable(me_ctx *ctx, int on);
int me_timers_reset(me_ctx *ctx);
int me_timer_get(me_ctx *ctx, const char *name, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif
