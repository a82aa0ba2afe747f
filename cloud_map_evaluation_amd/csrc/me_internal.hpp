// me_internal.hpp — shared declarations of libmapeval_hip.so (gfx950 only; no CPU fallback anywhere).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/mapeval_hip.h"

namespace me {

constexpr int kFan = 8;        // children per octree node
constexpr int kMaxLevels = 17; // octree levels above the leaf cells (taken-masks: 2 x 64 bits)
constexpr int kMortonBits = 21;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    bool owned = true;  // false: `p` is the caller's memory (ME_FLAG_BORROW_DEVICE_INPUT), read-only for the library
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    hipError_t ensure(size_t b) {
        if (owned && b <= bytes && p) return hipSuccess;
        release();
        if (b == 0) b = 16;
        hipError_t e = hipMalloc(&p, b);
        if (e == hipSuccess) bytes = b;
        else p = nullptr;
#ifdef ME_POISON_ALLOC  // debug builds (make EXTRA=-DME_POISON_ALLOC): fresh device memory is filled with a pattern, so that a kernel
        // which reads a buffer before anything wrote it shows at once (hipMalloc hands out zeroed pages in a fresh process and
        // recycled, dirty ones after a hipFree: such a bug appears only when a second context is created in a long-lived process)
        if (e == hipSuccess) (void) hipMemset(p, 0xCD, b);
#endif
        return e;
    }
    void release() {
        if (p && owned) (void) hipFree(p);
        p = nullptr;
        bytes = 0;
        owned = true;
    }
    void borrow(void *ptr, size_t b) {
        release();
        p = ptr;
        bytes = b;
        owned = false;
    }
    // before the library writes into the buffer: a borrowed one becomes a private copy
    hipError_t make_owned(hipStream_t stream) {
        if (owned) return hipSuccess;
        void *src = p;
        const size_t b = bytes;
        p = nullptr;
        bytes = 0;
        owned = true;
        hipError_t e = ensure(b);
        if (e == hipSuccess) e = hipMemcpyAsync(p, src, b, hipMemcpyDeviceToDevice, stream);
        return e;
    }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
    // for kernels that WRITE the buffer: a borrowed buffer (the caller's memory, ME_FLAG_BORROW_DEVICE_INPUT) yields nullptr — a writer
    // that forgot ensure() / make_owned() faults at once instead of changing the caller's cloud
    template <class T>
    T *as_mut() const { return owned ? reinterpret_cast<T *>(p) : nullptr; }
};

// Sorted point: xyz in fp64 + original index (bit pattern of an int64 in w).
struct alignas(32) SPoint {
    double x, y, z;
    long long idx;
};

// Sparse octree over the Morton prefixes of the sorted points (the general 1-NN path).  Level 0 = the occupied cells of
// the 1-NN grid (each a contiguous run of `sp`), level l+1 = their unique 3-bit-shorter prefixes, up to a single root.
// A node's children are contiguous on the level below; every node's box lies inside its octree cell, so boxes of one
// level never straddle a Morton seam (a fixed-count grouping of consecutive points does, and was measured to cost
// ~150 node visits per query instead of ~20).
struct alignas(32) ONode {
    float lo[3], hi[3];   // tight fp32 box of the points below, rounded OUTWARD from the fp64 extent
    unsigned int begin;   // first child on the level below (level 0: first point); the node after it holds the end
    unsigned int parent;  // index on the level above
};
struct OctView {
    const ONode *nodes;
    const unsigned int *pbegin;  // first sorted point below every node (indexed like `nodes`; a level's terminator holds n)
    int n_levels;  // level 0 = leaf cells ... level n_levels-1 = root (1 node)
    long long count[kMaxLevels];
    long long off[kMaxLevels];  // offset of each level inside `nodes` (each level stores count + 1 records)
};

struct GridView {
    const unsigned long long *cell_code;  // unique cell Morton codes, in the order of the sorted points [n_cells]
    const unsigned int *cell_start;       // [n_cells + 1] offsets into the sorted points
    const unsigned long long *hkeys;      // open-addressing table, EMPTY = ~0ull
    const unsigned int *hvals;            // cell index
    unsigned int hmask;
    long long n_cells;
    int shift;                            // fine Morton code >> (3*shift) = cell code
    const struct CellEntry *hent;         // the same table, slot for slot, as one 16-byte record per occupied cell
};
// One slot of GridView::hent: everything a probe of wave_group_table wants from hkeys[s] -> hvals[s] -> cell_start[ci], cell_start[ci + 1]
// in ONE 16-byte load.  Same slot function, same linear probing, same empty key (an empty slot is all ones) as hkeys / hvals.
struct alignas(16) CellEntry {
    unsigned long long key;
    unsigned int start, count;  // the cell's run of the sorted points
};
static_assert(sizeof(CellEntry) == 16, "one global_load_dwordx4 per probe");

struct GridTable {
    DevBuf cell_code, cell_start, hkeys, hvals;  // (hkeys: the keys, then — 16-byte aligned — the CellEntry table: one fill for both)
    int shift = -1;
};

// Spatial slab of a context (multi-GPU): a point is OWNED iff lo <= p[axis] < hi; [reg_lo, reg_hi) = slab + halo is
// everything the context holds.  axis < 0: no slab, every point is owned.  +-inf faces never fail a test.
struct SlabView {
    int axis;
    double lo, hi;
    double reg_lo, reg_hi;
};
#ifdef __HIPCC__
__device__ __forceinline__ bool slab_owned(const SlabView &s, double x, double y, double z) {
    if (s.axis < 0) return true;
    const double v = s.axis == 0 ? x : (s.axis == 1 ? y : z);
    return v >= s.lo && v < s.hi;
}
__device__ __forceinline__ double slab_face_distance(const SlabView &s, double x, double y, double z) {
    if (s.axis < 0) return INFINITY;
    const double v = s.axis == 0 ? x : (s.axis == 1 ? y : z);
    return fmin(v - s.reg_lo, s.reg_hi - v);  // distance to the nearest face beyond which this context holds nothing
}
#endif

// Morton frame of a cloud, as the kernels need it to place a foreign point into this cloud's grid
struct FrameView {
    double ox, oy, oz;  // origin (bbox min)
    double fine_h;      // edge of the finest (21-bit) cell
};

// sort key layout of the one-pass voxel build's run records (me_vox_rows.hpp)
struct VoxPack {
    double vs;
    int min_x, min_y, min_z;   // smallest voxel index of the cloud's bounding box per axis
    int bits_y, bits_z;        // bits of the y / z index ranges (x takes what is left)
    int pos_bits;              // bits below the compact voxel key: row (i >> 6) and the run inside the row (6 bits)
    unsigned long long sentinel;  // compact key of the halo points (slab mode): above every real one
};

struct Cloud {
    // run records of the one-pass voxel build, emitted by the index build's gather when the context carries a voxel-size hint
    // (me_run_suite_from): slot keys | populations | sums, the counter block [range error, appended records]
    DevBuf vox_rec_key, vox_rec_n, vox_rec_s, vox_rec_cnt;
    bool vox_rec_valid = false;
    long long vox_rec_cap = 0;
    VoxPack vox_rec_pack{};
    bool sort_pairs_hint = false;  // the keys-only sort had to cut the sort depth and the cloud was dense: use the pair sort (me_index.hip)
    long long hint_n = 0;          // ... for a cloud of this shape only (same count, lattice depth and cell edge)
    int hint_shift = 0;
    double hint_cell_h = 0;
    long long n = 0;        // points held (slab mode: owned + halo)
    long long n_total = 0;  // points the caller passed to the upload
    SlabView slab{-1, 0, 0, 0, 0};
    DevBuf nn_unres;        // slab mode: sorted positions of the not-yet-global 1-NN results
    DevBuf slab_orig;       // slab mode, filtered upload: int32[n] position of every kept point in the uploaded array
    bool slab_identity = true;  // ... or the identity (me_upload_slab_device, no filter pass)
    long long n_unres = 0;
    bool uploaded = false;
    DevBuf xyz;  // double[n][3] original order, after the optional transform
    // Morton frame
    double origin[3] = {0, 0, 0};
    double bbox_lo[3] = {0, 0, 0}, bbox_hi[3] = {0, 0, 0};
    double cell_size_req = 0;  // cell size the caller asked for (<= 0: automatic)
    double cell_h = 0;   // radius-grid cell edge
    double fine_h = 0;   // cell_h / 2^shift
    int shift = 0;
    bool index_valid = false;
    DevBuf codes;  // uint64[n] fine Morton code of every sorted point (the points are sorted along the Hilbert curve)
    DevBuf sp;     // SPoint[n] sorted
    // sparse octree (general 1-NN path)
    OctView oct{};
    bool oct_deferred = false;  // the index is valid but its octree is still to be built (cloud_finish_octree)
    int oct_nn_shift = 0;       // level of the octree's leaves (the 1-NN grid's)
    DevBuf oct_nodes;
    DevBuf oct_pbegin;
    // cell tables: `grid` at the radius level (MME), `nn_grid` at the level whose occupied cells hold ~16 points
    // (1-NN fast path); they share storage when the two levels coincide
    GridTable grid_tab, nn_tab;
    GridView grid{}, nn_grid{};
    // the levels strictly between the 1-NN grid and the radius grid (dense clouds only: at 10^4 pts/m^2 the 1-NN cells are 2.5 cm and
    // the radius cells 10 cm): the 1-NN cascade passes what a level leaves unresolved to the next coarser one
    static constexpr int kMaxMid = 4;
    GridTable mid_tab[kMaxMid];
    GridView mid_grid[kMaxMid]{};
    int n_mid = 0;
    long long level_unique[kMortonBits + 1] = {0};  // occupied cells per Morton level
    // last NN result with this cloud as the query (sorted query order)
    DevBuf nn_d2, nn_idx, nn_list;
    int nn_ref_slot = -1;
    // voxel table (ascending key order)
    double vox_size = 0;
    long long n_vox = 0;
    bool vox_valid = false, vox_raw = false;
    bool vox_merged = false;  // the table is the cross-rank merge of partials (me_voxel_merge_device): complete on every rank
    DevBuf mme_ent, mme_val;  // last me_mme of this cloud, sorted order: entropy (0 where invalid), validity byte
    bool mme_have = false;
#ifdef ME_AB  // measurement build only (profiles/ab/me_mme7.hip): digit features of the matrix-pipe MME kernel
    DevBuf mme_feat;        // [n_chunks][80 columns][16 candidates] signed bytes
    DevBuf mme_cell_chunk;  // uint32[n_cells + 1] first chunk of every cell
    bool mme_feat_valid = false, mme_feat_usable = false;
    double mme_feat_radius = 0;
    long long mme_fx_origin[3] = {0, 0, 0};
    int mme_fx_scale = 0;
#endif
    DevBuf vox_tmp;    // build scratch (segment starts when they outgrow the shared scratch)
    DevBuf vox_key;    // uint64[V] packed key
    DevBuf vox_n;      // int32[V]
    DevBuf vox_mu;     // double[V][3]
    DevBuf vox_sigma;  // double[V][9] as stored by the reference
    DevBuf vox_entropy;
    // per-point attributes of the registration path, ORIGINAL point order (me_reg.hip)
    DevBuf normals;  // double[n][3]
    DevBuf cov;      // double[n][9] generalized-ICP covariances
    bool have_normals = false, have_cov = false;
    // FPFH features of the cloud, ORIGINAL point order, double[n][33] (me_globreg.hip); dropped with the points (cloud_finish) and normals
    DevBuf fpfh;
    bool fpfh_valid = false;
    // keep-mask of the last me_statistical_outlier / me_radius_outlier, uint8[n] in cloud order (me_outlier.hip); dropped with the points
    DevBuf outlier_keep;
    bool outlier_keep_valid = false;
    // labels (int32[n], cloud order) and cluster sizes (uint64[cluster_n]) of the last me_cluster_dbscan (me_cluster.hip); dropped with the points
    DevBuf cluster_labels, cluster_sizes;
    long long cluster_n = 0;
    bool cluster_valid = false;
    // last me_local_geometry of this cloud, SORTED order (me_localgeom.hip): eigenvalues double[n][3] (l1 >= l2 >= l3, zeros where
    // invalid), neighbour count int32[n], validity byte; dropped with the points and with the sorted order (cloud_build_index)
    DevBuf lg_eig, lg_k, lg_val;
    bool lg_have = false;
    // labels (int32[n], cloud order, -1 = no plane) and per-plane records of the last me_segment_planes (me_plane.hip); dropped with the points
    DevBuf plane_labels;
    std::vector<me_plane_record> plane_rec;
    bool plane_valid = false;
    // every me_local_geometry / me_segment_planes that completes on this cloud gets a new serial: a product of both (me_mom.hip) is
    // current only while both flags are set and both serials are the ones it was made from
    unsigned long long lg_serial = 0, plane_serial = 0;
    // axis byte per point (int8[n], cloud order, -1 = not used) of the last me_mom (me_mom.hip); dropped with the labels and the eigenvalues
    DevBuf mom_axis;
    bool mom_have = false;
    // e and c of the last me_nn_surface_error with this cloud as the query, SORTED order, -1 where the pair was not used
    // (me_surface.hip); current only while the 1-NN result is (nn_ref_slot >= 0): a new one (nn_search, set_nn_result) clears the flag
    DevBuf surf_e, surf_c;
    bool surf_have = false;
    // last me_m3c2 with this cloud as the query, SORTED order (me_m3c2.hip): the counts int32[2][n] (own, other), the moments
    // double[4][n] (S_own, Q_own, S_other, Q_other; scratch of the call), the results double[4][n] (dist, lod, var_own, var_other) and
    // the flag byte (bit 0 valid, bit 1 significant); dropped with the sorted order (cloud_build_index) and with the points of EITHER slot
    DevBuf m3_cnt, m3_mom, m3_res, m3_flags;
    bool m3c2_have = false;
    unsigned long long mom_lg_serial = 0, mom_plane_serial = 0;
    // last me_mesh_distance with this cloud as the query, SORTED order (me_mesh.hip): d2 double[n], caller's triangle index int32[n],
    // region byte, closest point double[3][n], signed distance double[n] (NaN off the face region); dropped with the sorted order
    // (cloud_build_index), with the points, and with the mesh (me_mesh_upload, me_mesh_clear)
    DevBuf mesh_d2, mesh_tri, mesh_reg, mesh_cp, mesh_sd;
    bool mesh_have = false;
    // last me_mesh_signed_distance over that result, SORTED order (me_meshsign.hip): signed distance double[n], flag byte; current only
    // while mesh_have is, and cleared by a new me_mesh_distance on the slot
    DevBuf mesh_ssd, mesh_sfl;
    bool mesh_sign_have = false;
    // component (int32[n]) and flip byte per point of the last me_orient_normals, CLOUD order (me_orient.hip); dropped when the slot's
    // normals or points are next replaced (cloud_finish, the normal producers, rotate_attributes)
    DevBuf orient_comp, orient_flip;
    bool orient_have = false;
    // rows of the last me_voxel_deformation with this cloud as the query, ascending key order (me_deform.hip): keys int32[V][3], pair
    // counts int64[V], flag bytes, the 23 pair sums double[V][23] and the fit double[V][18] (t0, u, R, e0 / e_t / e_R); current only
    // while the 1-NN result is (nn_ref_slot >= 0): a new one (nn_search, set_nn_result) clears the flag
    DevBuf dfm_keys, dfm_n, dfm_flags, dfm_sums, dfm_fit;
    long long dfm_V = 0;
    bool dfm_have = false;
    // ray id int64[n] of every point, CLOUD order, while the slot holds the result of me_mesh_scan (me_ray.hip); dropped with the points
    DevBuf scan_ray;
    bool scan_have = false;
    // last me_cloud_visibility of this cloud, SORTED order (me_ray.hip): origins that see the point int32[n], the first of them int32[n]
    // (-1: none); dropped with the sorted order (cloud_build_index), with the points, and with the mesh (me_mesh_upload, me_mesh_clear)
    DevBuf vis_n, vis_first;
    bool vis_have = false;
};

// The resident triangle mesh (me_mesh.hip): one per primary context, beside the two clouds and untouched by what happens to them.
constexpr int kMeshMaxLevels = 12;        // 8^11 leaves of 8 triangles: more than the 2^31 triangles an upload accepts
constexpr double kMeshDeltaUlps = 32.0;   // the closest point of a triangle is evaluated to within this many 2^-53 |coordinate|max
struct Mesh {
    bool have = false;
    long long nv = 0, nt = 0, n_deg = 0;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // bounding box of the referenced vertices
    double area = 0, max_abs = 0;                 // total area (= cum[nt - 1]); largest |coordinate| of a referenced vertex
    int n_levels = 0;                             // level 0 = leaves (8 consecutive sorted triangles) ... n_levels - 1 = the root
    int lv_off[kMeshMaxLevels] = {0}, lv_cnt[kMeshMaxLevels] = {0};
    DevBuf tri_in;  // double[nt][9] corner coordinates, the CALLER's triangle order (the sampler's)
    DevBuf tri_s;   // the same sorted by the Morton code of the centroid
    DevBuf orig;    // uint32[nt] caller index of every sorted triangle, bit 31 = degenerate
    DevBuf cum;     // double[nt] cumulative area, caller's order
    DevBuf boxes;   // double[nodes][6] of all levels
    DevBuf lv;      // int2[kMeshMaxLevels] (offset, count) per level
    DevBuf idx;     // int32[nt][3] the caller's vertex indices (the mesh's connectivity)
    // topology and pseudo-normals (me_meshsign.hip), built on first use, dropped with the mesh: the edge id int32[nt][3] per
    // (triangle, local edge AB BC CA), -1 for a triangle without edges; N_e double[n_edges][3] and the edge flags; N_v double[nv][3]
    // and the vertex flags; the build's counters
    bool topo_have = false;
    long long n_edges = 0;
    DevBuf eid, e_n, e_fl, v_n, v_fl, topo_cnt;
    me_mesh_topo_out topo{};
};

// The last reconstruction (me_recon.hip): one per primary context, like the mesh; held until the next me_reconstruct / me_isosurface
// or me_mesh_clear.  The node arrays are in the Morton order of the lattice frame (origin `base`, 21 bits per axis).
struct Recon {
    bool have = false, have_nodes = false;  // have_nodes: the node field is me_reconstruct's (me_isosurface keeps none)
    long long n_nodes = 0, nv = 0, nt = 0;
    long long base[3] = {0, 0, 0};
    double voxel = 0;
    DevBuf verts, vedge, tris;                          // double[nv][3], int32[nv][4], int32[nt][3]
    DevBuf node_key, node_f, node_k, node_valid, cell_ok;  // uint64[n], double[n], int32[n], uint8[n], uint8[n] (corner 0 of an active cell)
    DevBuf counters;                                    // the integer totals of a call
    DevBuf s[11];                                       // scratch of the lattice build and of the extraction
};

struct TimerRec {
    double total_ms = 0;
    long long launches = 0;
};

}  // namespace me

struct me_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // The clouds live in `own_cloud` of the PRIMARY context; a twin lane (me_twin) points at the same two objects but has
    // its own stream, scratch and timers, so that two host threads can drive independent work concurrently.
    me::Cloud own_cloud[2];
    struct CloudSet {
        me::Cloud *p[2];
        me::Cloud &operator[](int i) const { return *p[i]; }
    } cloud;
    me_ctx *twin = nullptr;  // owned by the primary context
    me::Mesh own_mesh;       // the resident mesh lives in the primary context; a twin's `mesh` points at it
    me::Mesh *mesh = &own_mesh;
    me::Recon own_recon;     // the last reconstruction, likewise
    me::Recon *recon = &own_recon;
    // called by cloud_build_index right after its radix sort has been QUEUED on the context's stream (me_run_suite_from's second lane
    // uses it to let the main lane order its MME behind the sort: me_suite.hip)
    void (*sort_hook)(void *arg, hipStream_t stream) = nullptr;
    void *sort_hook_arg = nullptr;
    // me_run_suite_from's second-lane host thread (me_suite.hip: LaneWorker), created on first use, joined by me_destroy
    void *suite_event = nullptr;  // hipEvent_t of me_run_suite_from's "sort queued" hand-over, created on first use
    void *suite_worker = nullptr;
    void (*suite_worker_free)(void *) = nullptr;
    // me_run_suite_from's second lane (a twin, whose own stream has the lowest priority): while `index_tail` is set, cloud_build_index
    // queues everything AFTER its radix sort — gather, level histogram, block counts, scans, cell tables — on `tail_stream`, which has
    // the main lane's priority, ordered by tail_event[0] (sort done -> tail) and tail_event[1] (tail done -> `stream`).  Created by
    // me::tail_stream_ensure, destroyed with the context.
    hipStream_t tail_stream = nullptr;
    void *tail_event[2] = {nullptr, nullptr};  // hipEvent_t
    bool index_tail = false;
    // Small device -> host results (sums, counts, the level histogram) go through a pinned, device-mapped MAILBOX written by a
    // one-wavefront kernel (me::mail_post / me::mail_sync, me_api.hip; round 4).  hipMemcpyAsync to pageable host memory is a blit
    // kernel of ONE 1024-thread workgroup: it needs 16 free wave slots on one CU at once, and while the other lane's k_nn_grid /
    // k_mme3 keeps every CU full that took 3 - 5.6 ms per read on the critical path (profiles/r04_timeline_two_lane.txt).
    unsigned char *mail_h = nullptr, *mail_d = nullptr;
    size_t mail_used = 0;
    struct MailItem {
        void *host;
        size_t off, bytes;
    };
    std::vector<MailItem> mail_pending;
    bool is_twin = false;
    me_ctx() {
        cloud.p[0] = &own_cloud[0];
        cloud.p[1] = &own_cloud[1];
    }
    me::DevBuf tmp[6];  // scratch
    me::DevBuf red;     // reduction partials
    void *host_pinned = nullptr;
    size_t host_pinned_bytes = 0;
    int shard_rank = 0, shard_world = 1;
    bool borrow_device_input = false;   // me_create flag ME_FLAG_BORROW_DEVICE_INPUT
    bool morton_order = false;          // me_create flag ME_FLAG_MORTON_ORDER: points sorted along the Z curve instead of the Hilbert curve
    me::SlabView slab{-1, 0, 0, 0, 0};  // applied to the next uploads
    bool defer_octree = false;          // index builds leave the octree to cloud_finish_octree (me_run_suite_from)
    double vox_hint = 0;                // > 0: index builds also emit the voxel run records for this voxel size (me_run_suite_from)
    // instrumentation
    bool timers_on = false;
    std::map<std::string, me::TimerRec> timers;
    struct Pending {
        std::string name;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
    long long nn_fallback = 0, nn_queries = 0;  // counted only while timers are on
    long long mme_pairs = 0;                     // accepted (query, neighbour) pairs of the MME launches since the last reset (timers on)
    me::DevBuf mme_pairs_buf;
    me::DevBuf mme_refine;                       // k_mme3 -> k_mme_refine: [0] count, [1 ..] sorted offsets of the thin neighbourhoods
    long long mme_refined = 0;                   // queries recomputed by k_mme_refine since the last reset (me_timer_get "mme_refined")
    me::DevBuf nn_far;                           // queries whose octree walk k_nn1 handed over to k_nn_far
    me::DevBuf nn_flags, nn_list_a, nn_list_b;   // 1-NN cascade: unresolved flags of the fine-grid pass, their ordered list, ping-pong
    me::DevBuf mme_keep_e, mme_keep_v;           // me_run_suite_from: the map's per-point MME result across its transform (mme_carry_*)
    long long mme_keep_n = -1;
    me::DevBuf outlier_tmp[2];                   // me_outlier.hip: per-point avg_dist / counts and the fallback list, kept for repeated calls
    me::DevBuf cluster_tmp[5];                   // me_cluster.hip: parent, smallest index per root, the two flag arrays, the border list
    me::DevBuf mom_tmp[3];                       // me_mom.hip: selection keys, group bytes, the small state block (histograms, ranks, results)
    me::DevBuf rs_tmp[4];                        // me_errdist.hip: the select's state block, the two compacted lists, the use bytes
    long long rs_compact[2] = {0, 0};            // ... of the last select: compactions done, entries of the last list (me_timer_get)
    long long orient_rounds = 0;                 // me_orient.hip: Boruvka rounds of the last me_orient_normals (me_timer_get "orient_rounds")
    me::DevBuf plane_tmp[7];                     // me_plane.hip: remaining flags and list, the compacted coordinates, hypotheses, scores, scalars
    me::DevBuf nn1_dbg_buf;                      // octree-walk counters (nodes opened, leaves scanned, points, max per query)
    unsigned long long *nn1_dbg() {
        if (!nn1_dbg_buf.p) {
            if (nn1_dbg_buf.ensure(128) != hipSuccess) return nullptr;
            (void) hipMemsetAsync(nn1_dbg_buf.p, 0, 128, stream);  // ordered before the kernels that count into it
        }
        return nn1_dbg_buf.as<unsigned long long>();
    }

    int fail(int code, const std::string &msg) {
        err = msg;
        return code;
    }
    void shard_range(long long n, long long &b, long long &e) const {
        b = n * shard_rank / shard_world;
        e = n * (shard_rank + 1) / shard_world;
    }
    hipEvent_t get_event();
    void timer_begin(const char *name);
    void timer_end();
    void timers_collect();
};

#define ME_CHECK(ctx, expr)                                                                             \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return (ctx)->fail(ME_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__) + " at " + \
                                               __FILE__ + ":" + std::to_string(__LINE__));              \
    } while (0)

#ifdef ME_TRACE  // debug builds: wall-clock marks on stderr (which lane, where) — to locate a stall from outside
#include <chrono>
#define ME_TRACE_POINT(ctx, what)                                                                                              \
    do {                                                                                                                       \
        std::fprintf(stderr, "[me %.3f %s] %s\n",                                                                              \
                     std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(),                \
                     (ctx)->is_twin ? "twin" : "main", what);                                                                   \
        std::fflush(stderr);                                                                                                   \
    } while (0)
#else
#define ME_TRACE_POINT(ctx, what) do { } while (0)
#endif

#define ME_TRY(expr)              \
    do {                          \
        int rc__ = (expr);        \
        if (rc__ != ME_OK) return rc__; \
    } while (0)

namespace me {

// RAII scope for a named kernel-family timer
struct TimerScope {  // (scopes do not nest: a scope that calls into another timed phase ends itself first)
    me_ctx *c;
    bool open = true;
    TimerScope(me_ctx *ctx, const char *name) : c(ctx) { c->timer_begin(name); }
    void end() {
        if (open) c->timer_end();
        open = false;
    }
    ~TimerScope() { end(); }
};

// ---- tuning constants.  Compile-time only: the library reads NOTHING from the environment (a drop-in must not change its behaviour
// with the caller's environment).  Measurement builds override them on the command line (make EXTRA=-DME_TUNE_...=v); the values
// below are the measured optima (profiles/EXPERIMENTS.md, profiles/README.md "measurement knobs").
#ifndef ME_TUNE_XCD_CHUNK
#define ME_TUNE_XCD_CHUNK 128     // virtual blocks per XCD chunk (xcd_virtual_block); a huge value = one contiguous piece per XCD
#endif
#ifndef ME_TUNE_SORT_DEPTH
#define ME_TUNE_SORT_DEPTH 2      // Morton levels below the search cell that the sort order (and the choice of the 1-NN grid) may use
#endif
#ifndef ME_TUNE_SORT_PACK
#define ME_TUNE_SORT_PACK 1       // keys-only sort of packed (key, index) words when they fit 64 bits (0: always the pair sort)
#endif
#ifndef ME_TUNE_NN_OCC
#define ME_TUNE_NN_OCC 6.0        // points per occupied cell the 1-NN grid level is chosen for (6 beats 3 and 12 on the bench scene)
#endif
#ifndef ME_TUNE_MME_LEADER_ORIGIN
#define ME_TUNE_MME_LEADER_ORIGIN 1  // k_mme3: moments accumulated about the round leader's point (staged once per candidate) instead of each lane's own query
#endif
#ifndef ME_TUNE_NN_SGPR_MASKS
#define ME_TUNE_NN_SGPR_MASKS 1   // k_nn_grid: compare masks in scalar register pairs (written-out VOP3 encodings) instead of vcc
#endif
#ifndef ME_TUNE_NN1_FAR_CAP
#define ME_TUNE_NN1_FAR_CAP 64    // octree steps after which k_nn1 hands a walk over to k_nn_far (0 = never)
#endif
#ifndef ME_TUNE_NN_FAR_LEAF
#define ME_TUNE_NN_FAR_LEAF 1024  // points a node may hold for k_nn_far to scan it whole instead of descending further
#endif
#ifndef ME_TUNE_MME_WAVES
#define ME_TUNE_MME_WAVES 8  // k_mme3: wavefronts per SIMD the kernel is compiled for (measured 3 / 4 / 6 / 8: profiles/EXPERIMENTS.md "Round 6")
#endif
#ifndef ME_TUNE_MME_REFINE_COND
#define ME_TUNE_MME_REFINE_COND 1.8e-6  // k_mme3 flags a neighbourhood whose smallest covariance eigenvalue is below ~this x cell_h^2 for k_mme_refine (0: never)
#endif
#ifndef ME_TUNE_SUITE_SORT_FIRST
#define ME_TUNE_SUITE_SORT_FIRST 1  // me_run_suite_from: the map's MME is ordered behind the ground truth's radix sort (rocPRIM's onesweep crawls under a full chip)
#endif
#ifndef ME_TUNE_VOX_MERGE_SORT
#define ME_TUNE_VOX_MERGE_SORT 1  // voxel run records sorted by rocPRIM's merge sort (plain kernels) instead of its onesweep radix sort
#endif
#ifndef ME_TUNE_VOX_ONEPASS
#define ME_TUNE_VOX_ONEPASS 1     // voxel tables from ONE pass over the sorted cloud (records about the voxel centres; 0: the three-pass build)
#endif
#ifndef ME_TUNE_SUITE_DEFER_OCTREE
#define ME_TUNE_SUITE_DEFER_OCTREE 1  // me_run_suite_from: the octrees are built after the first MME has been queued, not inside the index build
#endif
#ifndef ME_TUNE_SUITE_VOX_EARLY
#define ME_TUNE_SUITE_VOX_EARLY 1  // me_run_suite_from, second lane: voxel tables whose run records the gather has emitted are finished BEFORE the reverse search (0: after it)
#endif
#ifndef ME_TUNE_SUITE_NN_FIRST
#define ME_TUNE_SUITE_NN_FIRST 1  // me_run_suite_from, second lane: the reverse 1-NN search before the voxel tables (0: round 5's order)
#endif
#ifndef ME_TUNE_SUITE_GT_TAIL_PRIO
// me_run_suite_from, device input with MME: the ground truth's index AFTER its sort on a priority stream of the second lane, and the map's
// octree built by the second lane instead of between the two MMEs (0: round 6's schedule; 2: the second lane's reverse search starts
// as soon as the lane gets there, under the map's MME; 1: it is held until the map's MME has ended, where it started in round 6.
// Bench step 44.07 / 43.98 / 43.76 / 43.18 ms for the parent / 0 / 1 / 2: profiles/EXPERIMENTS.md "Round 7")
#define ME_TUNE_SUITE_GT_TAIL_PRIO 2
#endif
inline unsigned int xcd_chunk_setting() { return (unsigned int) ME_TUNE_XCD_CHUNK; }
// blocks of `block` threads for n items, at least one: a kernel launched for n == 0 bounds-checks its index, a zero-sized grid is a launch error
inline unsigned int blocks_of(long long n, int block = 256) { return (unsigned int) std::max<long long>(1, (n + block - 1) / block); }

// ---- me_api.hip: copies between caller (host) memory and the device ----
int copy_h2d(me_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);  // ordered on ctx->stream
int copy_d2h(me_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);  // returns when dst holds the data
// ---- me_api.hip: small results to the host without a blit kernel (see me_ctx::mail_h) ----
constexpr size_t kMailBytes = 128 * 1024;
int mail_post(me_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);  // asynchronous on ctx->stream
int mail_sync(me_ctx *ctx);                                                     // hipStreamSynchronize + delivery of what was posted
void mail_drop(me_ctx *ctx);                                                    // forget what was posted (nothing is delivered)
// ---- me_api.hip: the context's priority stream for the tail of an index build (me_ctx::tail_stream) and its two events, on first use ----
int tail_stream_ensure(me_ctx *ctx);
// ---- me_api.hip: the check of the single-GPU features: slot in range, no slab or shard mode, uploaded ----
int need_single_gpu_cloud(me_ctx *ctx, int slot, const char *who);
// The host destinations of mail_post are usually LOCALS of the posting function: if it returns before its mail_sync (a failed
// allocation or launch in between), the queued entries must not survive it — the next mail_sync on the context would copy into a
// dead stack frame.  A MailGuard in scope between the first mail_post and the mail_sync drops them on every early return.
struct MailGuard {
    me_ctx *c;
    bool armed = true;
    explicit MailGuard(me_ctx *ctx) : c(ctx) {}
    int sync() {
        armed = false;
        return mail_sync(c);
    }
    ~MailGuard() {
        if (armed) mail_drop(c);
    }
};

// ---- me_prims.hip (rocPRIM-backed primitives) ----
int sort_pairs_u64_u32(me_ctx *ctx, const unsigned long long *k_in, unsigned long long *k_out,
                       const unsigned int *v_in, unsigned int *v_out, long long n, int begin_bit, int end_bit);
int sort_pairs_merge_u64_u32(me_ctx *ctx, const unsigned long long *k_in, unsigned long long *k_out, const unsigned int *v_in,
                             unsigned int *v_out, long long n);
int exclusive_scan_u32(me_ctx *ctx, const unsigned int *in, unsigned int *out, long long n);
int exclusive_scan_u32_plain(me_ctx *ctx, const unsigned int *in, unsigned int *out, long long n);  // no decoupled lookback (in != out)
int cell_start_ranks(me_ctx *ctx, const unsigned long long *codes, long long n, int shift3, unsigned int *out);
int sort_keys_f64(me_ctx *ctx, const double *in, double *out, long long n);
int sort_keys_u64(me_ctx *ctx, const unsigned long long *in, unsigned long long *out, long long n, int begin_bit, int end_bit);
int select_flagged_u32(me_ctx *ctx, const unsigned char *flags, long long n, unsigned int *out, unsigned int *count_device);
int exclusive_scan_i32_i64(me_ctx *ctx, const int *in, long long *out, long long n);  // 64-bit prefix sums of 32-bit counts

// ---- me_index.hip ----
int cloud_upload(me_ctx *ctx, int slot, const double *src, bool src_on_device, long long n, const double *T,
                 double cell_size, bool prefiltered = false);
int cloud_build_index(me_ctx *ctx, int slot, double cell_size);
int cloud_finish_octree(me_ctx *ctx, int slot);
int cell_table_fetch(me_ctx *ctx, int slot, int which, long long *n_slots, long long *n_cells, unsigned long long *hkeys, unsigned int *hvals,
                     unsigned int *cell_start, void *entries);
int cloud_finish(me_ctx *ctx, int slot, bool bbox_ready = false);
// the two lists of "this result is current" flags that every reset site clears: what goes with the slot's sorted order (every index
// rebuild), and what goes with its points (the former included); normals and covariances stay with the caller
void drop_sorted_results(me_ctx *ctx, int slot);
void drop_point_results(me_ctx *ctx, int slot);
// the upload-time reset of a slot whose points a device-side producer has just replaced (n points, no normals), before its cloud_finish
void cloud_reset_replaced(me_ctx *ctx, int slot, long long n, double cell_size_req);
int cloud_transform(me_ctx *ctx, int slot, const double *T);
int voxel_downsample(me_ctx *ctx, int slot, double voxel_size, long long *n_out);
int voxel_downsample_into(me_ctx *src_ctx, int src_slot, me_ctx *dst_ctx, int dst_slot, double voxel_size, long long *n_out);

// ---- me_perturb.hip ----
int perturb_cloud(me_ctx *ctx, int dst_slot, int src_slot, const me_perturb_params *p, long long *n_out);
// ---- me_globreg.hip ----
int fpfh(me_ctx *ctx, int slot, const me_fpfh_params *p, double *features_host);
int fpfh_match(me_ctx *ctx, int src_slot, int ref_slot, int mutual, int32_t *corr_host, long long *n_corr);
int global_register(me_ctx *ctx, int src_slot, int ref_slot, const me_globreg_params *p, double T_out[16], me_globreg_info *info,
                    int64_t *scores);
// ---- me_outlier.hip ----
int statistical_outlier(me_ctx *ctx, int slot, int nb_neighbors, double std_ratio, double *avg_host, uint8_t *keep_host,
                        me_outlier_info *info);
int radius_outlier(me_ctx *ctx, int slot, int nb_points, double radius, int32_t *counts_host, uint8_t *keep_host, me_outlier_info *info);
int outlier_select_into(me_ctx *src_ctx, int src_slot, me_ctx *dst_ctx, int dst_slot, long long *n_out);
// ---- me_localgeom.hip ----
int local_geometry(me_ctx *ctx, int slot, double radius, int min_k, me_local_geom_out *out);
int local_geometry_fetch(me_ctx *ctx, int slot, double *eig_host, int32_t *k_host, uint8_t *valid_host);
int radius_normals(me_ctx *ctx, int slot, double radius, int min_k, const double *viewpoint, int invalid_z, me_radius_normals_out *out);
// ---- me_surface.hip ----
int nn_surface_error(me_ctx *ctx, int qslot, const me_surface_params *p, me_surface_out *out);
int nn_surface_fetch(me_ctx *ctx, int qslot, double *plane_d_host, double *cos_n_host);
// ---- me_m3c2.hip ----
int m3c2(me_ctx *ctx, int qslot, const me_m3c2_params *p, const uint8_t *core_mask_host, me_m3c2_out *out);
int m3c2_fetch(me_ctx *ctx, int qslot, double *dist_host, double *lod_host, double *var_own_host, double *var_other_host, int32_t *n_own_host,
               int32_t *n_other_host, uint8_t *flags_host);
// ---- me_mesh.hip ----
int mesh_upload(me_ctx *ctx, const double *vertices_host, long long n_vertices, const int32_t *triangles_host, long long n_triangles, const double *T);
int mesh_clear(me_ctx *ctx);
int mesh_info(me_ctx *ctx, me_mesh_info_out *out);
int mesh_distance(me_ctx *ctx, int qslot, const me_mesh_params *p, me_mesh_out *out);
int mesh_distance_fetch(me_ctx *ctx, int qslot, double *d2_host, int32_t *tri_host, uint8_t *region_host, double *closest_host,
                        double *signed_host);
int mesh_sample(me_ctx *ctx, int dst_slot, long long n_points, unsigned long long seed);
// ---- me_meshsign.hip ----
int mesh_topology(me_ctx *ctx, me_mesh_topo_out *out);
int mesh_topology_fetch(me_ctx *ctx, double *vertex_normal_host, uint8_t *vertex_flags_host, double *edge_normal_host, uint8_t *edge_flags_host);
int mesh_signed_distance(me_ctx *ctx, int qslot, const me_mesh_sign_params *p, me_mesh_sign_out *out);
int mesh_signed_fetch(me_ctx *ctx, int qslot, double *signed_host, uint8_t *flags_host);
// ---- me_ray.hip: per triangle the watertight test of Woop, Benthin and Wald in fp64, one fixed operation order (include/mapeval_hip.h);
// winner = lexicographic minimum of (t, caller index); the tree only culls what cannot be a computed hit ----
int mesh_raycast(me_ctx *ctx, const double *origins_host, const double *dirs_host, long long n_rays, double t_min, double t_max, int mode,
                 double *t_host, int32_t *tri_host, double *u_host, double *v_host, uint8_t *flags_host, me_ray_out *out);
// ray p * n_dirs + b: o = translation of pose p, d_w[k] = (R[k][0] dx + R[k][1] dy) + R[k][2] dz, closest hit with t in
// [min_range, max_range] / sqrt(dot(d_w, d_w)); hits compacted in ray order into dst_slot, then cloud_finish
int mesh_scan(me_ctx *ctx, int dst_slot, const double *poses_host, long long n_poses, const double *dirs_host, long long n_dirs,
              const me_scan_params *p, int64_t *pose_hits_host, me_scan_out *out);
int mesh_scan_fetch(me_ctx *ctx, int slot, int64_t *ray_id_host);
// point p, origin o: d = p - o, len = sqrt(dot(d, d)); seen iff min_range <= len <= max_range and (len <= tolerance or no any-hit of
// the ray (o, d) with t in [0, (len - tolerance) / len]); writes the slot's keep mask (outlier_keep)
int cloud_visibility(me_ctx *ctx, int slot, const double *origins_host, long long n_origins, const me_vis_params *p, me_vis_out *out);
int cloud_visibility_fetch(me_ctx *ctx, int slot, int32_t *n_seen_host, int32_t *first_seen_host);
// ---- me_recon.hip ----
int reconstruct(me_ctx *ctx, int slot, const me_recon_params *p, me_recon_out *out);
int isosurface(me_ctx *ctx, const int32_t *node_ijk_host, const double *f_host, const uint8_t *valid_host, long long n_nodes, double voxel,
               me_recon_out *out);
int reconstruct_fetch(me_ctx *ctx, double *vertices_host, int32_t *vertex_edge_host, int32_t *triangles_host);
int reconstruct_nodes_fetch(me_ctx *ctx, int32_t *node_ijk_host, double *f_host, int32_t *k_host, uint8_t *valid_host);
int reconstruct_install(me_ctx *ctx);
void reconstruct_drop(me_ctx *ctx);
// ---- me_orient.hip ----
int orient_normals(me_ctx *ctx, int slot, const me_orient_params *p, me_orient_out *out);
int orient_fetch(me_ctx *ctx, int slot, int32_t *component_host, uint8_t *flipped_host);
// ---- me_search.hip ----
constexpr int kSearchSortTile = 512;  // entries of a radius row that one wave sorts in LDS; longer rows are sorted in global memory
int knn_search(me_ctx *ctx, int qslot, int rslot, int k, const uint8_t *mask_host, int32_t *idx_host, double *d2_host);
int hybrid_search(me_ctx *ctx, int qslot, int rslot, double radius, int max_nn, const uint8_t *mask_host, int32_t *counts_host, int32_t *idx_host,
                  double *d2_host);
int radius_search(me_ctx *ctx, int qslot, int rslot, double radius, const uint8_t *mask_host, int64_t *offsets_host, int32_t *idx_host,
                  double *d2_host, long long capacity, int64_t *total_host);
// ---- me_plane.hip ----
int segment_planes(me_ctx *ctx, int slot, const me_plane_params *p, me_plane_record *planes_host, int32_t *labels_host, int64_t *scores_host,
                   me_plane_info *info);
int plane_fetch(me_ctx *ctx, int slot, me_plane_record *planes_host, long long capacity, long long *n_planes, int32_t *labels_host);
int plane_keep(me_ctx *ctx, int slot, int plane, int invert, uint8_t *keep_host, me_outlier_info *info);
// ---- me_mom.hip ----
int group_order_stats(me_ctx *ctx, const double *values_host, const int32_t *group_host, long long n, int n_groups, me_group_stats *out);
int mom_select_axes(const me_plane_record *planes, int n_planes, const me_mom_params *p, int32_t *dir_of_plane, me_mom_axes *axes);
int mom(me_ctx *ctx, int slot, const me_mom_params *p, me_mom_out *out);
int mom_fetch(me_ctx *ctx, int slot, int8_t *axis_host);
// ---- me_errdist.hip ----
int rank_select(me_ctx *ctx, const double *values_host, const uint8_t *use_host, long long n, const int64_t *ranks, int n_ranks,
                me_rank_stats *out);
int nn_error_distribution(me_ctx *ctx, int qslot, const me_errdist_params *p, me_errdist_out *out, int64_t *hist_host);
void fscore_finalize(long long n_within_est, long long n_est, long long n_within_gt, long long n_gt, double prf[3]);
// ---- me_cluster.hip ----
int cluster_dbscan(me_ctx *ctx, int slot, double eps, int min_points, int32_t *labels_host, int32_t *counts_host, me_cluster_info *info);
int cluster_sizes(me_ctx *ctx, int slot, int64_t *sizes_host, long long capacity, long long *n_clusters);
int cluster_keep(me_ctx *ctx, int slot, long long min_cluster_size, long long keep_largest, uint8_t *keep_host, me_outlier_info *info);

// ---- me_nn.hip ----
int nn_search(me_ctx *ctx, int qslot, int rslot);
int nn_fetch(me_ctx *ctx, int qslot, int32_t *idx, double *d2);
int nn_unresolved(me_ctx *ctx, int qslot, double *xyz_device, double *d2_device, long long capacity, long long *count);
int nn_points(me_ctx *ctx, int rslot, const double *xyz_device, long long m, double *d2_device, bool bounded, int cov_axis = 0,
              const double *cov_device = nullptr);
int nn_patch(me_ctx *ctx, int qslot, const double *d2_device, long long count);
int nn_cross_message(me_ctx *ctx, double *msg_device, long long cap, long long n_loc_est, long long n_loc_gt, long long counts[2]);
int nn_cross_answer(me_ctx *ctx, const double *gathered_device, int world, long long cap, int own_rank, int dir_mask, int axis,
                    const double *cuts_host, double halo, double *d2_device);
int nn_cross_patch(me_ctx *ctx, const double *d2_reduced_device, long long cap, int own_rank);
int icp_p2p_sums(me_ctx *ctx, int qslot, double max_distance, me_icp_sums *out);
int nn_partial(me_ctx *ctx, int qslot, double gate, int gate_mode, const double trunc[5], me_nn_partial *out);
int nn_sigma(me_ctx *ctx, int qslot, double gate, int gate_mode, const double mean[5], double sigma_num[5]);

// ---- me_reg.hip (registration_methods 1 / 2) ----
int set_normals(me_ctx *ctx, int slot, const double *normals_host);
int get_normals(me_ctx *ctx, int slot, double *normals_host);
int estimate_normals(me_ctx *ctx, int slot, int knn, double *normals_host, int32_t *knn_idx_host, double *knn_d2_host);
int gicp_covariances(me_ctx *ctx, int slot, double epsilon, double *cov_host);
int get_covariances(me_ctx *ctx, int slot, double *cov_host);
int rotate_attributes(me_ctx *ctx, int slot, const double *T);
int icp_lsq_sums(me_ctx *ctx, int qslot, int mode, double max_distance, me_icp_lsq *out);
int icp_lsq_sums_robust(me_ctx *ctx, int qslot, int mode, double max_distance, int kernel, double k, me_icp_robust *out);
int icp_information(me_ctx *ctx, int qslot, double max_distance, double *info, long long *n_corr);
// the k nearest neighbours of every point of a slot in that slot (the walk of me_estimate_normals; normals untouched): idx / d2 [n][k],
// original order, ascending by (d2, index), -1 / inf past the end.  Device buffers; queued on ctx->stream.
constexpr int kKnnMax = 40;
int knn_lists(me_ctx *ctx, int slot, int k, int *idx_device, double *d2_device);

#ifdef ME_AB  // ---- profiles/ab/me_mme7.hip (round 4's matrix-pipe MME kernel: measurement build only) ----
int mme7_prepare(me_ctx *ctx, Cloud &c, double radius, bool *usable);
int mme7_launch(me_ctx *ctx, Cloud &c, long long b, long long e, unsigned int nb, double radius, int min_k, double *ent_s,
                unsigned char *valid_s, double *part_sum, long long *part_cnt);
#endif

// ---- me_mme.hip ----
int mme_run(me_ctx *ctx, int slot, double radius, int min_k, double *entropies, uint8_t *valid, double *sum_H,
            long long *n_valid);
int mme_fetch(me_ctx *ctx, int slot, double *entropies, uint8_t *valid);
int mme_carry_out(me_ctx *ctx, int slot);  // park the slot's per-point MME result in cloud order (before a transform re-indexes it)
int mme_carry_in(me_ctx *ctx, int slot);   // ... and put it back in the new sorted order

// ---- me_dist.hip (multi-GPU pieces) ----
int halo_pack(me_ctx *ctx, const double *xyz_device, long long n, int axis, const double *cuts_host, int world, double halo,
              double *out_device, long long capacity, long long *counts_host, long long *tags_device = nullptr, long long tag_base = 0);
int voxel_rows_device(me_ctx *ctx, int slot, double voxel_size, double *rows_device, long long capacity, long long *n_rows);
int lattice_messages(me_ctx *ctx, const double *const xyz_device[2], const long long n[2], int clouds, int e0, long long *msg_device);
int lattice_plan(me_ctx *ctx, const long long *msgs_device, int world, int clouds, double halo, int e0, long long *out_host);
int lattice_histograms(me_ctx *ctx, const double *xyz_device, long long n, int e0, int *level, long long origin_bin[3], long long neg_inf[3],
                       unsigned int *hist_device);
int voxel_merge(me_ctx *ctx, int slot, double voxel_size, const double *rows_device, long long m);
int transform_points_device(me_ctx *ctx, double *xyz_device, long long n, const double *T);
int set_mme_result(me_ctx *ctx, int slot, const double *entropies, const uint8_t *valid);
int set_nn_result(me_ctx *ctx, int qslot, int rslot, const double *d2);
int slab_points(me_ctx *ctx, int slot, int64_t *orig_index, uint8_t *owned, long long capacity, long long *count);

// ---- me_render.hip ----
int render_distance(me_ctx *ctx, int qslot, double dis, double gate, int gate_mode, double *rgb, uint8_t *inlier);
int render_entropy(me_ctx *ctx, int slot, double *xyz_out, double *rgb_out, long long capacity, long long *n_valid,
                   double *min_abs_out, double *max_abs_out);

// ---- me_voxel.hip ----
int voxel_build(me_ctx *ctx, int slot, double voxel_size, bool raw);
int voxel_export(me_ctx *ctx, int slot, int32_t *keys, int32_t *npts, double *mu, double *sigma, double *entropy,
                 int64_t *n_voxels);
int awd_scs(me_ctx *ctx, double voxel_size, int min_pts, int scs_radius, double *rows, double *w_sorted,
            int64_t *n_rows, double *awd, double *scs, int64_t counts[3]);
int w2_batch(me_ctx *ctx, const double *mu1, const double *sigma1, const int32_t *n1, const double *mu2,
             const double *sigma2, const int32_t *n2, long long count, double *w);
int scs_table(me_ctx *ctx, const int32_t *keys, const double *w, long long n, int scs_radius, double *scs);
int voxel_metrics(me_ctx *ctx, int slot, double voxel_size, double gate, int gate_mode, const double trunc[5], int32_t *keys,
                  me_nn_partial *nn, double *sum_H, int64_t *n_H, int *have_mme, int64_t *n_voxels);
// the tail of a one-pass record table, shared with me_deform.hip: the fullest overflow region, and the records' segments per voxel
int vox_region_fill(me_ctx *ctx, unsigned int *cnt, unsigned int h2[2]);
int vox_record_segments(me_ctx *ctx, long long cap, const unsigned long long *rec_pos, const unsigned long long *rec_vkey, DevBuf &vkey_d,
                        DevBuf &seg_d, const unsigned int **perm, long long *n_vox);
// ---- me_deform.hip ----
int voxel_deformation(me_ctx *ctx, int qslot, double voxel_size, double max_distance, int min_pairs, double min_spread, me_deform_summary *out);
int voxel_deformation_fetch(me_ctx *ctx, int qslot, int32_t *keys, int64_t *n_pairs, uint8_t *flags, double *sums, double *t0, double *u,
                            double *R, double *e, int64_t *n_voxels);
// ---- me_voxdist.hip ----
int voxel_distances(me_ctx *ctx, const me_voxdist_params *p, int32_t *keys, int32_t *n_pop, int32_t *n_used, double *ksum, double *mmd2,
                    double *gauss, int64_t *n_rows, me_voxdist_out *out);
// ---- me_transport.hip ----
int voxel_transport(me_ctx *ctx, const me_voxtrans_params *p, const double *directions, const double *eps_schedule, int32_t *keys,
                    int32_t *n_pop, int32_t *n_used, double *sliced, double *sinkhorn, double *per_direction, double *potentials,
                    int64_t *n_rows, me_voxtrans_out *out);

// ---- shared device helpers ----
#ifdef __HIPCC__
// XCD-aware block order.  The hardware deals consecutive block ids round-robin to the 8 XCDs (each with its own L2).
// XCD x gets the chunks x, x+8, x+16, ... of `chunk` consecutive virtual blocks: neighbouring blocks (which stream
// largely the same candidates) share an L2, and every XCD sees a sample of the whole cloud.  One contiguous eighth per
// XCD (the first version) left XCDs with dense regions running long after the others had drained.
// nblocks must be a multiple of 8; the map is a bijection of [0, nblocks).
__device__ __forceinline__ unsigned int xcd_virtual_block(unsigned int bid, unsigned int nblocks, unsigned int chunk) {
    const unsigned int per = nblocks >> 3, x = bid & 7u, s = bid >> 3;
    const unsigned int full = (per / chunk) * chunk;  // slots per XCD covered by whole chunks
    if (s < full) return ((s / chunk) * 8u + x) * chunk + (s % chunk);
    const unsigned int rem = per - full;              // leftover slots: one contiguous piece per XCD
    return full * 8u + x * rem + (s - full);
}

__device__ __forceinline__ double dist2_exact(double ax, double ay, double az, double bx, double by, double bz) {
    // ((dx*dx + dy*dy) + dz*dz) without FMA contraction (file compiled with -ffp-contract=off):
    // this expression must be bit-identical to the CPU path (nanoflann L2 adaptor order).
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}
// 3-vectors, the same association: tests/_reg_ref.py and tests/_globreg_ref.py restate it
__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// block-wide sum for blockDim.x == 256 (4 waves); result valid in thread 0. `sm` holds >= 4 doubles.
__device__ __forceinline__ double block_sum_256(double v, double *sm) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    double r = 0;
    if (threadIdx.x == 0) r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    return r;
}
__device__ __forceinline__ long long block_sum_256_ll(long long v, long long *sm) {
    v = wave_sum_ll(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    long long r = 0;
    if (threadIdx.x == 0) r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    return r;
}

__device__ __forceinline__ unsigned long long spread21(unsigned long long x) {
    x &= 0x1fffffULL;
    x = (x | x << 32) & 0x1f00000000ffffULL;
    x = (x | x << 16) & 0x1f0000ff0000ffULL;
    x = (x | x << 8) & 0x100f00f00f00f00fULL;
    x = (x | x << 4) & 0x10c30c30c30c30c3ULL;
    x = (x | x << 2) & 0x1249249249249249ULL;
    return x;
}
__device__ __forceinline__ unsigned int compact21(unsigned long long x) {
    x &= 0x1249249249249249ULL;
    x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ULL;
    x = (x ^ (x >> 4)) & 0x100f00f00f00f00fULL;
    x = (x ^ (x >> 8)) & 0x1f0000ff0000ffULL;
    x = (x ^ (x >> 16)) & 0x1f00000000ffffULL;
    x = (x ^ (x >> 32)) & 0x1fffffULL;
    return (unsigned int) x;
}
__device__ __forceinline__ int readlane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int lane) {
    const unsigned int lo = (unsigned int) __builtin_amdgcn_readlane((int) (unsigned int) v, lane);
    const unsigned int hi = (unsigned int) __builtin_amdgcn_readlane((int) (unsigned int) (v >> 32), lane);
    return ((unsigned long long) hi << 32) | lo;
}

// fine (21-bit/axis) grid coordinate of a coordinate in a cloud's frame — the ONE definition every kernel uses
// (division, not reciprocal multiply: (p-o)/(h*2^-s) == ((p-o)/h)*2^s exactly, so a coarser cell is a bit prefix)
__device__ __forceinline__ double fine_coord(double x, double o, double fine_h) { return floor((x - o) / fine_h); }

__device__ __forceinline__ unsigned long long hash_u64(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}
constexpr unsigned long long kEmptyKey = ~0ULL;

__device__ __forceinline__ int hash_lookup(const unsigned long long *__restrict__ keys,
                                           const unsigned int *__restrict__ vals, unsigned int mask,
                                           unsigned long long key) {
    unsigned int s = (unsigned int) hash_u64(key) & mask;
    for (;;) {
        const unsigned long long k = keys[s];
        if (k == key) return (int) vals[s];
        if (k == kEmptyKey) return -1;
        s = (s + 1) & mask;
    }
}

// ------------------------------------------------------------------------------------------------------------
// Wave-level candidate grouping shared by the radius (MME) and 1-NN grid kernels.
//
// Every lane holds one query and its grid cell (cx,cy,cz).  The group of a round = the pending lanes whose cell is
// within Chebyshev distance 1 of the leader's (first pending lane's) cell.  Their cells span at most 3x3x3, so the
// union of their 3x3x3 neighbourhoods is the group's cell bounding box grown by one: at most 5x5x5 = 125 cells,
// each resolved by ONE hash probe (lane t takes cells t and t+64).  The caller then streams every non-empty run once
// with wave-uniform addresses and lets ALL group lanes test each candidate: compared with one stencil per distinct
// cell this shares candidate fetches between neighbouring cells and keeps the whole wave busy.
// Returns whether this lane is in the group; (rs0,rc0) / (rs1,rc1) = start/count of this lane's two runs.
// ------------------------------------------------------------------------------------------------------------
struct GroupBox {
    int x0, y0, z0, nx, ny;  // origin and x/y extent of the probed cell box (wave-uniform)
};

__device__ __forceinline__ bool wave_group_runs(bool pending, int cx, int cy, int cz, const GridView &g, int cell_lim,
                                                int lane, int &rs0, int &rc0, int &rs1, int &rc1, GroupBox *box = nullptr) {
    const unsigned long long pm = __ballot(pending);  // caller guarantees pm != 0
    const int leader = __ffsll((long long) pm) - 1;
    const int lx = readlane_i(cx, leader), ly = readlane_i(cy, leader), lz = readlane_i(cz, leader);
    const int ex = cx - lx, ey = cy - ly, ez = cz - lz;
    const bool in = pending && ex >= -1 && ex <= 1 && ey >= -1 && ey <= 1 && ez >= -1 && ez <= 1;
    const int x0 = lx - 1 - (__ballot(in && ex < 0) ? 1 : 0), x1 = lx + 1 + (__ballot(in && ex > 0) ? 1 : 0);
    const int y0 = ly - 1 - (__ballot(in && ey < 0) ? 1 : 0), y1 = ly + 1 + (__ballot(in && ey > 0) ? 1 : 0);
    const int z0 = lz - 1 - (__ballot(in && ez < 0) ? 1 : 0), z1 = lz + 1 + (__ballot(in && ez > 0) ? 1 : 0);
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1, nz = z1 - z0 + 1;
    const int n_keys = nx * ny * nz;  // <= 125
    if (box) {
        box->x0 = x0;
        box->y0 = y0;
        box->z0 = z0;
        box->nx = nx;
        box->ny = ny;
    }
    rs0 = rc0 = rs1 = rc1 = 0;
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
        const int t = lane + 64 * slot;
        if (t < n_keys) {
            const int ix = x0 + t % nx, iy = y0 + (t / nx) % ny, iz = z0 + t / (nx * ny);
            if (ix >= 0 && iy >= 0 && iz >= 0 && ix < cell_lim && iy < cell_lim && iz < cell_lim) {
                const unsigned long long key = spread21((unsigned long long) ix) | (spread21((unsigned long long) iy) << 1) |
                                               (spread21((unsigned long long) iz) << 2);
                const int ci = hash_lookup(g.hkeys, g.hvals, g.hmask, key);
                if (ci >= 0) {
                    const int s = (int) g.cell_start[ci];
                    const int c = (int) g.cell_start[ci + 1] - s;
                    if (slot == 0) {
                        rs0 = s;
                        rc0 = c;
                    } else {
                        rs1 = s;
                        rc1 = c;
                    }
                }
            }
        }
    }
    return in;
}

__device__ __forceinline__ double uniform_f64(double v) {  // a wave-uniform double, moved to a scalar register pair
    const unsigned int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double((int) hi, (int) lo);
}
// Sum over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48 all end with the total, bit-identical: the two
// additions commute) with gfx950's half-exchange permutes — v_permlane16_swap trades the odd rows of one operand for the
// even rows of the other, v_permlane32_swap the upper half for the lower half — one VALU instruction per 32 bits and
// stage, no LDS round trip.
__device__ __forceinline__ int rows4_sum_i(int v) {
    auto a = __builtin_amdgcn_permlane16_swap((unsigned int) v, (unsigned int) v, false, false);
    v = (int) a[0] + (int) a[1];
    auto b = __builtin_amdgcn_permlane32_swap((unsigned int) v, (unsigned int) v, false, false);
    return (int) b[0] + (int) b[1];
}
__device__ __forceinline__ double rows4_sum_d(double v) {
    unsigned int lo = (unsigned int) __double2loint(v), hi = (unsigned int) __double2hiint(v);
    auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    v = __hiloint2double((int) b[0], (int) a[0]) + __hiloint2double((int) b[1], (int) a[1]);
    lo = (unsigned int) __double2loint(v);
    hi = (unsigned int) __double2hiint(v);
    auto c = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto d = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double((int) d[0], (int) c[0]) + __hiloint2double((int) d[1], (int) c[1]);
}
// ---- cross-lane exchanges on the VALU (DPP) instead of the LDS pipe.  `__shfl_xor` compiles to ds_bpermute_b32: an LDS
// round trip (~100 cycles) per 32 bits and butterfly stage, and the stages depend on each other.  The patterns below are
// plain data-parallel-primitive modifiers of a v_mov: a few cycles each.
// Partner of lane i inside its group of eight, stage 0: i^1 (quad_perm [1,0,3,2]), 1: i^2 (quad_perm [2,3,0,1]),
// 2: 7-i (row_half_mirror: the other quad) — three stages leave a symmetric reduction's result in all eight lanes.
template <int STAGE>
__device__ __forceinline__ int octet_partner_i(int v) {
    constexpr int ctrl = STAGE == 0 ? 0xB1 : (STAGE == 1 ? 0x4E : 0x141);
    return __builtin_amdgcn_update_dpp(0, v, ctrl, 0xF, 0xF, true);
}
template <int STAGE>
__device__ __forceinline__ double octet_partner_d(double v) {
    return __hiloint2double(octet_partner_i<STAGE>(__double2hiint(v)), octet_partner_i<STAGE>(__double2loint(v)));
}
template <int STAGE>
__device__ __forceinline__ long long octet_partner_ll(long long v) {
    const unsigned int lo = (unsigned int) octet_partner_i<STAGE>((int) (unsigned int) v);
    const unsigned int hi = (unsigned int) octet_partner_i<STAGE>((int) (unsigned int) ((unsigned long long) v >> 32));
    return (long long) (((unsigned long long) hi << 32) | lo);
}
// wave-wide min / max of an int, returned wave-uniform (scalar): four DPP stages reduce every row of 16 lanes (i^1, i^2,
// 7-i, row_mirror 15-i), four readlanes and scalar min / max combine the rows
__device__ __forceinline__ int wave_min_i(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ int wave_max_i(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// ------------------------------------------------------------------------------------------------------------
// Wave-level cell-run table for the PER-LANE walkers.  Group = pending lanes whose cell lies within Chebyshev
// distance kGroupR of the leader's; the cell box of the group grown by one (<= 7x7x7 = 343 cells) is resolved with
// one hash probe per (lane, slot) into a wave-private LDS table `tab` (>= kGroupTab entries of {start, count}).
// Every group lane then reads the runs of its own 3x3x3 block from the table: tab[(x-x0) + nx*((y-y0) + ny*(z-z0))].
// 64 curve-consecutive points almost always form one group, so the whole wave walks its candidates together.
// ------------------------------------------------------------------------------------------------------------
constexpr int kGroupR = 2;
constexpr int kGroupTab = 343;                               // (2R+1+2H)^3 for halo H = 1
constexpr int kGroupTab2 = (2 * kGroupR + 5) * (2 * kGroupR + 5) * (2 * kGroupR + 5);  // halo H = 2: 9^3 = 729

// H = halo in cells: 1 when the cell edge covers the search radius, 2 for half-radius cells (5x5x5 stencil).
// CULL: a cell of the box is kept only when it lies within Chebyshev distance H of the cell of SOME group lane (the box is
// the bounding box of the group's cells grown by H: when the cells of 64 curve-consecutive queries do not fill their
// bounding box — an L, a diagonal, a staircase — whole runs of it are adjacent to nobody, and every
// candidate of such a run would be tested by 64 lanes for nothing).  Per (y,z) row of the box the group lanes OR their x
// position into a bit mask (LDS atomics), a row's mask is then dilated over the 3x3 neighbouring rows and by one bit in x:
// a few dozen LDS operations per round against 64 x (9..19) VALU operations per candidate saved.  `rows` = 2 x 49 ints.
// `tcell` (optional) receives the box-relative cell coordinates of every table slot, packed x | y << 3 | z << 6.
// R: Chebyshev radius (in cells) of a group around its leader — kGroupR for the 64-query kernels, 1 for the 16-query
// passes of the MME kernel (a (2R+1+2H)^3 = 125-entry table).
// `tabc` / `cell_aux` (optional, both or neither): tabc[slot] = cell_aux[cell index] for every non-empty slot — a second per-cell
// array looked up with the same probe (the matrix-pipe MME kernel keeps the first feature chunk of every cell there).
// ENT (the two stream kernels, k_mme3 and k_nn_grid; needs H = 1, R <= 2, CULL, no tabc): the same table, slot for slot — same box, same
// slot order t = tx + nx * (ty + ny * tz), same runs — from fewer vector instructions.  What a slot cost before (two integer divisions and
// a modulo by the box extents, three spread21 of 64-bit values, six bounds compares, then hkeys[s] -> hvals[s] -> cell_start[ci],
// cell_start[ci + 1]) is moved to where it is paid once per ROUND or not at all:
//   * t / nx and q / ny are multiply-shifts with ceil(2^14 / n), n <= 7 (exact for every t < 5461: recip14_exact below);
//   * the lanes that dilate the cull's row masks (one per (ty, tz) row of the box, <= 49) also store their row's part of the key,
//     spread21(y) << 1 | spread21(z) << 2, and clear the mask bits of cells outside the lattice (the whole row when y or z is);
//     nx lanes store spread21(x).  A slot's key is then two LDS reads and an OR, its bounds test the cull bit it tested anyway;
//   * the probe reads GridView::hent: one 16-byte load per slot gives key, start and count.
// PRECONDITION of ENT: the cell (cx, cy, cz) of every PENDING lane lies inside the lattice, 0 <= c < cell_lim per axis (both callers
// derive it from a code of the grid or skip queries outside it), so that x0 >= -1 and x0 + nx <= cell_lim + 1 and the shifts of the
// bounds mask are in range; the other path tolerates cells outside the lattice through its per-slot compares, this one does not.
// `rows` must hold kGroupRowsEnt ints.  hash_u64 stays (it decides where every cell lives): its two 64 x 64 multiplies by constants
// compile to v_mul_lo_u32 / v_mul_hi_u32 / v_mad_u64_u32 chains of three to four instructions each.
__host__ __device__ constexpr unsigned int recip14(int n) {  // ceil(2^14 / n), 1 <= n <= 7, from two packed constants (scalar shifts, no table)
    return (unsigned int) (((n < 4 ? 0x1556200040000000ULL : 0x09250AAB0CCD1000ULL) >> (16 * (n & 3))) & 0xffffULL);
}
constexpr bool recip14_exact() {
    for (int n = 1; n <= 7; ++n)
        for (unsigned int t = 0; t < 5461; ++t)
            if (((t * recip14(n)) >> 14) != t / (unsigned int) n) return false;
    return true;
}
static_assert(recip14_exact(), "t / n as (t * recip14(n)) >> 14");
// spread21 from two 32-bit halves (bits 0..9 and 10..20): the same value from 32-bit shifts and masks, a third of the instructions and
// half the registers of the 64-bit ladder
__host__ __device__ constexpr unsigned int spread11_32(unsigned int x) {  // bit i of the low 11 -> bit 3 i
    x = (x | x << 16) & 0x070000ffu;
    x = (x | x << 8) & 0x0700f00fu;
    x = (x | x << 4) & 0x430c30c3u;
    x = (x | x << 2) & 0x49249249u;
    return x;
}
__host__ __device__ constexpr unsigned long long spread21_halves(unsigned int x) {
    return (unsigned long long) spread11_32(x & 0x3ffu) | ((unsigned long long) spread11_32((x >> 10) & 0x7ffu) << 30);
}
constexpr unsigned long long spread21_ladder(unsigned long long x) {  // (spread21 above, as a constant expression)
    x &= 0x1fffffULL;
    x = (x | x << 32) & 0x1f00000000ffffULL;
    x = (x | x << 16) & 0x1f0000ff0000ffULL;
    x = (x | x << 8) & 0x100f00f00f00f00fULL;
    x = (x | x << 4) & 0x10c30c30c30c30c3ULL;
    x = (x | x << 2) & 0x1249249249249249ULL;
    return x;
}
constexpr bool spread21_halves_exact() {  // every single bit, every run of ones from bit 0 and to bit 20, and a stride through the rest
    for (unsigned int i = 0; i < 21; ++i) {
        const unsigned int a = 1u << i, b = (2u << i) - 1u, c = 0x1fffffu & ~(a - 1u);
        if (spread21_halves(a) != spread21_ladder(a) || spread21_halves(b) != spread21_ladder(b) || spread21_halves(c) != spread21_ladder(c)) return false;
    }
    for (unsigned int x = 0; x < 0x200000u; x += 4099u)
        if (spread21_halves(x) != spread21_ladder(x)) return false;
    return true;
}
static_assert(spread21_halves_exact(), "spread21 from 32-bit halves");
constexpr int kGroupRowsEnt = 240;  // LDS ints per wave with ENT: the 128 of the cull, 49 row keys and 7 x keys of 8 bytes
template <int H = 1, bool CULL = false, int R = kGroupR, bool MLP = false, bool ENT = false>
__device__ __forceinline__ bool wave_group_table(bool pending, int cx, int cy, int cz, const GridView &g, int cell_lim,
                                                 int lane, int2 *tab, GroupBox &box, int *n_keys_out = nullptr,
                                                 unsigned int *rows = nullptr, unsigned short *tcell = nullptr,
                                                 unsigned int *tabc = nullptr, const unsigned int *cell_aux = nullptr,
                                                 int *leader_out = nullptr) {
    const unsigned long long pm = __ballot(pending);  // caller guarantees pm != 0
#ifdef ME_LEADER_FIRST
    const int leader = __ffsll((long long) pm) - 1;
#else
    // The leader is the MIDDLE pending lane, not the first: the lanes hold curve-consecutive points, the first pending lane
    // sits at one end of the stretch of space they cover and its Chebyshev ball reaches half as far into it.
    const int rank = __popcll(pm & ((1ULL << lane) - 1ULL));
    const int n_pending = __popcll(pm);
    int leader = __ffsll((long long) __ballot(pending && rank == (n_pending >> 1))) - 1;
#ifndef ME_LEADER_MIDDLE
    // Round 4: when the middle lane's group does not hold every pending lane, the lanes at the quartiles of the pending stretch
    // are tried as well — ranks k/6 of it — and the leader whose group is the largest wins (a few ballots; a round costs thousands of
    // instructions).
    {
        auto group_size = [&](int l) {
            const int ax = readlane_i(cx, l), ay = readlane_i(cy, l), az = readlane_i(cz, l);
            const int ux = cx - ax, uy = cy - ay, uz = cz - az;
            return __popcll(__ballot(pending && ux >= -R && ux <= R && uy >= -R && uy <= R && uz >= -R && uz <= R));
        };
        int best = group_size(leader);
        if (best < n_pending && n_pending >= 8) {
#pragma unroll
            for (int c = 1; c <= 5; ++c) {
                if (c == 3) continue;  // (the middle: tried already)
                const int l = __ffsll((long long) __ballot(pending && rank == ((c * n_pending) / 6))) - 1;
                const int b = group_size(l);
                if (b > best) {
                    best = b;
                    leader = l;
                }
            }
        }
    }
#endif
#endif
    if (leader_out) *leader_out = leader;
    const int lx = readlane_i(cx, leader), ly = readlane_i(cy, leader), lz = readlane_i(cz, leader);
    const int ex = cx - lx, ey = cy - ly, ez = cz - lz;
    const bool in = pending && ex >= -R && ex <= R && ey >= -R && ey <= R && ez >= -R && ez <= R;
    // (readfirstlane: the butterfly leaves the same value in every lane, but only this tells the compiler so — without it the
    // box, the table size and everything the callers derive from them live in vector registers and loops over them diverge)
    const int x0 = __builtin_amdgcn_readfirstlane(wave_min_i(in ? cx : lx)) - H;
    const int x1 = __builtin_amdgcn_readfirstlane(wave_max_i(in ? cx : lx)) + H;
    const int y0 = __builtin_amdgcn_readfirstlane(wave_min_i(in ? cy : ly)) - H;
    const int y1 = __builtin_amdgcn_readfirstlane(wave_max_i(in ? cy : ly)) + H;
    const int z0 = __builtin_amdgcn_readfirstlane(wave_min_i(in ? cz : lz)) - H;
    const int z1 = __builtin_amdgcn_readfirstlane(wave_max_i(in ? cz : lz)) + H;
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1, nz = z1 - z0 + 1;
    const int n_keys = nx * ny * nz;  // <= (2R+1+2H)^3
    if (n_keys_out) *n_keys_out = n_keys;
    box.x0 = x0;
    box.y0 = y0;
    box.z0 = z0;
    box.nx = nx;
    box.ny = ny;
    static_assert(!ENT || (H == 1 && R <= 2 && CULL && !MLP), "ENT: the <= 7 x 7 x 7 box of the stream kernels, with the cull");
    const unsigned int mx = ENT ? recip14(nx) : 0u, my = ENT ? recip14(ny) : 0u;  // (scalar)
    unsigned long long *ykey = ENT ? reinterpret_cast<unsigned long long *>(rows + 128) : nullptr, *xkey = ENT ? ykey + 49 : nullptr;
    if (CULL) {
        const int n_rows = ny * nz;  // <= 49 (H = 1)
        if (lane < n_rows) rows[lane] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (in) atomicOr(&rows[(cy - y0) + ny * (cz - z0)], 1u << (cx - x0));
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < n_rows) {
            const int rz = ENT ? (int) (((unsigned int) lane * my) >> 14) : lane / ny, ry = lane - rz * ny;
            unsigned int m = 0;
            for (int dz = -H; dz <= H; ++dz)
                for (int dy = -H; dy <= H; ++dy) {
                    const int yy = ry + dy, zz = rz + dz;
                    if (yy >= 0 && yy < ny && zz >= 0 && zz < nz) m |= rows[yy + ny * zz];
                }
            unsigned int d = m;
#pragma unroll
            for (int s = 1; s <= H; ++s) d |= (m << s) | (m >> s);
            if (ENT) {
                // cells outside the lattice [0, cell_lim)^3 are dropped here, once per row, not per slot: x by a wave-uniform bit mask
                // (x0 >= -1 and x0 + nx <= cell_lim + 1: both shifts are in range), y and z by the row
                const int iy = y0 + ry, iz = z0 + rz;
                const unsigned int okx = ((1u << (cell_lim - x0 < nx ? cell_lim - x0 : nx)) - 1u) & ~((1u << (x0 < 0 ? -x0 : 0)) - 1u);
                d = (iy >= 0 && iy < cell_lim && iz >= 0 && iz < cell_lim) ? d & okx : 0u;
                ykey[lane] = (spread21_halves((unsigned int) iy & 0x1fffffu) << 1) | (spread21_halves((unsigned int) iz & 0x1fffffu) << 2);
            }
            rows[64 + lane] = d;
        }
        if (ENT && lane < nx) xkey[lane] = spread21_halves((unsigned int) (x0 + lane) & 0x1fffffu);  // (a column outside the lattice: never read)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (MLP) {
        // Memory-level parallelism for kernels that run few waves per SIMD: the probes of ALL table slots of a lane are issued
        // before any is waited for (the plain loop below is four dependent round trips per 64 slots, one batch after the other).
        constexpr int NIT = ((2 * R + 1 + 2 * H) * (2 * R + 1 + 2 * H) * (2 * R + 1 + 2 * H) + 63) / 64;
        unsigned long long key[NIT], got[NIT];
        unsigned int slot[NIT];
        bool want[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int t = lane + 64 * i;
            const int tx = t % nx, ty = (t / nx) % ny, tz = t / (nx * ny);
            const int ix = x0 + tx, iy = y0 + ty, iz = z0 + tz;
            want[i] = t < n_keys && ix >= 0 && iy >= 0 && iz >= 0 && ix < cell_lim && iy < cell_lim && iz < cell_lim;
            if (CULL) want[i] = want[i] && ((rows[64 + (t < n_keys ? ty + ny * tz : 0)] >> tx) & 1u);
            key[i] = spread21((unsigned long long) ix) | (spread21((unsigned long long) iy) << 1) | (spread21((unsigned long long) iz) << 2);
            slot[i] = (unsigned int) hash_u64(key[i]) & g.hmask;
            got[i] = kEmptyKey;
            if (tcell && t < n_keys) tcell[t] = (unsigned short) (tx | (ty << 3) | (tz << 6));
        }
#pragma unroll
        for (int i = 0; i < NIT; ++i)
            if (want[i]) got[i] = g.hkeys[slot[i]];
        int ci[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            // (collisions: linear probing, rare)
            while (want[i] && got[i] != key[i] && got[i] != kEmptyKey) {
                slot[i] = (slot[i] + 1) & g.hmask;
                got[i] = g.hkeys[slot[i]];
            }
            want[i] = want[i] && got[i] == key[i];
            ci[i] = 0;
        }
#pragma unroll
        for (int i = 0; i < NIT; ++i)
            if (want[i]) ci[i] = (int) g.hvals[slot[i]];
        unsigned int cs0[NIT], cs1[NIT], ax[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            cs0[i] = cs1[i] = ax[i] = 0;
            if (want[i]) {
                cs0[i] = g.cell_start[ci[i]];
                cs1[i] = g.cell_start[ci[i] + 1];
                if (tabc) ax[i] = cell_aux[ci[i]];
            }
        }
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int t = lane + 64 * i;
            if (t < n_keys) {
                tab[t] = make_int2((int) cs0[i], (int) (cs1[i] - cs0[i]));
                if (tabc) tabc[t] = ax[i];
            }
        }
    } else if (ENT) {
        for (int t = lane; t < n_keys; t += 64) {
            const unsigned int q = ((unsigned int) t * mx) >> 14, tx = (unsigned int) t - q * (unsigned int) nx;  // q = ty + ny * tz: the slot's row
            int2 run = make_int2(0, 0);
            if ((rows[64 + q] >> tx) & 1u) {
                const unsigned long long key = ykey[q] | xkey[tx];
                unsigned int s = (unsigned int) hash_u64(key) & g.hmask;
                for (;;) {  // (collisions: linear probing, rare)
                    uint4 e = *reinterpret_cast<const uint4 *>(g.hent + s);
                    asm volatile("" : "+v"(e.x), "+v"(e.y), "+v"(e.z), "+v"(e.w));  // (ONE 16-byte load, not the key first and the run after it)
                    const unsigned long long k = ((unsigned long long) e.y << 32) | e.x;
                    if (k == key) {
                        run = make_int2((int) e.z, (int) e.w);
                        break;
                    }
                    if (k == kEmptyKey) break;
                    s = (s + 1) & g.hmask;
                }
            }
            tab[t] = run;
            if (tcell) {
                const unsigned int tz = (q * my) >> 14, ty = q - tz * (unsigned int) ny;
                tcell[t] = (unsigned short) (tx | (ty << 3) | (tz << 6));
            }
        }
    } else
    for (int t = lane; t < n_keys; t += 64) {
        const int tx = t % nx, ty = (t / nx) % ny, tz = t / (nx * ny);
        const int ix = x0 + tx, iy = y0 + ty, iz = z0 + tz;
        int2 run = make_int2(0, 0);
        unsigned int aux = 0;
        bool want = ix >= 0 && iy >= 0 && iz >= 0 && ix < cell_lim && iy < cell_lim && iz < cell_lim;
        if (CULL) want = want && ((rows[64 + ty + ny * tz] >> tx) & 1u);
        if (want) {
            const unsigned long long key = spread21((unsigned long long) ix) | (spread21((unsigned long long) iy) << 1) |
                                           (spread21((unsigned long long) iz) << 2);
            const int ci = hash_lookup(g.hkeys, g.hvals, g.hmask, key);
            if (ci >= 0) {
                run.x = (int) g.cell_start[ci];
                run.y = (int) g.cell_start[ci + 1] - run.x;
                if (tabc) aux = cell_aux[ci];
            }
        }
        tab[t] = run;
        if (tabc) tabc[t] = aux;
        if (tcell) tcell[t] = (unsigned short) (tx | (ty << 3) | (tz << 6));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return in;
}
constexpr int kGroupRows = 128;  // LDS ints per wave for the CULL row masks (64 raw + 64 dilated)

// Calls f(begin, end, slot) once per non-empty run of the wave's table, with WAVE-UNIFORM arguments (so that a loop over
// [begin, end) fetches candidates with scalar loads and all lanes test the same candidate); slot = its table index.
// MERGE: consecutive table slots whose runs are contiguous in the sorted array (the curve visits cell x + 1 right after
// cell x) are handed over as ONE run — with 6-point cells the per-run set-up of the 1-NN grid kernel (staging a tile,
// two barriers, the tail of the group-of-four loop) costs more than ranking the run's candidates.
template <bool MERGE = false, class F>
__device__ __forceinline__ void wave_for_each_run(const int2 *tab, int n_keys, int lane, F &&f) {
    for (int base = 0; base < n_keys; base += 64) {
        const int t = base + lane;
        const int cnt = (t < n_keys) ? tab[t].y : 0;
        unsigned long long m = __ballot(cnt > 0);
        while (m) {
            const int n = __ffsll((long long) m) - 1;
            m &= m - 1;
            const int2 run = tab[base + n];
            const int cs = __builtin_amdgcn_readfirstlane(run.x);
            int cc = __builtin_amdgcn_readfirstlane(run.y);
            if (MERGE) {
                while (m) {
                    const int n2 = __ffsll((long long) m) - 1;
                    const int2 nx = tab[base + n2];
                    if (__builtin_amdgcn_readfirstlane(nx.x) != cs + cc) break;
                    cc += __builtin_amdgcn_readfirstlane(nx.y);
                    m &= m - 1;
                }
            }
            f(cs, cs + cc, base + n);
        }
    }
}

// inclusive prefix sum over the 64 lanes of a wave: four DPP row shifts (zero fill) sum every row of 16 lanes, three readlanes and
// scalar additions give the rows their bases; *total (wave-uniform, scalar) = the sum over all lanes
__device__ __forceinline__ int wave_incl_scan_i(int v, int lane, int *total) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);  // row_shr:8
    const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = t0 + __builtin_amdgcn_readlane(v, 31), t2 = t1 + __builtin_amdgcn_readlane(v, 47);
    *total = t2 + __builtin_amdgcn_readlane(v, 63);
    return v + (lane < 32 ? (lane < 16 ? 0 : t0) : (lane < 48 ? t1 : t2));
}

// The round's table as a RUN LIST, in place: the non-empty slots of tab[0 .. n_keys) compacted in slot order — the order in which
// wave_for_each_run hands them out — into tab[i] = {start of run i in the sorted array, offset of run i in the round's candidate
// stream} (an exclusive prefix of the counts), i < *n_runs, closed by tab[*n_runs] = {0, stream length}: `tab` holds kGroupTab + 1
// entries.  Batch by batch: all 64 slots of a batch are read before any is written, and the writes go to indices no higher than the
// slots read so far.  Returns the stream's length; it and *n_runs are wave-uniform (scalar).
__device__ __forceinline__ int wave_run_list(int2 *tab, int n_keys, int lane, int *n_runs) {
    int nr = 0, total = 0;
    for (int base = 0; base < n_keys; base += 64) {
        const int t = base + lane;
        int2 run = make_int2(0, 0);
        if (t < n_keys) run = tab[t];
        const unsigned long long m = __ballot(run.y > 0);
        int batch = 0;
        const int incl = wave_incl_scan_i(run.y, lane, &batch);  // (empty and culled slots count 0)
        const int rank = (int) __builtin_amdgcn_mbcnt_hi((unsigned int) (m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int) m, 0u));
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (run.y > 0) tab[nr + rank] = make_int2(run.x, total + incl - run.y);  // nr + rank <= t
        nr += __popcll(m);
        total += batch;
    }
    if (lane == 0) tab[nr] = make_int2(0, total);  // nr <= n_keys <= kGroupTab
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    *n_runs = nr;
    return total;
}
#endif

}  // namespace me
