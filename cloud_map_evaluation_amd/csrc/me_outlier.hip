// me_outlier.hip — Open3D's PointCloud::RemoveStatisticalOutlier / RemoveRadiusOutlier on a resident cloud.  DESIGN.md section 4.8.
//   k_knn_mean     per point: the mean distance to its k nearest points of the same cloud (itself included), distances only.  A wave
//                  streams the runs of its group's cell box (wave_group_table) through LDS, every lane keeps its k smallest d2 in
//                  registers; a lane is settled when its k-th d2 lies inside its own 3x3x3 block.  The grid level is the finest
//                  table of the index whose occupied cells hold >= ME_TUNE_KNN_MEAN_OCC x k points      (me_statistical_outlier, "outlier")
//   k_knn_mean_walk  what the grid pass leaves (isolated points, n < k): the exact nearest-first octree walk of me_oct_walk.hpp
//                  (the one k_knn_normals uses), distances only                                                             ("outlier")
//   k_sor_partials / k_sor_final  mean and std in fp64: block partials in point order, then one block — no float atomics
//   k_radius_count per point: the points with d2 < r^2 in the 27-cell stencil of the radius grid (cell >= r), exact fp64
//                                                                                                  (me_radius_outlier, "outlier")
//   k_keep_gather  the kept points (and normals) in cloud order, after a stable select of the mask  (me_outlier_select_into, "outlier_select")
// The per-point results and the mask are in cloud (original) order.  The file is compiled with -ffp-contract=off: tests/_outlier_ref.py
// restates the arithmetic.
#include <algorithm>
#include <cmath>
#include <utility>

#include "me_internal.hpp"
#include "me_oct_walk.hpp"
#include "me_wave_stream.hpp"

#ifndef ME_TUNE_KNN_MEAN_OCC
#define ME_TUNE_KNN_MEAN_OCC 1.5  // k_knn_mean: points per occupied cell of the grid level, per neighbour asked for
#endif

namespace me {

namespace {

// v_min_f64 / v_max_f64 without the NaN canonicalisation fmin() / fmax() carry (squared distances are never NaN)
__device__ __forceinline__ double min_raw(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double max_raw(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// The k smallest squared distances seen, in registers: KC slots ascending, the first KC - k held at -inf (never displaced), so the
// k-th smallest is always the last slot — a compile-time index (no scratch).  An insertion is one min / max pass over the slots.
template <int KC>
struct TopK {
    double a[KC];
    __device__ __forceinline__ void init(int k) {
#pragma unroll
        for (int j = 0; j < KC; ++j) a[j] = j < KC - k ? -INFINITY : INFINITY;
    }
    __device__ __forceinline__ double worst() const { return a[KC - 1]; }
    __device__ __forceinline__ void push(double d) {
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const double lo = min_raw(a[j], d), hi = max_raw(a[j], d);
            a[j] = lo;
            d = hi;
        }
    }
    // avg_i: sqrt(d2) summed in ascending d2 order from 0, divided by the neighbour count (min(n, k))
    __device__ __forceinline__ double mean() const {
        double s = 0.0;
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const double v = a[j];
            if (v >= 0.0 && v < INFINITY) {
                s += sqrt(v);
                ++cnt;
            }
        }
        return cnt ? s / (double) cnt : 0.0;
    }
};

// ---- statistical: grid pass ----
// Settled when the k-th smallest d2 is below the squared distance from the query to the faces of its own 3x3x3 block, less 2^-20
// of a cell edge (a point outside the block is at least that far: its cell index came from a floor of the same coordinates).
// Every other query goes to `list` (sorted positions) for the octree walk.
template <int KC>
__global__ void __launch_bounds__(256)
k_knn_mean(const SPoint *__restrict__ sp, const unsigned long long *__restrict__ codes, long long n, GridView g, FrameView fr, int k,
           double *__restrict__ avg, unsigned int *__restrict__ list, unsigned int *__restrict__ list_count) {
    __shared__ WaveTile s_tile[4];
    __shared__ int2 s_tab[4][kGroupTab + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const StreamQuery q = stream_query(sp, codes, i, n, g.shift);
    TopK<KC> t;
    t.init(k);
    wave_stream(q.active, q.cx, q.cy, q.cz, sp, g, lane, s_tab[w], &s_tile[w], [&](double px, double py, double pz, int, int) {
        const double d = dist2_exact(q.qx, q.qy, q.qz, px, py, pz);
        if (d < t.worst()) t.push(d);
    });
    if (!q.active) return;
    const double hs = ldexp(fr.fine_h, g.shift);
    const double bx = fmin(q.qx - (fr.ox + (double) (q.cx - 1) * hs), (fr.ox + (double) (q.cx + 2) * hs) - q.qx);
    const double by = fmin(q.qy - (fr.oy + (double) (q.cy - 1) * hs), (fr.oy + (double) (q.cy + 2) * hs) - q.qy);
    const double bz = fmin(q.qz - (fr.oz + (double) (q.cz - 1) * hs), (fr.oz + (double) (q.cz + 2) * hs) - q.qz);
    const double bd = fmin(fmin(bx, by), bz) - hs * 0x1p-20;
    if (bd > 0.0 && t.worst() < bd * bd) {
        avg[sp[i].idx] = t.mean();
    } else {
        const unsigned int pos = atomicAdd(list_count, 1u);
        list[pos] = (unsigned int) i;
    }
}

// ---- statistical: the exact walk for the listed queries (oct_walk_nearest, me_oct_walk.hpp; a box whose bound is not below the
// k-th d2 cannot change the k smallest distances, so ties need no index rule: < where k_knn_normals admits with <=) ----
constexpr int kWalkBlock = 128;
template <int KC>
__global__ void __launch_bounds__(kWalkBlock)
k_knn_mean_walk(const SPoint *__restrict__ sp, OctView oct, int k, const unsigned int *__restrict__ list,
                const unsigned int *__restrict__ list_count, double *__restrict__ avg) {
    __shared__ long long s_off[kMaxLevels];
    if (threadIdx.x < kMaxLevels) s_off[threadIdx.x] = oct.off[threadIdx.x];
    __syncthreads();
    const unsigned int n_list = *list_count;
    const ONode *__restrict__ nodes = oct.nodes;
    const int L = oct.n_levels - 1;
    for (unsigned int t = blockIdx.x * kWalkBlock + threadIdx.x; t < n_list; t += gridDim.x * kWalkBlock) {
        const SPoint q = sp[list[t]];
        const double qx = q.x, qy = q.y, qz = q.z;
        TopK<KC> top;
        top.init(k);
        auto scan_leaf = [&](long long leaf) {
            const long long jb = nodes[leaf].begin, je = nodes[leaf + 1].begin;
            for (long long j = jb; j < je; ++j) {
                const SPoint p = sp[j];
                const double d = dist2_exact(qx, qy, qz, p.x, p.y, p.z);
                if (d < top.worst()) top.push(d);
            }
        };
        oct_walk_nearest(nodes, s_off, L, qx, qy, qz, [&](double lb) { return lb < top.worst(); }, scan_leaf);
        avg[q.idx] = top.mean();
    }
}

// ---- statistical: mean and std.  Block b sums the points [b * per, (b + 1) * per) (thread t: t, t + 256, ... in order), the
// partials are added by one block in the same pattern: a fixed order, bit-identical from run to run.
// PASS 0: sum of avg_i > 0;  PASS 1: sum of (avg_i - mean)^2 over avg_i > 0 (stats[0] = mean) ----
template <int PASS>
__global__ void __launch_bounds__(256)
k_sor_partials(const double *__restrict__ avg, long long n, long long per, const double *__restrict__ stats, double *__restrict__ part) {
    __shared__ double sm[4];
    const double mean = PASS ? stats[0] : 0.0;
    const long long b = (long long) blockIdx.x * per, e = b + per < n ? b + per : n;
    double s = 0.0;
    for (long long i = b + threadIdx.x; i < e; i += 256) {
        const double v = avg[i];
        if (v > 0.0) {
            if (PASS == 0) {
                s += v;
            } else {
                const double d = v - mean;
                s += d * d;
            }
        }
    }
    const double r = block_sum_256(s, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// stats: [0] mean = sum / n (Open3D divides by every point), [1] std = sqrt(sum / (n - 1)), [2] threshold = mean + ratio std
template <int PASS>
__global__ void __launch_bounds__(256)
k_sor_final(const double *__restrict__ part, int nb, long long n, double ratio, double *__restrict__ stats) {
    __shared__ double sm[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
    const double r = block_sum_256(s, sm);
    if (threadIdx.x == 0) {
        if (PASS == 0) {
            stats[0] = r / (double) n;
        } else {
            const double sd = sqrt(r / (double) (n - 1));
            stats[1] = sd;
            stats[2] = stats[0] + ratio * sd;
        }
    }
}

__global__ void __launch_bounds__(256)
k_sor_mask(const double *__restrict__ avg, long long n, const double *__restrict__ stats, unsigned char *__restrict__ keep,
           unsigned long long *__restrict__ kept) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    bool k = false;
    if (i < n) {
        const double v = avg[i], thr = stats[2];
        k = v > 0.0 && v < thr;  // (a NaN threshold keeps nothing)
        keep[i] = k ? 1 : 0;
    }
    const int c = __syncthreads_count(k);  // (one counter atomic per block: per-wave adds to one address cost 9 ms at 50 M points)
    if (threadIdx.x == 0 && c) atomicAdd(kept, (unsigned long long) c);
}

// ---- radius: the points with d2 < r^2 (strict, the library's radius convention), the query itself included ----
__global__ void __launch_bounds__(256)
k_radius_count(const SPoint *__restrict__ sp, const unsigned long long *__restrict__ codes, long long n, GridView g, double r2,
               int nb_points, int *__restrict__ counts, unsigned char *__restrict__ keep, unsigned long long *__restrict__ kept) {
    __shared__ WaveTile s_tile[4];
    __shared__ int2 s_tab[4][kGroupTab + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const StreamQuery q = stream_query(sp, codes, i, n, g.shift);
    int cnt = 0;
    wave_stream(q.active, q.cx, q.cy, q.cz, sp, g, lane, s_tab[w], &s_tile[w], [&](double px, double py, double pz, int, int) {
        cnt += dist2_exact(q.qx, q.qy, q.qz, px, py, pz) < r2 ? 1 : 0;
    });
    bool k = false;
    if (q.active) {
        const long long qi = sp[i].idx;
        counts[qi] = cnt;
        k = cnt > nb_points;
        keep[qi] = k ? 1 : 0;
    }
    const int c = __syncthreads_count(k);
    if (threadIdx.x == 0 && c) atomicAdd(kept, (unsigned long long) c);
}

// ---- selection: the kept points (and their normals) in cloud order ----
__global__ void __launch_bounds__(256)
k_keep_gather(const unsigned int *__restrict__ idx, long long m, const double *__restrict__ xyz, const double *__restrict__ nrm,
              double *__restrict__ xyz_out, double *__restrict__ nrm_out) {
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const long long j = idx[t];
#pragma unroll
    for (int d = 0; d < 3; ++d) xyz_out[3 * t + d] = xyz[3 * j + d];
    if (nrm) {
#pragma unroll
        for (int d = 0; d < 3; ++d) nrm_out[3 * t + d] = nrm[3 * j + d];
    }
}

// the finest cell table of the index whose occupied cells hold >= ME_TUNE_KNN_MEAN_OCC x k points on average (the radius grid when
// none does): its 3x3x3 block then usually holds the k nearest points of a surface point
const GridView &knn_mean_grid(const Cloud &c, int k) {
    const double want = ME_TUNE_KNN_MEAN_OCC * (double) k;
    auto occ = [&](const GridView &g) { return (double) c.n / (double) std::max<long long>(1, c.level_unique[g.shift]); };
    if (occ(c.nn_grid) >= want) return c.nn_grid;
    for (int m = 0; m < c.n_mid; ++m)
        if (occ(c.mid_grid[m]) >= want) return c.mid_grid[m];
    return c.grid;
}

template <int KC>
void launch_knn_mean(me_ctx *ctx, const Cloud &c, const GridView &g, int k, double *avg, unsigned int *list, unsigned int *list_count) {
    const FrameView fr{c.origin[0], c.origin[1], c.origin[2], c.fine_h};
    hipLaunchKernelGGL(k_knn_mean<KC>, dim3(blocks_of(c.n)), dim3(256), 0, ctx->stream, c.sp.as<SPoint>(), c.codes.as<unsigned long long>(),
                       c.n, g, fr, k, avg, list, list_count);
    // (the list's length stays on the device: a fixed grid strides over it)
    const unsigned int nb = (unsigned int) std::min<long long>(1024, (c.n + kWalkBlock - 1) / kWalkBlock);
    hipLaunchKernelGGL(k_knn_mean_walk<KC>, dim3(std::max(1u, nb)), dim3(kWalkBlock), 0, ctx->stream, c.sp.as<SPoint>(), c.oct, k,
                       (const unsigned int *) list, (const unsigned int *) list_count, avg);
}

// scratch of one filter call: [stats: 4 doubles][kept: u64][list count: u32, pad][partials: nb doubles]
constexpr size_t kAuxHead = 64;

}  // namespace

int statistical_outlier(me_ctx *ctx, int slot, int nb_neighbors, double std_ratio, double *avg_host, uint8_t *keep_host,
                        me_outlier_info *info) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_statistical_outlier"));
    if (nb_neighbors < 1 || nb_neighbors > kKnnMax) return ctx->fail(ME_ERR_ARG, "me_statistical_outlier: nb_neighbors must be in [1, 40]");
    if (!(std_ratio > 0) || !std::isfinite(std_ratio)) return ctx->fail(ME_ERR_ARG, "me_statistical_outlier: std_ratio must be > 0");
    Cloud &c = ctx->cloud[slot];
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    if (!c.index_valid) ME_TRY(cloud_build_index(ctx, slot, c.cell_size_req));
    ME_TRY(cloud_finish_octree(ctx, slot));
    const long long n = c.n;
    const int k = nb_neighbors;
    const unsigned int nb = (unsigned int) std::min<long long>(1024, std::max<long long>(1, (n + 255) / 256));
    const long long per = ((n + nb - 1) / nb + 255) / 256 * 256;
    DevBuf &avg = ctx->outlier_tmp[0], &list = ctx->outlier_tmp[1], aux;
    ME_CHECK(ctx, avg.ensure((size_t) n * 8));
    ME_CHECK(ctx, list.ensure((size_t) n * 4));
    ME_CHECK(ctx, aux.ensure(kAuxHead + (size_t) nb * 8));
    ME_CHECK(ctx, c.outlier_keep.ensure((size_t) n));
    c.outlier_keep_valid = false;
    double *stats = aux.as<double>();
    unsigned long long *kept = reinterpret_cast<unsigned long long *>(aux.as<char>() + 32);
    unsigned int *list_count = reinterpret_cast<unsigned int *>(aux.as<char>() + 40);
    double *part = reinterpret_cast<double *>(aux.as<char>() + kAuxHead);
    ME_CHECK(ctx, hipMemsetAsync(aux.p, 0, kAuxHead, ctx->stream));
    {
        TimerScope ts(ctx, "outlier");
        const GridView &g = knn_mean_grid(c, k);
        if (k <= 8) launch_knn_mean<8>(ctx, c, g, k, avg.as<double>(), list.as<unsigned int>(), list_count);
        else if (k <= 16) launch_knn_mean<16>(ctx, c, g, k, avg.as<double>(), list.as<unsigned int>(), list_count);
        else if (k <= 24) launch_knn_mean<24>(ctx, c, g, k, avg.as<double>(), list.as<unsigned int>(), list_count);
        else if (k <= 32) launch_knn_mean<32>(ctx, c, g, k, avg.as<double>(), list.as<unsigned int>(), list_count);
        else launch_knn_mean<40>(ctx, c, g, k, avg.as<double>(), list.as<unsigned int>(), list_count);
        hipLaunchKernelGGL(k_sor_partials<0>, dim3(nb), dim3(256), 0, ctx->stream, avg.as<double>(), n, per, stats, part);
        hipLaunchKernelGGL(k_sor_final<0>, dim3(1), dim3(256), 0, ctx->stream, part, (int) nb, n, std_ratio, stats);
        hipLaunchKernelGGL(k_sor_partials<1>, dim3(nb), dim3(256), 0, ctx->stream, avg.as<double>(), n, per, stats, part);
        hipLaunchKernelGGL(k_sor_final<1>, dim3(1), dim3(256), 0, ctx->stream, part, (int) nb, n, std_ratio, stats);
        hipLaunchKernelGGL(k_sor_mask, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, avg.as<double>(), n, stats,
                           c.outlier_keep.as<unsigned char>(), kept);
    }
    ME_CHECK(ctx, hipGetLastError());
    double h_stats[4] = {0, 0, 0, 0};
    unsigned long long h_kept = 0;
    unsigned int h_list = 0;
    {
        MailGuard mg(ctx);  // (the one device -> host read of the statistics)
        ME_TRY(mail_post(ctx, h_stats, stats, sizeof(h_stats)));
        ME_TRY(mail_post(ctx, &h_kept, kept, 8));
        ME_TRY(mail_post(ctx, &h_list, list_count, 4));
        ME_TRY(mg.sync());
    }
    if (avg_host) ME_TRY(copy_d2h(ctx, avg_host, avg.p, (size_t) n * 8));
    if (keep_host) ME_TRY(copy_d2h(ctx, keep_host, c.outlier_keep.p, (size_t) n));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    c.outlier_keep_valid = true;
    if (info) {
        info->n_in = n;
        info->n_kept = (int64_t) h_kept;
        info->n_fallback = (int64_t) h_list;
        info->mean = h_stats[0];
        info->std_dev = h_stats[1];
        info->threshold = h_stats[2];
    }
    return ME_OK;
}

int radius_outlier(me_ctx *ctx, int slot, int nb_points, double radius, int32_t *counts_host, uint8_t *keep_host, me_outlier_info *info) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_radius_outlier"));
    if (nb_points < 0) return ctx->fail(ME_ERR_ARG, "me_radius_outlier: nb_points must be >= 0");
    if (!(radius > 0) || !std::isfinite(radius)) return ctx->fail(ME_ERR_ARG, "me_radius_outlier: radius must be > 0");
    Cloud &c = ctx->cloud[slot];
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    // the radius grid, rebuilt as me_mme does: the 27-cell stencil is exact when the cell edge is >= r, and not needlessly coarse
    const double want_h = radius * (1.0 + 0x1p-20);
    if (!c.index_valid || c.cell_h < want_h || c.cell_h > 1.5 * want_h) {
        const double req = c.cell_size_req;
        ME_TRY(cloud_build_index(ctx, slot, radius));
        c.cell_size_req = req;  // (a selection re-indexes the kept points at the cell the caller asked for, as an upload of them would)
    }
    const long long n = c.n;
    DevBuf &counts = ctx->outlier_tmp[0], aux;
    ME_CHECK(ctx, counts.ensure((size_t) n * 4));
    ME_CHECK(ctx, aux.ensure(kAuxHead));
    ME_CHECK(ctx, c.outlier_keep.ensure((size_t) n));
    c.outlier_keep_valid = false;
    unsigned long long *kept = aux.as<unsigned long long>();
    ME_CHECK(ctx, hipMemsetAsync(aux.p, 0, kAuxHead, ctx->stream));
    {
        TimerScope ts(ctx, "outlier");
        hipLaunchKernelGGL(k_radius_count, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, c.sp.as<SPoint>(), c.codes.as<unsigned long long>(),
                           n, c.grid, radius * radius, nb_points, counts.as<int>(), c.outlier_keep.as<unsigned char>(), kept);
    }
    ME_CHECK(ctx, hipGetLastError());
    unsigned long long h_kept = 0;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h_kept, kept, 8));
        ME_TRY(mg.sync());
    }
    if (counts_host) ME_TRY(copy_d2h(ctx, counts_host, counts.p, (size_t) n * 4));
    if (keep_host) ME_TRY(copy_d2h(ctx, keep_host, c.outlier_keep.p, (size_t) n));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    c.outlier_keep_valid = true;
    if (info) {
        info->n_in = n;
        info->n_kept = (int64_t) h_kept;
        info->n_fallback = 0;
        info->mean = 0.0;
        info->std_dev = 0.0;
        info->threshold = (double) nb_points;
    }
    return ME_OK;
}

// The kept points of src's last mask into dst (in place when dst is src), in cloud order; dst gets the reset of a changed cloud and a
// new index.  Another context's stream waits for src's pending work, as in voxel_downsample_into.
int outlier_select_into(me_ctx *sctx, int src_slot, me_ctx *dctx, int dst_slot, long long *n_out) {
    if (src_slot < 0 || src_slot > 1 || dst_slot < 0 || dst_slot > 1) return dctx->fail(ME_ERR_ARG, "me_outlier_select_into: bad slot");
    if (sctx->device != dctx->device) return dctx->fail(ME_ERR_ARG, "me_outlier_select_into: the contexts are on different devices");
    Cloud &S = sctx->cloud[src_slot];
    Cloud &D = dctx->cloud[dst_slot];
    if (sctx->shard_world != 1 || dctx->shard_world != 1 || sctx->slab.axis >= 0 || dctx->slab.axis >= 0 || S.slab.axis >= 0)
        return dctx->fail(ME_ERR_ARG, "me_outlier_select_into: single GPU only (no slab or shard mode)");
    if (!S.uploaded) return dctx->fail(ME_ERR_STATE, "me_outlier_select_into: source cloud not uploaded");
    if (!S.outlier_keep_valid)
        return dctx->fail(ME_ERR_STATE, "me_outlier_select_into: the source has no outlier mask (me_statistical_outlier / me_radius_outlier)");
    ME_CHECK(dctx, hipSetDevice(dctx->device));
    struct EventGuard {  // destroyed only once dst's stream has passed its wait (below) or on an early return
        hipEvent_t ev = nullptr;
        hipStream_t s = nullptr;
        ~EventGuard() {
            if (!ev) return;
            (void) hipStreamSynchronize(s);
            (void) hipEventDestroy(ev);
        }
    } eg;
    if (sctx->stream != dctx->stream) {
        ME_CHECK(dctx, hipEventCreateWithFlags(&eg.ev, hipEventDisableTiming));
        eg.s = dctx->stream;
        ME_CHECK(dctx, hipEventRecord(eg.ev, sctx->stream));
        ME_CHECK(dctx, hipStreamWaitEvent(dctx->stream, eg.ev, 0));
    }
    const long long n = S.n;
    DevBuf idx, cnt;
    ME_CHECK(dctx, idx.ensure((size_t) n * 4));
    ME_CHECK(dctx, cnt.ensure(16));
    TimerScope ts(dctx, "outlier_select");
    ME_TRY(select_flagged_u32(dctx, S.outlier_keep.as<unsigned char>(), n, idx.as<unsigned int>(), cnt.as<unsigned int>()));
    unsigned int h_m = 0;
    {
        MailGuard mg(dctx);
        ME_TRY(mail_post(dctx, &h_m, cnt.p, 4));
        ME_TRY(mg.sync());
    }
    const long long m = h_m;
    if (m == 0) return dctx->fail(ME_ERR_STATE, "me_outlier_select_into: the mask keeps no point (a cloud cannot be empty)");
    const bool normals = S.have_normals;
    DevBuf xyz_out, nrm_out;
    ME_CHECK(dctx, xyz_out.ensure((size_t) m * 24));
    if (normals) ME_CHECK(dctx, nrm_out.ensure((size_t) m * 24));
    hipLaunchKernelGGL(k_keep_gather, dim3(blocks_of(m)), dim3(256), 0, dctx->stream, idx.as<unsigned int>(), m, S.xyz.as<double>(),
                       normals ? S.normals.as<double>() : (const double *) nullptr, xyz_out.as<double>(), normals ? nrm_out.as<double>() : nullptr);
    ts.end();
    ME_CHECK(dctx, hipStreamSynchronize(dctx->stream));  // (src is read; from here on only dst changes)
    ME_CHECK(dctx, hipGetLastError());
    const double cell_req = S.cell_size_req;
    std::swap(D.xyz.p, xyz_out.p);
    std::swap(D.xyz.bytes, xyz_out.bytes);
    std::swap(D.xyz.owned, xyz_out.owned);
    if (normals) {
        std::swap(D.normals.p, nrm_out.p);
        std::swap(D.normals.bytes, nrm_out.bytes);
        std::swap(D.normals.owned, nrm_out.owned);
    }
    // the reset of a replaced cloud (as voxel_downsample_into's): covariances, features, NN and MME results are dropped
    cloud_reset_replaced(dctx, dst_slot, m, cell_req);
    D.have_normals = normals;
    if (n_out) *n_out = m;
    return cloud_finish(dctx, dst_slot);
}

}  // namespace me
