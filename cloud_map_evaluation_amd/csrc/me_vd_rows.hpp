// me_vd_rows.hpp — THE ROWS OF THE AWD TABLE AND THEIR USED POINTS, shared by me_voxdist.hip and me_transport.hip: the join of the two
// voxel tables with the min_pts gate, per row the start of the voxel's points in each cloud's OWN order (me_point_order.hpp: by voxel,
// inside a voxel by original index), the stride rule of the sub-sample, the offsets of the rows' used points and the gather of those
// points into contiguous fp64 xyz per cloud.  DESIGN.md sections 4.24 and 4.26.
//   pass 0  k_vd_join / k_vd_rows    the join; per row the start, the stride and the used counts
//   pass 1  k_vd_scan                offsets of a row's used points and of its pair tiles (one block, 64-bit)
//   pass 2  k_vd_gather              the used points of the rows, contiguous fp64 xyz per cloud
#pragma once

#include "me_internal.hpp"
#include "me_point_order.hpp"
#include "me_vox_rows.hpp"

#ifndef ME_TUNE_VOXDIST_TILE
#define ME_TUNE_VOXDIST_TILE 256  // points per side of a pair tile = lanes of its workgroup (a multiple of 64)
#endif

#ifdef __HIPCC__
namespace me {

constexpr int kVdT = ME_TUNE_VOXDIST_TILE;
static_assert(kVdT % 64 == 0 && kVdT >= 64 && kVdT <= 1024, "a tile is a whole number of wavefronts of one workgroup");

// per row: what the later passes read
struct VdRows {
    int *ei, *gi;            // the row's voxel in either table
    unsigned int *start;     // [M][2] first entry of the voxel in the cloud's own order (est, gt)
    int *stride;             // [M][2]
    int *pop, *used;         // [M][2] each
    long long *pairs;        // [M]
    long long *cnt;          // [3][M + 1]: used est, used gt, tiles -> (in place) their exclusive prefix sums, the totals at [M]
};

__device__ __forceinline__ long long vd_tri(long long t) { return t * (t + 1) / 2; }

// match[i] = 1 iff est voxel i has a ground-truth voxel of the same key and both populations are >= min_pts (k_join of me_voxel.hip)
static __global__ void __launch_bounds__(256)
k_vd_join(const unsigned long long *__restrict__ ekey, const int *__restrict__ en, long long Ve, const unsigned long long *__restrict__ gkey,
          const int *__restrict__ gn, long long Vg, int min_pts, int *__restrict__ gi_out, unsigned int *__restrict__ match) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Ve) return;
    const unsigned long long k = ekey[i];
    long long lo = 0, hi = Vg;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (gkey[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    const bool found = lo < Vg && gkey[lo] == k;
    gi_out[i] = found ? (int) lo : -1;
    match[i] = (found && en[i] >= min_pts && gn[lo] >= min_pts) ? 1u : 0u;
}

__device__ __forceinline__ unsigned int vd_lower_bound(const unsigned long long *__restrict__ a, long long n, unsigned long long k) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return (unsigned int) lo;
}

// the stride rule: every s-th point of the voxel's list, s = ceil(n / max_points), ceil(n / s) of them
__device__ __forceinline__ void vd_stride(int n, long long max_points, int &s, int &used) {
    s = 1;
    if (max_points > 0 && (long long) n > max_points) s = (int) (((long long) n + max_points - 1) / max_points);
    used = (n + s - 1) / s;
}

static __global__ void __launch_bounds__(256)
k_vd_rows(const unsigned int *__restrict__ match, const unsigned int *__restrict__ mpos, const int *__restrict__ gi, long long Ve,
          const unsigned long long *__restrict__ ekey, const int *__restrict__ en, const int *__restrict__ gn,
          const unsigned long long *__restrict__ skey_e, long long n_e, const unsigned long long *__restrict__ skey_g, long long n_g,
          long long max_points, long long M, VdRows R, int *__restrict__ keys3) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Ve || !match[i]) return;
    const long long r = mpos[i];
    const int g = gi[i];
    const unsigned long long key = ekey[i];
    int kx, ky, kz;
    unpack_key(key, kx, ky, kz);
    keys3[3 * r] = kx, keys3[3 * r + 1] = ky, keys3[3 * r + 2] = kz;
    R.ei[r] = (int) i;
    R.gi[r] = g;
    const int pe = en[i], pg = gn[g];
    int se, sg, ue, ug;
    vd_stride(pe, max_points, se, ue);
    vd_stride(pg, max_points, sg, ug);
    R.start[2 * r] = vd_lower_bound(skey_e, n_e, key);
    R.start[2 * r + 1] = vd_lower_bound(skey_g, n_g, key);
    R.stride[2 * r] = se, R.stride[2 * r + 1] = sg;
    R.pop[2 * r] = pe, R.pop[2 * r + 1] = pg;
    R.used[2 * r] = ue, R.used[2 * r + 1] = ug;
    const long long n = ue, m = ug;
    R.pairs[r] = (n * (n - 1) / 2 + m * (m - 1) / 2) + n * m;
    const long long ti = (n + kVdT - 1) / kVdT, tj = (m + kVdT - 1) / kVdT;
    R.cnt[r] = n;
    R.cnt[(M + 1) + r] = m;
    R.cnt[2 * (M + 1) + r] = (vd_tri(ti) + vd_tri(tj)) + ti * tj;
}

// ONE block: the three rows of cnt ([3][M + 1]) -> their exclusive prefix sums in place, the totals in entry M.  Thread t scans the
// chunk [t c, (t + 1) c), thread 0 the 256 chunk totals.
static __global__ void __launch_bounds__(256)
k_vd_scan(long long *__restrict__ cnt, long long M) {
    __shared__ long long s_tot[256];
    const long long c = (M + 255) / 256;
    const long long b = (long long) threadIdx.x * c, e = b + c < M ? b + c : M;
    for (int q = 0; q < 3; ++q) {
        long long *a = cnt + (size_t) q * (M + 1);
        long long s = 0;
        for (long long k = b; k < e; ++k) s += a[k];
        s_tot[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long run = 0;
            for (int t = 0; t < 256; ++t) {
                const long long v = s_tot[t];
                s_tot[t] = run;
                run += v;
            }
            a[M] = run;
        }
        __syncthreads();
        long long run = s_tot[threadIdx.x];
        for (long long k = b; k < e; ++k) {
            const long long v = a[k];
            a[k] = run;
            run += v;
        }
        __syncthreads();
    }
}

// block (r, side): the used points of row r in cloud `side`, in the cloud's own order -> dst[side][off[r] ..][3]
static __global__ void __launch_bounds__(256)
k_vd_gather(VdRows R, long long M, const unsigned int *__restrict__ spos_e, const SPoint *__restrict__ sp_e, long long n_e,
            const unsigned int *__restrict__ spos_g, const SPoint *__restrict__ sp_g, long long n_g, double *__restrict__ X,
            double *__restrict__ Y) {
    const long long r = blockIdx.x;
    const int side = blockIdx.y;
    if (r >= M) return;
    const unsigned int *spos = side ? spos_g : spos_e;
    const SPoint *sp = side ? sp_g : sp_e;
    const long long n_c = side ? n_g : n_e;
    double *dst = (side ? Y : X) + 3 * R.cnt[(size_t) side * (M + 1) + r];
    const long long start = R.start[2 * r + side], stride = R.stride[2 * r + side];
    const int used = R.used[2 * r + side];
    for (int u = threadIdx.x; u < used; u += 256) {
        const long long i = start + (long long) u * stride;
        double x = 0.0, y = 0.0, z = 0.0;
        if (i < n_c) {  // (always: the voxel's list holds its population)
            const long long s = spos[i];
            if (s < n_c) {
                const SPoint p = sp[s];
                x = p.x, y = p.y, z = p.z;
            }
        }
        dst[3 * u] = x, dst[3 * u + 1] = y, dst[3 * u + 2] = z;
    }
}

// HOST: the join of the two slots' voxel tables (built here when a slot holds none of this size) -> M, the number of rows; gi, match
// and mpos stay in ctx->tmp[0 .. 2] for vd_rows_build.  The stream is synchronised once.
static inline int vd_rows_count(me_ctx *ctx, double vs, int min_pts, long long &M) {
    Cloud &E = ctx->cloud[ME_SLOT_EST], &G = ctx->cloud[ME_SLOT_GT];
    ME_TRY(voxel_build(ctx, ME_SLOT_GT, vs, false));
    ME_TRY(voxel_build(ctx, ME_SLOT_EST, vs, false));
    const long long Ve = E.n_vox, Vg = G.n_vox;
    M = 0;
    DevBuf &gi_d = ctx->tmp[0], &match_d = ctx->tmp[1], &mpos_d = ctx->tmp[2];
    if (Ve > 0 && Vg > 0) {
        ME_CHECK(ctx, gi_d.ensure((size_t) Ve * 4));
        ME_CHECK(ctx, match_d.ensure((size_t) Ve * 4));
        ME_CHECK(ctx, mpos_d.ensure((size_t) Ve * 4));
        hipLaunchKernelGGL(k_vd_join, dim3(blocks_of(Ve)), dim3(256), 0, ctx->stream, (const unsigned long long *) E.vox_key.as<unsigned long long>(),
                           (const int *) E.vox_n.as<int>(), Ve, (const unsigned long long *) G.vox_key.as<unsigned long long>(),
                           (const int *) G.vox_n.as<int>(), Vg, min_pts, gi_d.as<int>(), match_d.as<unsigned int>());
        ME_TRY(exclusive_scan_u32(ctx, match_d.as<unsigned int>(), mpos_d.as<unsigned int>(), Ve));
        unsigned int last_pos = 0, last_flag = 0;
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &last_pos, mpos_d.as<unsigned int>() + (Ve - 1), 4));
        ME_TRY(mail_post(ctx, &last_flag, match_d.as<unsigned int>() + (Ve - 1), 4));
        ME_TRY(mg.sync());
        M = (long long) last_pos + last_flag;
    }
    return ME_OK;
}

// what vd_rows_build leaves: the rows (in ctx->tmp[3]), the own orders of both clouds (local buffers: they die with this object) and
// the totals of the three counts
struct VdBuilt {
    VdRows R;
    int *keys3 = nullptr;
    long long tot[3] = {0, 0, 0};  // used est, used gt, pair tiles
    DevBuf okey_d, opos_d, skey_e, spos_e, skey_g, spos_g;
};

// HOST: passes 0 and 1 for the M > 0 rows counted by vd_rows_count just before (ctx->tmp[0 .. 2] untouched since).  ctx->red must hold
// 8 bytes at least; its first two ints are used as the range-check flags.  Kernels under the device timer `timer`.
static inline int vd_rows_build(me_ctx *ctx, double vs, long long max_points, long long M, const char *timer, const char *who, VdBuilt &B) {
    Cloud &E = ctx->cloud[ME_SLOT_EST], &G = ctx->cloud[ME_SLOT_GT];
    const long long Ve = E.n_vox;
    DevBuf &gi_d = ctx->tmp[0], &match_d = ctx->tmp[1], &mpos_d = ctx->tmp[2];
    int *err = ctx->red.as<int>();
    ME_CHECK(ctx, hipMemsetAsync(err, 0, 8, ctx->stream));
    ME_TRY(points_own_order(ctx, E, vs, err, timer, who, B.okey_d, B.opos_d, B.skey_e, B.spos_e));
    ME_TRY(points_own_order(ctx, G, vs, err + 1, timer, who, B.okey_d, B.opos_d, B.skey_g, B.spos_g));
    DevBuf &rows_d = ctx->tmp[3];
    // [M] ei | gi | [M][2] start | stride | pop | used | [M][3] keys | [M] pairs | [3][M + 1] cnt   (8-byte words last)
    const size_t w4 = (size_t) M * (2 + 4 * 2 + 3);
    const size_t off8 = (w4 * 4 + 7) & ~(size_t) 7;
    ME_CHECK(ctx, rows_d.ensure(off8 + (size_t) M * 8 + (size_t) 3 * (M + 1) * 8));
    VdRows &R = B.R;
    R.ei = rows_d.as<int>();
    R.gi = R.ei + M;
    R.start = reinterpret_cast<unsigned int *>(R.gi + M);
    R.stride = reinterpret_cast<int *>(R.start + 2 * M);
    R.pop = R.stride + 2 * M;
    R.used = R.pop + 2 * M;
    B.keys3 = R.used + 2 * M;
    R.pairs = reinterpret_cast<long long *>(reinterpret_cast<char *>(rows_d.p) + off8);
    R.cnt = R.pairs + M;
    {
        TimerScope ts(ctx, timer);
        hipLaunchKernelGGL(k_vd_rows, dim3(blocks_of(Ve)), dim3(256), 0, ctx->stream, (const unsigned int *) match_d.as<unsigned int>(),
                           (const unsigned int *) mpos_d.as<unsigned int>(), (const int *) gi_d.as<int>(), Ve,
                           (const unsigned long long *) E.vox_key.as<unsigned long long>(), (const int *) E.vox_n.as<int>(),
                           (const int *) G.vox_n.as<int>(), (const unsigned long long *) B.skey_e.as<unsigned long long>(), E.n,
                           (const unsigned long long *) B.skey_g.as<unsigned long long>(), G.n, max_points, M, R, B.keys3);
        hipLaunchKernelGGL(k_vd_scan, dim3(1), dim3(256), 0, ctx->stream, R.cnt, M);
    }
    {
        MailGuard mg(ctx);
        for (int q = 0; q < 3; ++q) ME_TRY(mail_post(ctx, &B.tot[q], R.cnt + (size_t) q * (M + 1) + M, 8));
        ME_TRY(mg.sync());
    }
    return ME_OK;
}

// HOST: pass 2, queued on the context's stream (inside the caller's timer scope)
static inline void vd_gather_launch(me_ctx *ctx, const VdBuilt &B, long long M, double *X, double *Y) {
    const Cloud &E = ctx->cloud[ME_SLOT_EST], &G = ctx->cloud[ME_SLOT_GT];
    hipLaunchKernelGGL(k_vd_gather, dim3((unsigned int) M, 2), dim3(256), 0, ctx->stream, B.R, M, (const unsigned int *) B.spos_e.as<unsigned int>(),
                       (const SPoint *) E.sp.as<SPoint>(), E.n, (const unsigned int *) B.spos_g.as<unsigned int>(),
                       (const SPoint *) G.sp.as<SPoint>(), G.n, X, Y);
}

}  // namespace me
#endif
