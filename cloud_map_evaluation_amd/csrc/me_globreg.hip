// me_globreg.hip — coarse global registration on the device: Open3D's compute_fpfh_feature + registration_ransac_based_on_feature_matching
// (the initial pose the reference's users find by hand, its FAQ "How to obtain initial pose?").  DESIGN.md section 4.7.
//   k_spfh        per point: the hybrid neighbour list (the exact k-NN lists of k_knn_normals, d2 < r^2, self removed by index),
//                 the pair features and the 3 x 11-bin SPFH                                               (me_fpfh, timer "fpfh")
//   k_fpfh        per point: sum of SPFH(j) / d2 over the list, per-block scaling to 100, + SPFH(i)
//   k_feat_nn     exact 1-NN in the 33-dimensional feature space: reference features staged through LDS in tiles, one query per lane,
//                 the running best in registers; the reference set is split into chunks (a grid column each) merged by k_feat_merge
//                 in chunk order, so that ties keep the smallest index                                  (me_fpfh_match, "fpfh_match")
//   k_ransac_hyp  per hypothesis h: Philox sample, validity checks, Horn fit (me_horn.hpp)              (me_global_register, "ransac")
//   k_ransac_score per valid hypothesis (compacted, hypothesis order kept): correspondence inliers, correspondences streamed through LDS
//   k_fit_moved + me_nn_points + k_fit_reduce: the top hypotheses re-scored on the whole source cloud          ("ransac_validate")
// Every sum has a fixed order and the file is compiled with -ffp-contract=off: tests/_globreg_ref.py restates the arithmetic.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "me_horn.hpp"
#include "me_internal.hpp"
#include "me_philox.hpp"

namespace me {

namespace {

constexpr int kFeat = 33;

// ComputePairFeatures [Open3D] of (p1, n1, p2, n2) -> (f0, f1, f2); the swap test |a1| < |a2| stands for acos(|a1|) > acos(|a2|)
__device__ __forceinline__ void pair_feature(const double *p1, const double *n1, const double *p2, const double *n2, double f[3]) {
    f[0] = f[1] = f[2] = 0.0;
    double d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double L = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (L == 0.0) return;
    const double a1 = dot3(n1, d) / L, a2 = dot3(n2, d) / L;
    const double *m1 = n1, *m2 = n2;
    double f2 = a1;
    if (fabs(a1) < fabs(a2)) {
        m1 = n2;
        m2 = n1;
        d[0] = -d[0];
        d[1] = -d[1];
        d[2] = -d[2];
        f2 = -a2;
    }
    double v[3], w[3];
    cross3(d, m1, v);
    const double vn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (vn == 0.0) return;
    v[0] /= vn;
    v[1] /= vn;
    v[2] /= vn;
    cross3(m1, v, w);
    f[0] = atan2(dot3(w, m2), dot3(m1, m2));
    f[1] = dot3(v, m2);
    f[2] = f2;
}

__device__ __forceinline__ int clamp_bin(double b) { return !(b > 0.0) ? 0 : (b >= 10.0 ? 10 : (int) b); }

// the hybrid neighbour j of the list entry (idx, d2), or -1: inside the radius and not the query itself
__device__ __forceinline__ bool hybrid_keep(int idx, double d2, long long i, double r2) { return idx >= 0 && idx != i && d2 < r2; }

__global__ void __launch_bounds__(256) k_spfh(const double *__restrict__ xyz, const double *__restrict__ nrm, long long n,
                                              const int *__restrict__ nidx, const double *__restrict__ nd2, int k, double r2,
                                              double *__restrict__ spfh) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int m = 0;
    for (int j = 0; j < k; ++j) m += hybrid_keep(nidx[i * k + j], nd2[i * k + j], i, r2) ? 1 : 0;
    double *out = spfh + i * kFeat;  // zeroed by the caller; this lane's own row
    if (m == 0) return;
    const double inc = 100.0 / (double) m;
    const double p1[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    const double n1[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
    for (int j = 0; j < k; ++j) {
        const int q = nidx[i * k + j];
        if (!hybrid_keep(q, nd2[i * k + j], i, r2)) continue;
        const double p2[3] = {xyz[3 * q], xyz[3 * q + 1], xyz[3 * q + 2]};
        const double n2[3] = {nrm[3 * q], nrm[3 * q + 1], nrm[3 * q + 2]};
        double f[3];
        pair_feature(p1, n1, p2, n2, f);
        out[clamp_bin(floor(11.0 * (f[0] + M_PI) / (2.0 * M_PI)))] += inc;
        out[11 + clamp_bin(floor(11.0 * (f[1] + 1.0) * 0.5))] += inc;
        out[22 + clamp_bin(floor(11.0 * (f[2] + 1.0) * 0.5))] += inc;
    }
}

__global__ void __launch_bounds__(256) k_fpfh(const double *__restrict__ spfh, long long n, const int *__restrict__ nidx,
                                              const double *__restrict__ nd2, int k, double r2, double *__restrict__ feat) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double f[kFeat], s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < kFeat; ++b) f[b] = 0.0;
    for (int j = 0; j < k; ++j) {
        const int q = nidx[i * k + j];
        const double d2 = nd2[i * k + j];
        if (!hybrid_keep(q, d2, i, r2) || d2 == 0.0) continue;
        const double *sq = spfh + (long long) q * kFeat;
#pragma unroll
        for (int b = 0; b < kFeat; ++b) {
            const double val = sq[b] / d2;
            s[b / 11] += val;
            f[b] += val;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (s[c] != 0.0) s[c] = 100.0 / s[c];
    const double *si = spfh + i * kFeat;
#pragma unroll
    for (int b = 0; b < kFeat; ++b) {
        const double sc = s[b / 11];
        const double v = (sc != 0.0 ? f[b] * sc : f[b]) + si[b];
        feat[i * kFeat + b] = v;
    }
}

// ---- feature-space 1-NN ----
constexpr int kNnBlock = 256;
constexpr int kNnTile = 64;  // reference features per LDS tile: 64 x 33 x 8 B = 16.9 KB

// queries blockIdx.x * 256 + tid, references of chunk blockIdx.y: [y * chunk, min(nr, (y + 1) * chunk)); partial best per (chunk, query)
__global__ void __launch_bounds__(kNnBlock) k_feat_nn(const double *__restrict__ Q, long long nq, const double *__restrict__ R, long long nr,
                                                      long long chunk, double *__restrict__ part_d, int *__restrict__ part_i) {
    __shared__ double tile[kNnTile * kFeat];
    const long long qi = (long long) blockIdx.x * kNnBlock + threadIdx.x;
    double q[kFeat];
#pragma unroll
    for (int b = 0; b < kFeat; ++b) q[b] = qi < nq ? Q[qi * kFeat + b] : 0.0;
    const long long r0 = (long long) blockIdx.y * chunk, r1 = nr < r0 + chunk ? nr : r0 + chunk;
    double bd = INFINITY;
    int bi = -1;
    for (long long base = r0; base < r1; base += kNnTile) {
        const int cnt = (int) (r1 - base < kNnTile ? r1 - base : kNnTile);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * kFeat; e += kNnBlock) tile[e] = R[base * kFeat + e];
        __syncthreads();
        for (int r = 0; r < cnt; ++r) {
            const double *t = tile + r * kFeat;
            double d = 0.0;
#pragma unroll
            for (int b = 0; b < kFeat; ++b) {
                const double e = q[b] - t[b];
                d += e * e;
            }
            if (d < bd) {
                bd = d;
                bi = (int) (base + r);
            }
        }
    }
    if (qi < nq) {
        part_d[blockIdx.y * nq + qi] = bd;
        part_i[blockIdx.y * nq + qi] = bi;
    }
}

__global__ void __launch_bounds__(256) k_feat_merge(const double *__restrict__ part_d, const int *__restrict__ part_i, long long nq, int chunks,
                                                    int *__restrict__ nn) {
    const long long qi = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    double bd = INFINITY;
    int bi = -1;
    for (int c = 0; c < chunks; ++c) {  // ascending chunks hold ascending indices: a strict < keeps the smallest on a tie
        const double d = part_d[c * nq + qi];
        if (d < bd) {
            bd = d;
            bi = part_i[c * nq + qi];
        }
    }
    nn[qi] = bi;
}

__global__ void __launch_bounds__(256) k_corr(const int *__restrict__ nn_sr, long long ns, const int *__restrict__ nn_rs, int mutual,
                                              int *__restrict__ corr, unsigned char *__restrict__ flag) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    int j = nn_sr[i];
    if (j >= 0 && mutual && nn_rs[j] != (int) i) j = -1;
    corr[i] = j;
    flag[i] = j >= 0 ? 1 : 0;
}

// correspondence c = (source point list[c], reference point corr[list[c]]) packed as (sx, sy, sz, qx, qy, qz)
__global__ void __launch_bounds__(256) k_pack_corr(const unsigned int *__restrict__ list, long long nc, const int *__restrict__ corr,
                                                   const double *__restrict__ sxyz, const double *__restrict__ rxyz, double *__restrict__ c6) {
    const long long c = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const long long i = list[c], j = corr[i];
    c6[6 * c] = sxyz[3 * i];
    c6[6 * c + 1] = sxyz[3 * i + 1];
    c6[6 * c + 2] = sxyz[3 * i + 2];
    c6[6 * c + 3] = rxyz[3 * j];
    c6[6 * c + 4] = rxyz[3 * j + 1];
    c6[6 * c + 5] = rxyz[3 * j + 2];
}

__device__ __forceinline__ double moved_d2(const double *T, double sx, double sy, double sz, double qx, double qy, double qz) {
    const double x = ((T[0] * sx + T[1] * sy) + T[2] * sz) + T[3];
    const double y = ((T[4] * sx + T[5] * sy) + T[6] * sz) + T[7];
    const double z = ((T[8] * sx + T[9] * sy) + T[10] * sz) + T[11];
    const double dx = x - qx, dy = y - qy, dz = z - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ double edge(const double *a, const double *b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

struct RansacK {
    u64 seed;
    u64 n_corr;
    double eps2, edge_ratio;
};

// hypothesis h = h0 + t (or hlist[t]): sample, check, fit.  T[t] = [R | t] (3 x 4), valid[t] = 0 / 1
__global__ void __launch_bounds__(256) k_ransac_hyp(long long h0, long long nh, const long long *__restrict__ hlist, RansacK k,
                                                    const double *__restrict__ c6, double *__restrict__ Tout, unsigned char *__restrict__ valid) {
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nh) return;
    const u64 h = hlist ? (u64) hlist[t] : (u64) (h0 + t);
    u64 w[4];
    philox_block(k.seed, h, 4, 0, w);
    const u64 s0 = mulhi64(w[0], k.n_corr), s1 = mulhi64(w[1], k.n_corr), s2 = mulhi64(w[2], k.n_corr);
    double T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.0;
    bool ok = s0 != s1 && s0 != s2 && s1 != s2;
    if (ok) {
        const u64 sid[3] = {s0, s1, s2};
        double p[9], q[9];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                p[3 * j + a] = c6[6 * sid[j] + a];
                q[3 * j + a] = c6[6 * sid[j] + 3 + a];
            }
        // CorrespondenceCheckerBasedOnEdgeLength: pairs (0,1), (0,2), (1,2)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a + 1; b < 3; ++b) {
                const double ds = edge(p + 3 * a, p + 3 * b), dt = edge(q + 3 * a, q + 3 * b);
                if (ds < dt * k.edge_ratio || dt < ds * k.edge_ratio) ok = false;
            }
        // degenerate source triangle: |e01 x e02|^2 <= 1e-12 |e01|^2 |e02|^2
        const double e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
        double cr[3];
        cross3(e1, e2, cr);
        if (dot3(cr, cr) <= (1e-12 * dot3(e1, e1)) * dot3(e2, e2)) ok = false;
        if (ok) {
            horn_fit3(p, q, T);
#pragma unroll
            for (int j = 0; j < 3; ++j)  // CorrespondenceCheckerBasedOnDistance on the sample
                if (moved_d2(T, p[3 * j], p[3 * j + 1], p[3 * j + 2], q[3 * j], q[3 * j + 1], q[3 * j + 2]) > k.eps2) ok = false;
        }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) Tout[t * 12 + e] = T[e];
    valid[t] = ok ? 1 : 0;
}

constexpr int kScoreTile = 256;  // correspondences per LDS tile: 256 x 48 B = 12 KB

// one lane per valid hypothesis (vlist[c] = its slot in T); the correspondences stream through LDS
__global__ void __launch_bounds__(256) k_ransac_score(const unsigned int *__restrict__ vlist, const unsigned int *__restrict__ nv_d,
                                                      const double *__restrict__ Tall, const double *__restrict__ c6, long long nc, double eps2,
                                                      int *__restrict__ score) {
    __shared__ double tile[kScoreTile * 6];
    const unsigned int nv = *nv_d;
    if ((unsigned int) blockIdx.x * blockDim.x >= nv) return;  // (block-uniform: the grid is sized for the batch, not the valid count)
    const unsigned int c = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = c < nv;
    double T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = live ? Tall[(size_t) vlist[c] * 12 + e] : 0.0;
    int cnt = 0;
    for (long long base = 0; base < nc; base += kScoreTile) {
        const int m = (int) (nc - base < kScoreTile ? nc - base : kScoreTile);
        __syncthreads();
        for (int e = threadIdx.x; e < m * 6; e += blockDim.x) tile[e] = c6[base * 6 + e];
        __syncthreads();
        for (int r = 0; r < m; ++r) {
            const double *u = tile + 6 * r;
            cnt += moved_d2(T, u[0], u[1], u[2], u[3], u[4], u[5]) < eps2 ? 1 : 0;
        }
    }
    if (live) score[c] = cnt;
}

// the source cloud moved by each of nh hypotheses: out[t * n + i]
__global__ void __launch_bounds__(256) k_fit_moved(const double *__restrict__ xyz, long long n, const double *__restrict__ T, int nh,
                                                   double *__restrict__ out) {
    const long long g = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * nh) return;
    const long long t = g / n, i = g - t * n;
    const double *M = T + 12 * t;
    const double sx = xyz[3 * i], sy = xyz[3 * i + 1], sz = xyz[3 * i + 2];
    out[3 * g] = ((M[0] * sx + M[1] * sy) + M[2] * sz) + M[3];
    out[3 * g + 1] = ((M[4] * sx + M[5] * sy) + M[6] * sz) + M[7];
    out[3 * g + 2] = ((M[8] * sx + M[9] * sy) + M[10] * sz) + M[11];
}

// one block per hypothesis: inliers (d2 < eps2) and their d2 sum, fixed order (strided lanes, then block_sum_256)
__global__ void __launch_bounds__(256) k_fit_reduce(const double *__restrict__ d2, long long n, double eps2, long long *__restrict__ cnt,
                                                    double *__restrict__ sum) {
    __shared__ double sm_d[4];
    __shared__ long long sm_c[4];
    const double *dd = d2 + (long long) blockIdx.x * n;
    long long c = 0;
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const double v = dd[i];
        if (v < eps2) {
            ++c;
            s += v;
        }
    }
    const double ts = block_sum_256(s, sm_d);
    const long long tc = block_sum_256_ll(c, sm_c);
    if (threadIdx.x == 0) {
        cnt[blockIdx.x] = tc;
        sum[blockIdx.x] = ts;
    }
}

bool fpfh_params_ok(const me_fpfh_params *p) {
    return p && p->radius > 0 && std::isfinite(p->radius) && p->max_nn >= 1 && p->max_nn <= kKnnMax && p->normal_knn >= 1 &&
           p->normal_knn <= kKnnMax;
}

// feature-space matches on the device: corr[n_src] (int32, -1 = none) and the ascending list of matched source points
int match_device(me_ctx *ctx, int s_slot, int r_slot, int mutual, DevBuf &corr, DevBuf &list, long long *n_corr) {
    Cloud &S = ctx->cloud[s_slot], &R = ctx->cloud[r_slot];
    if (!S.fpfh_valid || !R.fpfh_valid) return ctx->fail(ME_ERR_STATE, "me_fpfh_match: both slots need me_fpfh features");
    const long long ns = S.n, nr = R.n;
    DevBuf nn_sr, nn_rs, part_d, part_i, flag, cnt;
    ME_CHECK(ctx, nn_sr.ensure((size_t) ns * 4));
    ME_CHECK(ctx, nn_rs.ensure((size_t) nr * 4));
    ME_CHECK(ctx, corr.ensure((size_t) ns * 4));
    ME_CHECK(ctx, list.ensure((size_t) ns * 4));
    ME_CHECK(ctx, flag.ensure((size_t) ns));
    ME_CHECK(ctx, cnt.ensure(16));
    {
        TimerScope ts(ctx, "fpfh_match");
        for (int dir = 0; dir < 2; ++dir) {
            const Cloud &A = dir == 0 ? S : R, &B = dir == 0 ? R : S;
            const long long nq = A.n, nb = B.n;
            const unsigned int qb = blocks_of(nq, kNnBlock);
            // enough grid columns to fill the chip (~4 blocks per CU), each at least a few tiles long
            long long chunks = std::max<long long>(1, std::min<long long>((1024 + qb - 1) / qb, (nb + 4 * kNnTile - 1) / (4 * kNnTile)));
            const long long chunk = (nb + chunks - 1) / chunks;
            chunks = (nb + chunk - 1) / chunk;
            ME_CHECK(ctx, part_d.ensure((size_t) chunks * nq * 8));
            ME_CHECK(ctx, part_i.ensure((size_t) chunks * nq * 4));
            hipLaunchKernelGGL(k_feat_nn, dim3(qb, (unsigned int) chunks), dim3(kNnBlock), 0, ctx->stream, A.fpfh.as<double>(), nq,
                               B.fpfh.as<double>(), nb, chunk, part_d.as<double>(), part_i.as<int>());
            hipLaunchKernelGGL(k_feat_merge, dim3(blocks_of(nq)), dim3(256), 0, ctx->stream, part_d.as<double>(), part_i.as<int>(), nq,
                               (int) chunks, (dir == 0 ? nn_sr : nn_rs).as<int>());
        }
        hipLaunchKernelGGL(k_corr, dim3(blocks_of(ns)), dim3(256), 0, ctx->stream, nn_sr.as<int>(), ns, nn_rs.as<int>(), mutual ? 1 : 0,
                           corr.as<int>(), flag.as<unsigned char>());
    }
    ME_TRY(select_flagged_u32(ctx, flag.as<unsigned char>(), ns, list.as<unsigned int>(), cnt.as<unsigned int>()));
    unsigned int h_cnt = 0;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h_cnt, cnt.p, 4));
        ME_TRY(mg.sync());
    }
    ME_CHECK(ctx, hipGetLastError());
    *n_corr = h_cnt;
    return ME_OK;
}

}  // namespace

int fpfh(me_ctx *ctx, int slot, const me_fpfh_params *p, double *features_host) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_fpfh"));
    if (!fpfh_params_ok(p))
        return ctx->fail(ME_ERR_ARG, "me_fpfh: radius must be finite and > 0, max_nn and normal_knn in [1, 40]");
    Cloud &c = ctx->cloud[slot];
    if (!c.index_valid) return ctx->fail(ME_ERR_STATE, "me_fpfh: cloud has no index");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    if (!c.have_normals) ME_TRY(estimate_normals(ctx, slot, p->normal_knn, nullptr, nullptr, nullptr));
    const long long n = c.n;
    const int k = p->max_nn;
    const double r2 = p->radius * p->radius;
    DevBuf nidx, nd2, spfh;  // released on return (n * k * 12 bytes)
    ME_CHECK(ctx, nidx.ensure((size_t) n * k * 4));
    ME_CHECK(ctx, nd2.ensure((size_t) n * k * 8));
    ME_CHECK(ctx, spfh.ensure((size_t) n * kFeat * 8));
    ME_CHECK(ctx, c.fpfh.ensure((size_t) n * kFeat * 8));
    c.fpfh_valid = false;
    {
        TimerScope ts(ctx, "fpfh");
        ME_TRY(knn_lists(ctx, slot, k, nidx.as<int>(), nd2.as<double>()));
        ME_CHECK(ctx, hipMemsetAsync(spfh.p, 0, (size_t) n * kFeat * 8, ctx->stream));
        hipLaunchKernelGGL(k_spfh, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, c.xyz.as<double>(), c.normals.as<double>(), n,
                           nidx.as<int>(), nd2.as<double>(), k, r2, spfh.as<double>());
        hipLaunchKernelGGL(k_fpfh, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, spfh.as<double>(), n, nidx.as<int>(), nd2.as<double>(), k,
                           r2, c.fpfh.as<double>());
    }
    ME_CHECK(ctx, hipGetLastError());
    if (features_host) ME_TRY(copy_d2h(ctx, features_host, c.fpfh.p, (size_t) n * kFeat * 8));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    c.fpfh_valid = true;
    return ME_OK;
}

int fpfh_match(me_ctx *ctx, int src_slot, int ref_slot, int mutual, int32_t *corr_host, long long *n_corr) {
    ME_TRY(need_single_gpu_cloud(ctx, src_slot, "me_fpfh_match"));
    ME_TRY(need_single_gpu_cloud(ctx, ref_slot, "me_fpfh_match"));
    if (src_slot == ref_slot) return ctx->fail(ME_ERR_ARG, "me_fpfh_match: src_slot == ref_slot");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    DevBuf corr, list;
    long long nc = 0;
    ME_TRY(match_device(ctx, src_slot, ref_slot, mutual, corr, list, &nc));
    if (corr_host) ME_TRY(copy_d2h(ctx, corr_host, corr.p, (size_t) ctx->cloud[src_slot].n * 4));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (n_corr) *n_corr = nc;
    return ME_OK;
}

int global_register(me_ctx *ctx, int src_slot, int ref_slot, const me_globreg_params *p, double T_out[16], me_globreg_info *info,
                    int64_t *scores) {
    ME_TRY(need_single_gpu_cloud(ctx, src_slot, "me_global_register"));
    ME_TRY(need_single_gpu_cloud(ctx, ref_slot, "me_global_register"));
    if (src_slot == ref_slot) return ctx->fail(ME_ERR_ARG, "me_global_register: src_slot == ref_slot");
    if (!p || !T_out) return ctx->fail(ME_ERR_ARG, "me_global_register: params or T_out is NULL");
    if (!(p->max_corr_dist > 0) || !std::isfinite(p->max_corr_dist) || !(p->edge_ratio > 0 && p->edge_ratio <= 1) ||
        p->max_iterations < 1 || p->validate_top < 1)
        return ctx->fail(ME_ERR_ARG, "me_global_register: max_corr_dist must be finite and > 0, edge_ratio in (0, 1], max_iterations and "
                                     "validate_top >= 1");
    Cloud &S = ctx->cloud[src_slot], &R = ctx->cloud[ref_slot];
    if ((!S.fpfh_valid || !R.fpfh_valid) && !fpfh_params_ok(&p->fpfh))
        return ctx->fail(ME_ERR_ARG, "me_global_register: fpfh.radius must be finite and > 0, max_nn and normal_knn in [1, 40]");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    if (!S.fpfh_valid) ME_TRY(fpfh(ctx, src_slot, &p->fpfh, nullptr));
    if (!R.fpfh_valid) ME_TRY(fpfh(ctx, ref_slot, &p->fpfh, nullptr));
    DevBuf corr, list;
    long long nc = 0;
    ME_TRY(match_device(ctx, src_slot, ref_slot, p->mutual, corr, list, &nc));
    if (nc < 3)
        return ctx->fail(ME_ERR_STATE, "me_global_register: " + std::to_string(nc) + " feature correspondences (RANSAC needs at least 3)");
    DevBuf c6;
    ME_CHECK(ctx, c6.ensure((size_t) nc * 48));
    hipLaunchKernelGGL(k_pack_corr, dim3(blocks_of(nc)), dim3(256), 0, ctx->stream, list.as<unsigned int>(), nc, corr.as<int>(),
                       S.xyz.as<double>(), R.xyz.as<double>(), c6.as<double>());
    RansacK rk{p->seed, (u64) nc, p->max_corr_dist * p->max_corr_dist, p->edge_ratio};
    const long long H = p->max_iterations;
    constexpr long long kBatch = 1LL << 18;  // hypotheses per batch (T: 24 MiB)
    const long long B = std::min(H, kBatch);
    DevBuf Tb, valid, vlist, nv_d, score_d;
    ME_CHECK(ctx, Tb.ensure((size_t) B * 96));
    ME_CHECK(ctx, valid.ensure((size_t) B));
    ME_CHECK(ctx, vlist.ensure((size_t) B * 4));
    ME_CHECK(ctx, nv_d.ensure(16));
    ME_CHECK(ctx, score_d.ensure((size_t) B * 4));
    std::vector<std::pair<long long, long long>> cand;  // (score, h) of every valid hypothesis, h ascending
    std::vector<unsigned int> h_list;
    std::vector<int> h_score;
    if (scores) std::fill(scores, scores + H, (int64_t) -1);
    for (long long h0 = 0; h0 < H; h0 += B) {
        const long long nb = std::min(B, H - h0);
        {
            TimerScope ts(ctx, "ransac");
            hipLaunchKernelGGL(k_ransac_hyp, dim3(blocks_of(nb)), dim3(256), 0, ctx->stream, h0, nb, (const long long *) nullptr, rk,
                               c6.as<double>(), Tb.as<double>(), valid.as<unsigned char>());
            ME_TRY(select_flagged_u32(ctx, valid.as<unsigned char>(), nb, vlist.as<unsigned int>(), nv_d.as<unsigned int>()));
            hipLaunchKernelGGL(k_ransac_score, dim3(blocks_of(nb)), dim3(256), 0, ctx->stream, vlist.as<unsigned int>(),
                               nv_d.as<unsigned int>(), Tb.as<double>(), c6.as<double>(), nc, rk.eps2, score_d.as<int>());
        }
        unsigned int nv = 0;
        {
            MailGuard mg(ctx);
            ME_TRY(mail_post(ctx, &nv, nv_d.p, 4));
            ME_TRY(mg.sync());
        }
        ME_CHECK(ctx, hipGetLastError());
        if (nv == 0) continue;
        h_list.resize(nv);
        h_score.resize(nv);
        ME_TRY(copy_d2h(ctx, h_list.data(), vlist.p, (size_t) nv * 4));
        ME_TRY(copy_d2h(ctx, h_score.data(), score_d.p, (size_t) nv * 4));
        ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        for (unsigned int c = 0; c < nv; ++c) {
            const long long h = h0 + h_list[c];
            cand.emplace_back(h_score[c], h);
            if (scores) scores[h] = h_score[c];
        }
    }
    if (cand.empty())
        return ctx->fail(ME_ERR_STATE, "me_global_register: no valid hypothesis among " + std::to_string(H) + " (" + std::to_string(nc) +
                                           " correspondences): more iterations, a larger max_corr_dist or another feature radius");
    // the top K by (score desc, h asc)
    const long long K = std::min<long long>(p->validate_top, (long long) cand.size());
    std::partial_sort(cand.begin(), cand.begin() + K, cand.end(), [](const std::pair<long long, long long> &a, const std::pair<long long, long long> &b) {
        return a.first != b.first ? a.first > b.first : a.second < b.second;
    });
    std::vector<long long> top(K);
    for (long long t = 0; t < K; ++t) top[t] = cand[t].second;
    DevBuf top_d, Tk, vk, moved, d2, cnt_d, sum_d;
    ME_CHECK(ctx, top_d.ensure((size_t) K * 8));
    ME_CHECK(ctx, Tk.ensure((size_t) K * 96));
    ME_CHECK(ctx, vk.ensure((size_t) K));
    ME_CHECK(ctx, cnt_d.ensure((size_t) K * 8));
    ME_CHECK(ctx, sum_d.ensure((size_t) K * 8));
    ME_TRY(copy_h2d(ctx, top_d.p, top.data(), (size_t) K * 8));
    const long long ns = S.n;
    const long long per = std::max<long long>(1, std::min<long long>(K, (1LL << 23) / std::max<long long>(1, ns)));  // hypotheses per 1-NN pass
    ME_CHECK(ctx, moved.ensure((size_t) per * ns * 24));
    ME_CHECK(ctx, d2.ensure((size_t) per * ns * 8));
    {
        TimerScope ts(ctx, "ransac_validate");
        hipLaunchKernelGGL(k_ransac_hyp, dim3(blocks_of(K)), dim3(256), 0, ctx->stream, 0LL, K, top_d.as<long long>(), rk, c6.as<double>(),
                           Tk.as<double>(), vk.as<unsigned char>());
    }
    for (long long t0 = 0; t0 < K; t0 += per) {
        const int nh = (int) std::min(per, K - t0);
        {
            TimerScope ts(ctx, "ransac_validate");
            hipLaunchKernelGGL(k_fit_moved, dim3(blocks_of(ns * nh)), dim3(256), 0, ctx->stream, S.xyz.as<double>(), ns, Tk.as<double>() + 12 * t0,
                               nh, moved.as<double>());
        }
        ME_TRY(nn_points(ctx, ref_slot, moved.as<double>(), ns * nh, d2.as<double>(), false));
        {
            TimerScope ts(ctx, "ransac_validate");
            hipLaunchKernelGGL(k_fit_reduce, dim3(nh), dim3(256), 0, ctx->stream, d2.as<double>(), ns, rk.eps2, cnt_d.as<long long>() + t0,
                               sum_d.as<double>() + t0);
        }
    }
    std::vector<long long> h_cnt(K);
    std::vector<double> h_sum(K), h_T((size_t) K * 12);
    ME_TRY(copy_d2h(ctx, h_cnt.data(), cnt_d.p, (size_t) K * 8));
    ME_TRY(copy_d2h(ctx, h_sum.data(), sum_d.p, (size_t) K * 8));
    ME_TRY(copy_d2h(ctx, h_T.data(), Tk.p, (size_t) K * 96));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ME_CHECK(ctx, hipGetLastError());
    // the winner by (fitness desc, rmse asc, h asc)
    long long best = -1;
    double bf = 0, br = 0;
    for (long long t = 0; t < K; ++t) {
        const double f = (double) h_cnt[t] / (double) ns;
        const double r = h_cnt[t] > 0 ? std::sqrt(h_sum[t] / (double) h_cnt[t]) : 0.0;
        if (best < 0 || f > bf || (f == bf && (r < br || (r == br && top[t] < top[best])))) {
            best = t;
            bf = f;
            br = r;
        }
    }
    for (int e = 0; e < 12; ++e) T_out[e] = h_T[(size_t) best * 12 + e];
    T_out[12] = T_out[13] = T_out[14] = 0.0;
    T_out[15] = 1.0;
    if (info) {
        info->n_corr = nc;
        info->n_valid_hypotheses = (int64_t) cand.size();
        info->best_hypothesis = top[best];
        info->best_corr_inliers = cand[best].first;
        info->fitness = bf;
        info->inlier_rmse = br;
    }
    return ME_OK;
}

}  // namespace me
