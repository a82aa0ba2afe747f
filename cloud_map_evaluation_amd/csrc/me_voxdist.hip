// me_voxdist.hip — per-voxel distribution distances on the AWD lattice (me_voxel_distances; the reference declares
// computeKLDivergenceGaussian, computeGaussianKernel, computeGaussianBhattacharyya and computeMMD at voxel_calculator.hpp:71-79 and
// defines none of them).  DESIGN.md section 4.24.
//
// The rows are the rows of me_awd_scs: the keys of both voxel tables with both populations >= min_pts, ascending.  Per row
//   the point-set MMD   every pair of the voxel's used points through a Gaussian kernel, per bandwidth: Sxx, Syy (i < j) and Sxy;
//   the closed forms    KL both ways, Bhattacharyya and the textbook 2-Wasserstein distance of the two voxel Gaussians.
//   pass 0  k_vd_join / k_vd_rows    the join of the two voxel tables; per row the start of the voxel's points in each cloud's OWN order
//                                    (me_point_order.hpp: by voxel, inside a voxel by original index), the stride and the used counts
//   pass 1  k_vd_scan                offsets of a row's used points and of its tiles (one block, 64-bit)
//   pass 2  k_vd_gather              the used points of the rows, contiguous fp64 xyz per cloud
//   pass 3  k_vd_tiles               the work list, built on the device: (row, block, i-tile, j-tile); XX and YY cover the upper
//                                    triangle only
//   pass 4  k_vd_pairs               ONE workgroup per tile.  A lane keeps its x_i in registers, the tile's y_j are staged once in LDS
//                                    and read at one address by all lanes (a broadcast), one fp64 accumulator per bandwidth, ascending
//                                    j, d2 once per pair for all bandwidths.  Lanes folded by wave_sum, the waves in wave order: one
//                                    partial per (tile, bandwidth) in the tile's own slot.
//   pass 5  k_vd_row_sums            one wavefront per row adds the row's tile partials (lane l takes the tiles l, l + 64, ... of a block in
//                                    order, then the xor butterfly) and forms the two estimates
//   pass 6  k_vd_gauss               one lane per row, plain arithmetic only (+ - * /, sqrt, log, jacobi_sym): tests/_voxdist_ref.py
//                                    restates it operation by operation (-ffp-contract=off)
//   pass 7  k_vd_totals              the means' sums over the rows in key order by the shared fixed-order reduction (me_reduce.hpp)
// No floating-point atomics anywhere: bit-identical from call to call and after any re-index of the same points.
#include <cmath>
#include <cstring>

#include "me_horn.hpp"
#include "me_internal.hpp"
#include "me_reduce.hpp"
#include "me_vd_rows.hpp"  // passes 0 - 2, shared with me_transport.hip

namespace me {
namespace {

constexpr int kVdBlocks = 1024;       // blocks of the totals pass at most; part of the order
constexpr int kVdND = 12, kVdNI = 2;  // totals: mmd [4], mmd2_u [4], gauss [4] | rows sub-sampled, pairs
typedef RedBufs<kVdND, kVdNI> VdRed;

struct VdGamma {
    double g[4];
};

// entry q of the upper triangle of a t x t tile grid, row by row: (i, j), i <= j
__device__ __forceinline__ void vd_tri_decode(long long q, long long t, int &i_out, int &j_out) {
    // row i starts at i t - i (i - 1) / 2; the estimate from the quadratic, then exact steps
    const double b = 2.0 * (double) t + 1.0;
    long long i = (long long) ((b - sqrt(b * b - 8.0 * (double) q)) * 0.5);
    if (i < 0) i = 0;
    if (i > t - 1) i = t - 1;
    while (i > 0 && i * t - i * (i - 1) / 2 > q) --i;
    while (i + 1 < t && (i + 1) * t - (i + 1) * i / 2 <= q) ++i;
    i_out = (int) i;
    j_out = (int) (i + (q - (i * t - i * (i - 1) / 2)));
}

// block r: the tiles of row r -> tiles[tile offset of r ..]: the XX block's upper triangle, the YY block's, the XY block row by row
__global__ void __launch_bounds__(256)
k_vd_tiles(VdRows R, long long M, int4 *__restrict__ tiles) {
    const long long r = blockIdx.x;
    if (r >= M) return;
    const long long *toff = R.cnt + 2 * (size_t) (M + 1);
    const long long t0 = toff[r], nt = toff[r + 1] - t0;
    const long long ti = ((long long) R.used[2 * r] + kVdT - 1) / kVdT, tj = ((long long) R.used[2 * r + 1] + kVdT - 1) / kVdT;
    const long long nxx = vd_tri(ti), nyy = vd_tri(tj);
    for (long long q = threadIdx.x; q < nt; q += 256) {
        int4 t;
        t.x = (int) r;
        if (q < nxx) {
            t.y = 0;
            vd_tri_decode(q, ti, t.z, t.w);
        } else if (q < nxx + nyy) {
            t.y = 1;
            vd_tri_decode(q - nxx, tj, t.z, t.w);
        } else {
            const long long p = q - nxx - nyy;
            t.y = 2;
            t.z = (int) (p / tj);
            t.w = (int) (p % tj);
        }
        tiles[t0 + q] = t;
    }
}

// ONE workgroup per tile, lane = point i of the i-tile: sum over the j-tile of exp(-(d2 g_b)), d2 = ((dx dx) + (dy dy)) + (dz dz)
template <int NS>
__global__ void __launch_bounds__(kVdT)
k_vd_pairs(const int4 *__restrict__ tiles, VdRows R, long long M, const double *__restrict__ X, const double *__restrict__ Y, VdGamma G,
           double *__restrict__ partial) {
    __shared__ double s_y[3 * kVdT];
    __shared__ double s_w[NS * (kVdT / 64)];
    const int4 t = tiles[blockIdx.x];
    const long long r = t.x;
    const int kind = t.y;  // 0: X x X (i < j), 1: Y x Y (i < j), 2: X x Y
    const long long xo = R.cnt[r], yo = R.cnt[(M + 1) + r];
    const int n = R.used[2 * r], m = R.used[2 * r + 1];
    const double *A = kind == 1 ? Y + 3 * yo : X + 3 * xo;
    const double *B = kind == 0 ? X + 3 * xo : Y + 3 * yo;
    const int na = kind == 1 ? m : n, nb = kind == 0 ? n : m;
    const int tid = threadIdx.x;
    const int j0 = t.w * kVdT;
    const int cnt = nb - j0 < kVdT ? nb - j0 : kVdT;  // 1 ... kVdT: a listed tile is never empty
    for (int k = tid; k < 3 * cnt; k += kVdT) s_y[k] = B[3 * (long long) j0 + k];
    const int i = t.z * kVdT + tid;
    const bool valid = i < na;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (valid) xi = A[3 * (long long) i], yi = A[3 * (long long) i + 1], zi = A[3 * (long long) i + 2];
    __syncthreads();
    double acc[NS];
#pragma unroll
    for (int b = 0; b < NS; ++b) acc[b] = 0.0;
    const bool diag = kind != 2 && t.z == t.w;
    const int wave0 = tid & ~63;
    // wave-uniform bounds: a wave past the end of the i-tile has nothing; on the diagonal tile a wave's lanes start after its first lane
    const int jb = diag ? wave0 + 1 : 0;
    const int je = (t.z * kVdT + wave0 < na) ? cnt : 0;
    const int jmin = diag ? tid + 1 : 0;  // this lane's first j: i < j
    for (int j = jb; j < je; ++j) {
        const double dx = xi - s_y[3 * j], dy = yi - s_y[3 * j + 1], dz = zi - s_y[3 * j + 2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const bool use = valid && j >= jmin;
#pragma unroll
        for (int b = 0; b < NS; ++b) {
            const double k = exp(-(d2 * G.g[b]));
            acc[b] += use ? k : 0.0;  // (+ 0.0 leaves a sum of non-negative terms as it is)
        }
    }
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int b = 0; b < NS; ++b) {
        const double v = wave_sum(acc[b]);
        if (lane == 0) s_w[b * (kVdT / 64) + w] = v;
    }
    __syncthreads();
    if (tid < NS) {
        double s = s_w[tid * (kVdT / 64)];
        for (int q = 1; q < kVdT / 64; ++q) s += s_w[tid * (kVdT / 64) + q];
        partial[(size_t) blockIdx.x * NS + tid] = s;
    }
}

// one wavefront per row: the tile partials of each of its three blocks in tile order -> ksum [ns][3], mmd2 [ns][2]
__global__ void __launch_bounds__(256)
k_vd_row_sums(VdRows R, long long M, const double *__restrict__ partial, int ns, double *__restrict__ ksum, double *__restrict__ mmd2) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const long long *toff = R.cnt + 2 * (size_t) (M + 1);
    const long long t0 = toff[r];
    const int n = R.used[2 * r], m = R.used[2 * r + 1];
    const long long ti = ((long long) n + kVdT - 1) / kVdT, tj = ((long long) m + kVdT - 1) / kVdT;
    const long long lo[3] = {t0, t0 + vd_tri(ti), t0 + vd_tri(ti) + vd_tri(tj)};
    const long long hi[3] = {lo[1], lo[2], toff[r + 1]};
    const double dn = (double) n, dm = (double) m;
    for (int b = 0; b < ns; ++b) {
        double S[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double s = 0.0;
            for (long long t = lo[k] + lane; t < hi[k]; t += 64) s += partial[(size_t) t * ns + b];
            S[k] = wave_allsum(s);
        }
        if (lane == 0) {
            double *ks = ksum + ((size_t) r * ns + b) * 3;
            ks[0] = S[0], ks[1] = S[1], ks[2] = S[2];
            const double cross = (2.0 * S[2]) / (dn * dm);
            const double u = ((2.0 * S[0]) / (dn * (dn - 1.0)) + (2.0 * S[1]) / (dm * (dm - 1.0))) - cross;
            const double bi = ((dn + 2.0 * S[0]) / (dn * dn) + (dm + 2.0 * S[1]) / (dm * dm)) - cross;
            mmd2[((size_t) r * ns + b) * 2] = u;
            mmd2[((size_t) r * ns + b) * 2 + 1] = bi;
        }
    }
}

// ---- the closed forms: 3 x 3, row-major, in this order of operations (tests/_voxdist_ref.py) ----
__device__ __forceinline__ void vd_matmul(const double *A, const double *B, double *C) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
// V diag(w) V^T
__device__ __forceinline__ void vd_compose(const double *V, const double *w, double *O) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            O[3 * r + c] = ((V[3 * r] * w[0]) * V[3 * c] + (V[3 * r + 1] * w[1]) * V[3 * c + 1]) + (V[3 * r + 2] * w[2]) * V[3 * c + 2];
}
// the symmetric part of C, jacobi_sym, the eigenvalues raised to `floor`: lam, V, ln det = (ln lam0 + ln lam1) + ln lam2
__device__ __forceinline__ double vd_decompose(const double *C, double floor_, double *lam, double *V) {
    double A[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[3 * r + c] = 0.5 * (C[3 * r + c] + C[3 * c + r]);
    jacobi_sym(3, A, lam, V);
#pragma unroll
    for (int k = 0; k < 3; ++k) lam[k] = lam[k] < floor_ ? floor_ : lam[k];
    return (log(lam[0]) + log(lam[1])) + log(lam[2]);
}
// d^T P d
__device__ __forceinline__ double vd_quad(const double *P, const double *d) {
    const double w[3] = {dot3(P, d), dot3(P + 3, d), dot3(P + 6, d)};
    return dot3(d, w);
}
// tr(P Q) = sum_r (row r of P) . (column r of Q)
__device__ __forceinline__ double vd_trace_prod(const double *P, const double *Q) {
    const double c0[3] = {Q[0], Q[3], Q[6]}, c1[3] = {Q[1], Q[4], Q[7]}, c2[3] = {Q[2], Q[5], Q[8]};
    return (dot3(P, c0) + dot3(P + 3, c1)) + dot3(P + 6, c2);
}

// one lane per row: KL(est || gt), KL(gt || est), Bhattacharyya, W2
__global__ void __launch_bounds__(256)
k_vd_gauss(VdRows R, long long M, const int *__restrict__ en, const double *__restrict__ emu, const double *__restrict__ esig,
           const int *__restrict__ gn, const double *__restrict__ gmu, const double *__restrict__ gsig, double eig_floor,
           double *__restrict__ gauss) {
    const long long r = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const long long ie = R.ei[r], ig = R.gi[r];
    const double fe = (double) (en[ie] - 1), fg = (double) (gn[ig] - 1);
    double Ce[9], Cg[9], d[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Ce[k] = esig[9 * ie + k] * fe, Cg[k] = gsig[9 * ig + k] * fg;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = gmu[3 * ig + k] - emu[3 * ie + k];
    double le[3], Ve[9], lg[3], Vg[9], w[3];
    const double lde = vd_decompose(Ce, eig_floor, le, Ve), ldg = vd_decompose(Cg, eig_floor, lg, Vg);
    double Se[9], Sg[9], Ie[9], Ig[9];
    vd_compose(Ve, le, Se);
    vd_compose(Vg, lg, Sg);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = 1.0 / le[k];
    vd_compose(Ve, w, Ie);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = 1.0 / lg[k];
    vd_compose(Vg, w, Ig);
    const double kl_eg = 0.5 * ((((vd_trace_prod(Ig, Se) + vd_quad(Ig, d)) - 3.0) + ldg) - lde);
    const double kl_ge = 0.5 * ((((vd_trace_prod(Ie, Sg) + vd_quad(Ie, d)) - 3.0) + lde) - ldg);
    // Bhattacharyya: S = (Se + Sg) / 2, decomposed the same way
    double Sm[9], ls[3], Vs[9], Is[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Sm[k] = 0.5 * (Se[k] + Sg[k]);
    const double lds = vd_decompose(Sm, eig_floor, ls, Vs);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = 1.0 / ls[k];
    vd_compose(Vs, w, Is);
    const double bd = 0.125 * vd_quad(Is, d) + 0.5 * (lds - 0.5 * (lde + ldg));
    // W2: |d|^2 + tr Se + tr Sg - 2 tr (Se^1/2 Sg Se^1/2)^1/2
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = sqrt(le[k]);
    double He[9], T1[9], Mm[9], A[9], lm[3], Vm[9];
    vd_compose(Ve, w, He);
    vd_matmul(He, Sg, T1);
    vd_matmul(T1, He, Mm);
#pragma unroll
    for (int rr = 0; rr < 3; ++rr)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[3 * rr + c] = 0.5 * (Mm[3 * rr + c] + Mm[3 * c + rr]);
    jacobi_sym(3, A, lm, Vm);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = sqrt(lm[k] > 0.0 ? lm[k] : 0.0);
    const double tre = (le[0] + le[1]) + le[2], trg = (lg[0] + lg[1]) + lg[2], trm = (w[0] + w[1]) + w[2];
    const double D = ((dot3(d, d) + tre) + trg) - 2.0 * trm;
    gauss[4 * r] = kl_eg;
    gauss[4 * r + 1] = kl_ge;
    gauss[4 * r + 2] = bd;
    gauss[4 * r + 3] = sqrt(D > 0.0 ? D : 0.0);
}

// the sums of the means over the rows: thread (b, t) takes the rows 256 b + t, + the grid's size, ... in order (me_reduce.hpp)
__global__ void __launch_bounds__(256)
k_vd_totals(VdRows R, long long M, int ns, const double *__restrict__ mmd2, const double *__restrict__ gauss, double *__restrict__ pd,
            long long *__restrict__ pi) {
    double sd[kVdND];
    long long ci[kVdNI] = {0, 0};
#pragma unroll
    for (int k = 0; k < kVdND; ++k) sd[k] = 0.0;
    for (long long r = (long long) blockIdx.x * 256 + threadIdx.x; r < M; r += (long long) gridDim.x * 256) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < ns) {
                const double u = mmd2[((size_t) r * ns + b) * 2], bi = mmd2[((size_t) r * ns + b) * 2 + 1];
                sd[b] += sqrt(bi > 0.0 ? bi : 0.0);
                sd[4 + b] += u;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) sd[8 + k] += gauss[4 * r + k];
        ci[0] += (R.stride[2 * r] > 1 || R.stride[2 * r + 1] > 1) ? 1 : 0;
        ci[1] += R.pairs[r];
    }
    red_store_partial<kVdND, kVdNI, false>(sd, ci, 0ULL, -1, ~0ULL, pd + (size_t) blockIdx.x * kVdND,
                                           pi + (size_t) blockIdx.x * VdRed::Totals::NR);
}

template <int NS>
void vd_launch_pairs(me_ctx *ctx, long long n_tiles, const int4 *tiles, const VdRows &R, long long M, const double *X, const double *Y,
                     const VdGamma &G, double *partial) {
    hipLaunchKernelGGL((k_vd_pairs<NS>), dim3((unsigned int) n_tiles), dim3(kVdT), 0, ctx->stream, tiles, R, M, X, Y, G, partial);
}

}  // namespace

int voxel_distances(me_ctx *ctx, const me_voxdist_params *p, int32_t *keys, int32_t *n_pop, int32_t *n_used, double *ksum, double *mmd2,
                    double *gauss, int64_t *n_rows, me_voxdist_out *out) {
    if (!p || !n_rows) return ctx->fail(ME_ERR_ARG, "me_voxel_distances: params or n_rows is NULL");
    if (!(p->voxel_size > 0)) return ctx->fail(ME_ERR_ARG, "me_voxel_distances: voxel_size must be > 0");
    if (p->min_pts < 11) return ctx->fail(ME_ERR_ARG, "me_voxel_distances: min_pts must be >= 11 (sigma as stored is M2 / (n - 1)^2 only for n > 10)");
    if (p->n_sigma < 1 || p->n_sigma > 4) return ctx->fail(ME_ERR_ARG, "me_voxel_distances: n_sigma must be in [1, 4]");
    for (int b = 0; b < p->n_sigma; ++b)
        if (!(p->sigma[b] > 0)) return ctx->fail(ME_ERR_ARG, "me_voxel_distances: every sigma must be > 0");
    if (p->max_points < 0 || (p->max_points >= 1 && p->max_points <= 10))
        return ctx->fail(ME_ERR_ARG, "me_voxel_distances: max_points must be 0 (all points) or >= 11");
    if (!(p->eig_floor > 0)) return ctx->fail(ME_ERR_ARG, "me_voxel_distances: eig_floor must be > 0");
    Cloud &E = ctx->cloud[ME_SLOT_EST], &G = ctx->cloud[ME_SLOT_GT];
    if (E.slab.axis >= 0 || G.slab.axis >= 0 || ctx->slab.axis >= 0 || ctx->shard_world > 1)
        return ctx->fail(ME_ERR_STATE, "me_voxel_distances: single GPU only (no slab or shard mode)");
    if (!E.uploaded || !G.uploaded) return ctx->fail(ME_ERR_STATE, "me_voxel_distances: cloud not uploaded");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const double vs = p->voxel_size;
    const int ns = p->n_sigma;
    const bool arrays = keys || n_pop || n_used || ksum || mmd2 || gauss;
    // the voxel tables me_awd_scs joins (the slots' cached tables; built here when a slot holds none of this size)
    const long long capacity = *n_rows;
    const double nan = std::nan("");
    long long M = 0;
    ME_TRY(vd_rows_count(ctx, vs, (int) p->min_pts, M));
    *n_rows = M;
    if (out) {
        std::memset(out, 0, sizeof(*out));
        out->n_rows = M;
        for (int b = 0; b < 4; ++b) out->mean_mmd[b] = out->mean_mmd2_u[b] = out->mean_gauss[b] = nan;  // (the mean of no rows, as AWD's)
    }
    if (!arrays && !out) return ME_OK;  // the count alone
    if (arrays && capacity < M) return ctx->fail(ME_ERR_CAPACITY, "me_voxel_distances: capacity too small");
    if (M == 0) return ME_OK;
    // ---- pass 0: the clouds' own orders and the rows ----
    ME_CHECK(ctx, ctx->red.ensure(std::max<size_t>(VdRed::bytes(kVdBlocks), 64)));
    VdBuilt B;
    ME_TRY(vd_rows_build(ctx, vs, (long long) p->max_points, M, "voxel_distances", "me_voxel_distances", B));
    const VdRows &R = B.R;
    const int *keys3 = B.keys3;
    const long long nx = B.tot[0], ny = B.tot[1], n_tiles = B.tot[2];
    if (n_tiles > 0x7fffffffLL)
        return ctx->fail(ME_ERR_ARG, "me_voxel_distances: more than 2^31 - 1 pair tiles (set max_points to sub-sample the fullest voxels)");
    // ---- passes 2 - 7 ----
    DevBuf &xy_d = ctx->tmp[4], &tiles_d = ctx->tmp[0], &part_d = ctx->tmp[1], &res_d = ctx->tmp[2];  // (the join's three are done with)
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ME_CHECK(ctx, xy_d.ensure((size_t) (nx + ny) * 24));
    ME_CHECK(ctx, tiles_d.ensure((size_t) n_tiles * 16));
    ME_CHECK(ctx, part_d.ensure((size_t) n_tiles * ns * 8));
    ME_CHECK(ctx, res_d.ensure((size_t) M * (ns * 5 + 4) * 8));  // ksum [M][ns][3] | mmd2 [M][ns][2] | gauss [M][4]
    double *X = xy_d.as<double>(), *Y = X + 3 * nx;
    double *ksum_d = res_d.as<double>(), *mmd2_d = ksum_d + (size_t) M * ns * 3, *gauss_d = mmd2_d + (size_t) M * ns * 2;
    VdGamma Gm;
    for (int b = 0; b < 4; ++b) Gm.g[b] = b < ns ? 1.0 / (2.0 * p->sigma[b] * p->sigma[b]) : 0.0;
    const int nb = (int) std::min<long long>(kVdBlocks, blocks_of(M));
    const VdRed red(ctx, kVdBlocks);
    {
        TimerScope ts(ctx, "voxel_distances");
        vd_gather_launch(ctx, B, M, X, Y);
        hipLaunchKernelGGL(k_vd_tiles, dim3((unsigned int) M), dim3(256), 0, ctx->stream, R, M, tiles_d.as<int4>());
        const int4 *tl = tiles_d.as<int4>();
        double *pt = part_d.as<double>();
        switch (ns) {
            case 1: vd_launch_pairs<1>(ctx, n_tiles, tl, R, M, X, Y, Gm, pt); break;
            case 2: vd_launch_pairs<2>(ctx, n_tiles, tl, R, M, X, Y, Gm, pt); break;
            case 3: vd_launch_pairs<3>(ctx, n_tiles, tl, R, M, X, Y, Gm, pt); break;
            default: vd_launch_pairs<4>(ctx, n_tiles, tl, R, M, X, Y, Gm, pt); break;
        }
        hipLaunchKernelGGL(k_vd_row_sums, dim3((unsigned int) ((M + 3) / 4)), dim3(256), 0, ctx->stream, R, M, (const double *) pt, ns, ksum_d,
                           mmd2_d);
        hipLaunchKernelGGL(k_vd_gauss, dim3(blocks_of(M)), dim3(256), 0, ctx->stream, R, M, (const int *) E.vox_n.as<int>(),
                           (const double *) E.vox_mu.as<double>(), (const double *) E.vox_sigma.as<double>(), (const int *) G.vox_n.as<int>(),
                           (const double *) G.vox_mu.as<double>(), (const double *) G.vox_sigma.as<double>(), p->eig_floor, gauss_d);
        hipLaunchKernelGGL(k_vd_totals, dim3(nb), dim3(256), 0, ctx->stream, R, M, ns, (const double *) mmd2_d, (const double *) gauss_d, red.pd,
                           red.pi);
        red.total(ctx, nb, red.tot);
    }
    ME_CHECK(ctx, hipGetLastError());
    VdRed::Totals h;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h, red.tot, sizeof(h)));
        ME_TRY(mg.sync());  // (the local buffers die with this frame: the stream is idle from here on)
    }
    if (keys) ME_TRY(copy_d2h(ctx, keys, keys3, (size_t) M * 12));
    if (n_pop) ME_TRY(copy_d2h(ctx, n_pop, R.pop, (size_t) M * 8));
    if (n_used) ME_TRY(copy_d2h(ctx, n_used, R.used, (size_t) M * 8));
    if (ksum) ME_TRY(copy_d2h(ctx, ksum, ksum_d, (size_t) M * ns * 24));
    if (mmd2) ME_TRY(copy_d2h(ctx, mmd2, mmd2_d, (size_t) M * ns * 16));
    if (gauss) ME_TRY(copy_d2h(ctx, gauss, gauss_d, (size_t) M * 32));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (out) {
        const double dM = (double) M;
        out->n_rows_subsampled = h.i[0];
        out->n_pairs = h.i[1];
        for (int b = 0; b < ns; ++b) {
            out->mean_mmd[b] = h.d[b] / dM;
            out->mean_mmd2_u[b] = h.d[4 + b] / dM;
        }
        for (int k = 0; k < 4; ++k) out->mean_gauss[k] = h.d[8 + k] / dM;
    }
    return ME_OK;
}

}  // namespace me
