// me_transport.hip — per-voxel point-set Wasserstein distances on the AWD lattice (me_voxel_transport): the sliced 2-Wasserstein
// distance, exact per direction, and the debiased Sinkhorn divergence on a fixed eps schedule.  DESIGN.md section 4.26; the
// definitions and every order of summation: include/mapeval_hip.h; the restatement: tests/_transport_ref.py.
//   passes 0 - 2  me_vd_rows.hpp     the rows of the AWD table, their used points, contiguous fp64 xyz per cloud (as me_voxdist.hip)
//   pass 3  k_vt_sliced              ONE workgroup per (row, direction): both sides projected into LDS (padded with +inf to a power of
//                                    two), a bitonic sort of each, then the interval merge with integer overlaps
//   pass 4  k_vt_sinkhorn            ONE workgroup per (row, problem), problem = (X, Y), (X, X), (Y, Y).  The point sets and the
//                                    potentials stay in LDS as records (x, y, z, potential) for all T iterations; a lane owns the entries
//                                    lane, lane + 256, ... of the side being updated and streams the other side at one address per step
//                                    (a broadcast read); C_ij is recomputed in every pass
//   pass 5  k_vt_row_out             one lane per row: the sliced summary and S
//   pass 6  k_vt_totals              the means' sums over the rows in key order by the shared fixed-order reduction (me_reduce.hpp)
// No floating-point atomics anywhere.
#include <cmath>
#include <cstring>

#include "me_internal.hpp"
#include "me_reduce.hpp"
#include "me_vd_rows.hpp"

namespace me {
namespace {

constexpr int kVtBlocks = 1024;     // blocks of the totals pass at most; part of the order
constexpr int kVtND = 5, kVtNI = 2;  // totals: sw2, sqrt(max_sw2_sq), S, sqrt(max(0, S)), marginal_err | rows sub-sampled, pairs
typedef RedBufs<kVtND, kVtNI> VtRed;
constexpr int kVtMaxPoints = 1024;  // used points per side at most: 4 entries per lane, 64 KiB of records per workgroup
constexpr int kVtOwn = kVtMaxPoints / 256;

// ascending bitonic sort of s[0 .. P), P a power of two >= 2, by all 256 threads of the block
__device__ __forceinline__ void vt_bitonic(double *s, int P) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const bool up = (i & k) == 0;
                const double a = s[i], b = s[i + j];
                if ((a > b) == up) s[i] = b, s[i + j] = a;
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int vt_pow2(int n) {
    int P = 2;
    while (P < n) P <<= 1;
    return P;
}

// block (r, l): W2^2 of the projections of row r on direction l -> w2[r][l]
__global__ void __launch_bounds__(256)
k_vt_sliced(VdRows R, long long M, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ dirs, int L,
            double *__restrict__ w2) {
    __shared__ double s_a[kVtMaxPoints], s_b[kVtMaxPoints];
    __shared__ double s_red[4];
    const long long r = blockIdx.x;
    const int l = blockIdx.y;
    const int n = R.used[2 * r], m = R.used[2 * r + 1];
    if (n > kVtMaxPoints || m > kVtMaxPoints) return;  // (never: max_points <= 1024)
    const double *A = X + 3 * R.cnt[r], *B = Y + 3 * R.cnt[(M + 1) + r];
    const double ux = dirs[3 * l], uy = dirs[3 * l + 1], uz = dirs[3 * l + 2];
    const int Pa = vt_pow2(n), Pb = vt_pow2(m);
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    for (int i = threadIdx.x; i < Pa; i += 256) s_a[i] = i < n ? (A[3 * i] * ux + A[3 * i + 1] * uy) + A[3 * i + 2] * uz : inf;
    for (int j = threadIdx.x; j < Pb; j += 256) s_b[j] = j < m ? (B[3 * j] * ux + B[3 * j + 1] * uy) + B[3 * j + 2] * uz : inf;
    __syncthreads();
    vt_bitonic(s_a, Pa);
    vt_bitonic(s_b, Pb);
    // in units of 1 / (n m): atom i of X covers [i m, (i + 1) m), atom j of Y covers [j n, (j + 1) n)
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const long long lo = (long long) i * m, hi = lo + m;
        const double a = s_a[i];
        for (int j = (int) (lo / n); j < m && (long long) j * n < hi; ++j) {
            const long long b0 = (long long) j * n, b1 = b0 + n;
            const long long w = (hi < b1 ? hi : b1) - (lo > b0 ? lo : b0);
            const double d = a - s_b[j];
            acc += (double) w * (d * d);
        }
    }
    const double S = block_sum_256(acc, s_red);
    if (threadIdx.x == 0) w2[(size_t) r * L + l] = S / ((double) n * (double) m);
}

// -eps (M + log sum_j exp(t_j - M)), t_j = lq + (q[j].pot - C_j) / eps, M = max_j t_j, over the nq records q (x, y, z, pot), j ascending
__device__ __forceinline__ double vt_softmin(const double *__restrict__ q, int nq, double xi, double yi, double zi, double lq, double eps) {
    double mx = __longlong_as_double(0xfff0000000000000LL);  // -inf
    for (int j = 0; j < nq; ++j) {
        const double dx = xi - q[4 * j], dy = yi - q[4 * j + 1], dz = zi - q[4 * j + 2];
        const double c = (dx * dx + dy * dy) + dz * dz;
        const double t = lq + (q[4 * j + 3] - c) / eps;
        mx = t > mx ? t : mx;
    }
    double s = 0.0;
    for (int j = 0; j < nq; ++j) {
        const double dx = xi - q[4 * j], dy = yi - q[4 * j + 1], dz = zi - q[4 * j + 2];
        const double c = (dx * dx + dy * dy) + dz * dz;
        const double t = lq + (q[4 * j + 3] - c) / eps;
        s += exp(t - mx);
    }
    return -eps * (mx + log(s));
}

// the sum of the potentials of the np records p: lane t takes t, t + 256, ... ascending, then block_sum_256 (valid in thread 0)
__device__ __forceinline__ double vt_pot_sum(const double *p, int np, double *s_red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) s += p[4 * i + 3];
    return block_sum_256(s, s_red);
}

// block 3 r + kind: kind 0 the cross problem (X, Y), 1 (X, X), 2 (Y, Y) of row r -> ot[r][kind]; kind 0 also merr[r] and the potentials
__global__ void __launch_bounds__(256)
k_vt_sinkhorn(VdRows R, long long M, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ eps_s, int T,
              double *__restrict__ ot, double *__restrict__ merr, double *__restrict__ fpot, double *__restrict__ gpot) {
    extern __shared__ __align__(16) double s_dyn[];  // [4] the block sums' scratch | [na] records of the first side | [nb] of the second (cross only)
    const long long r = blockIdx.x / 3;
    const int kind = (int) (blockIdx.x % 3);
    const int n = R.used[2 * r], m = R.used[2 * r + 1];
    if (n > kVtMaxPoints || m > kVtMaxPoints) return;  // (never: max_points <= 1024)
    const long long xo = R.cnt[r], yo = R.cnt[(M + 1) + r];
    const double *A = kind == 2 ? Y + 3 * yo : X + 3 * xo;
    const double *B = Y + 3 * yo;  // (read when kind == 0)
    const int na = kind == 2 ? m : n, nb = kind == 0 ? m : na;
    double *s_red = s_dyn, *sa = s_dyn + 4, *sb = kind == 0 ? sa + 4 * (size_t) na : sa;
    const int tid = threadIdx.x;
    for (int i = tid; i < na; i += 256) sa[4 * i] = A[3 * i], sa[4 * i + 1] = A[3 * i + 1], sa[4 * i + 2] = A[3 * i + 2], sa[4 * i + 3] = 0.0;
    if (kind == 0)
        for (int j = tid; j < nb; j += 256) sb[4 * j] = B[3 * j], sb[4 * j + 1] = B[3 * j + 1], sb[4 * j + 2] = B[3 * j + 2], sb[4 * j + 3] = 0.0;
    __syncthreads();
    const double la = -log((double) na), lb = -log((double) nb);
    if (kind == 0) {
        for (int t = 0; t < T; ++t) {
            const double eps = eps_s[t];
            // f from g: a lane writes only the potentials of its own records, which nobody reads in this half
            for (int i = tid; i < na; i += 256) sa[4 * i + 3] = vt_softmin(sb, nb, sa[4 * i], sa[4 * i + 1], sa[4 * i + 2], lb, eps);
            __syncthreads();
            for (int j = tid; j < nb; j += 256) sb[4 * j + 3] = vt_softmin(sa, na, sb[4 * j], sb[4 * j + 1], sb[4 * j + 2], la, eps);
            __syncthreads();
        }
        // the first marginal of the plan at the last eps
        const double eps = eps_s[T - 1], lab = la + lb, wa = 1.0 / (double) na;
        double e = 0.0;
        for (int i = tid; i < na; i += 256) {
            const double xi = sa[4 * i], yi = sa[4 * i + 1], zi = sa[4 * i + 2], fi = sa[4 * i + 3];
            double rs = 0.0;
            for (int j = 0; j < nb; ++j) {
                const double dx = xi - sb[4 * j], dy = yi - sb[4 * j + 1], dz = zi - sb[4 * j + 2];
                const double c = (dx * dx + dy * dy) + dz * dz;
                rs += exp(lab + ((fi + sb[4 * j + 3]) - c) / eps);
            }
            e += fabs(rs - wa);
        }
        const double et = block_sum_256(e, s_red);
        const double sf = vt_pot_sum(sa, na, s_red);
        const double sg = vt_pot_sum(sb, nb, s_red);
        if (tid == 0) {
            ot[3 * r] = sf / (double) na + sg / (double) nb;
            merr[r] = et;
        }
        if (fpot) {
            for (int i = tid; i < na; i += 256) fpot[xo + i] = sa[4 * i + 3];
            for (int j = tid; j < nb; j += 256) gpot[yo + j] = sb[4 * j + 3];
        }
    } else {
        for (int t = 0; t < T; ++t) {
            const double eps = eps_s[t];
            double nv[kVtOwn];
#pragma unroll
            for (int k = 0; k < kVtOwn; ++k) {
                const int i = tid + 256 * k;
                nv[k] = 0.0;
                if (i < na) nv[k] = 0.5 * (sa[4 * i + 3] + vt_softmin(sa, na, sa[4 * i], sa[4 * i + 1], sa[4 * i + 2], la, eps));
            }
            __syncthreads();  // every lane has read the potentials of the iteration before
#pragma unroll
            for (int k = 0; k < kVtOwn; ++k) {
                const int i = tid + 256 * k;
                if (i < na) sa[4 * i + 3] = nv[k];
            }
            __syncthreads();
        }
        const double sf = vt_pot_sum(sa, na, s_red);
        if (tid == 0) ot[3 * r + kind] = sf / (double) na + sf / (double) na;
    }
}

// one lane per row: sliced[r] = sw2_sq, sw2, max_sw2_sq, its direction | sink[r] = the three OT values, S, sqrt(max(0, S)), marginal_err
__global__ void __launch_bounds__(256)
k_vt_row_out(long long M, int L, int T, const double *__restrict__ w2, const double *__restrict__ ot, const double *__restrict__ merr,
             double *__restrict__ sliced, double *__restrict__ sink) {
    const long long r = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    if (L > 0) {
        const double *w = w2 + (size_t) r * L;
        double s = 0.0, mx = w[0];
        int arg = 0;
        for (int l = 0; l < L; ++l) {
            const double v = w[l];
            s += v;
            if (v > mx) mx = v, arg = l;
        }
        const double q = s / (double) L;
        sliced[4 * r] = q, sliced[4 * r + 1] = sqrt(q), sliced[4 * r + 2] = mx, sliced[4 * r + 3] = (double) arg;
    }
    if (T > 0) {
        const double oxy = ot[3 * r], oxx = ot[3 * r + 1], oyy = ot[3 * r + 2];
        const double S = (oxy - 0.5 * oxx) - 0.5 * oyy;
        double *o = sink + 6 * r;
        o[0] = oxy, o[1] = oxx, o[2] = oyy, o[3] = S, o[4] = sqrt(S > 0.0 ? S : 0.0), o[5] = merr[r];
    }
}

// the sums of the means over the rows: thread (b, t) takes the rows 256 b + t, + the grid's size, ... in order (me_reduce.hpp); the
// largest marginal_err and its row (a non-negative double orders as its bits do)
__global__ void __launch_bounds__(256)
k_vt_totals(VdRows R, long long M, int L, int T, const double *__restrict__ sliced, const double *__restrict__ sink, double *__restrict__ pd,
            long long *__restrict__ pi) {
    double sd[kVtND];
    long long ci[kVtNI] = {0, 0};
#pragma unroll
    for (int k = 0; k < kVtND; ++k) sd[k] = 0.0;
    unsigned long long mx = 0ull;
    long long arg = -1;
    for (long long r = (long long) blockIdx.x * 256 + threadIdx.x; r < M; r += (long long) gridDim.x * 256) {
        if (L > 0) {
            sd[0] += sliced[4 * r + 1];
            sd[1] += sqrt(sliced[4 * r + 2]);
        }
        if (T > 0) {
            sd[2] += sink[6 * r + 3];
            sd[3] += sink[6 * r + 4];
            const double e = sink[6 * r + 5];
            sd[4] += e;
            take_max(mx, arg, (unsigned long long) __double_as_longlong(e >= 0.0 ? e : 0.0), r);
        }
        ci[0] += (R.stride[2 * r] > 1 || R.stride[2 * r + 1] > 1) ? 1 : 0;
        ci[1] += (long long) R.used[2 * r] * R.used[2 * r + 1];
    }
    red_store_partial<kVtND, kVtNI, false>(sd, ci, mx, arg, ~0ULL, pd + (size_t) blockIdx.x * kVtND, pi + (size_t) blockIdx.x * VtRed::Totals::NR);
}

}  // namespace

int voxel_transport(me_ctx *ctx, const me_voxtrans_params *p, const double *directions, const double *eps_schedule, int32_t *keys,
                    int32_t *n_pop, int32_t *n_used, double *sliced, double *sinkhorn, double *per_direction, double *potentials,
                    int64_t *n_rows, me_voxtrans_out *out) {
    if (!p || !n_rows) return ctx->fail(ME_ERR_ARG, "me_voxel_transport: params or n_rows is NULL");
    if (!(p->voxel_size > 0)) return ctx->fail(ME_ERR_ARG, "me_voxel_transport: voxel_size must be > 0");
    if (p->min_pts < 11) return ctx->fail(ME_ERR_ARG, "me_voxel_transport: min_pts must be >= 11 (the rows of me_voxel_distances)");
    const int L = p->n_dir, T = p->n_eps;
    if (L < 0 || L > 64) return ctx->fail(ME_ERR_ARG, "me_voxel_transport: n_dir must be in [0, 64]");
    if (T < 0 || T > 512) return ctx->fail(ME_ERR_ARG, "me_voxel_transport: n_eps must be in [0, 512]");
    if (L == 0 && T == 0) return ctx->fail(ME_ERR_ARG, "me_voxel_transport: n_dir and n_eps are both 0");
    if (L > 0 && !directions) return ctx->fail(ME_ERR_ARG, "me_voxel_transport: directions is NULL");
    if (T > 0 && !eps_schedule) return ctx->fail(ME_ERR_ARG, "me_voxel_transport: eps_schedule is NULL");
    for (int t = 0; t < T; ++t)
        if (!(eps_schedule[t] > 0) || (t > 0 && !(eps_schedule[t] <= eps_schedule[t - 1])))
            return ctx->fail(ME_ERR_ARG, "me_voxel_transport: eps_schedule must be positive and non-increasing");
    if (p->max_points < 11 || p->max_points > kVtMaxPoints) return ctx->fail(ME_ERR_ARG, "me_voxel_transport: max_points must be in [11, 1024]");
    Cloud &E = ctx->cloud[ME_SLOT_EST], &G = ctx->cloud[ME_SLOT_GT];
    if (E.slab.axis >= 0 || G.slab.axis >= 0 || ctx->slab.axis >= 0 || ctx->shard_world > 1)
        return ctx->fail(ME_ERR_STATE, "me_voxel_transport: single GPU only (no slab or shard mode)");
    if (!E.uploaded || !G.uploaded) return ctx->fail(ME_ERR_STATE, "me_voxel_transport: cloud not uploaded");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const double vs = p->voxel_size;
    const bool solve = sliced || sinkhorn || per_direction || potentials || out;
    const bool arrays = keys || n_pop || n_used || sliced || sinkhorn || per_direction || potentials;
    const long long capacity = *n_rows;
    const double nan = std::nan("");
    long long M = 0;
    ME_TRY(vd_rows_count(ctx, vs, (int) p->min_pts, M));
    *n_rows = M;
    if (out) {
        std::memset(out, 0, sizeof(*out));
        out->n_rows = M;
        out->max_marginal_row = -1;
        out->mean_sw2 = out->mean_max_sw2 = out->mean_s = out->mean_sinkhorn = out->mean_marginal_err = out->max_marginal_err = nan;
    }
    if (!arrays && !out) return ME_OK;  // the count alone
    if (arrays && capacity < M) return ctx->fail(ME_ERR_CAPACITY, "me_voxel_transport: capacity too small");
    if (M == 0) return ME_OK;
    // ---- passes 0 and 1 ----
    ME_CHECK(ctx, ctx->red.ensure(std::max<size_t>(VtRed::bytes(kVtBlocks), 64)));
    VdBuilt B;
    ME_TRY(vd_rows_build(ctx, vs, (long long) p->max_points, M, "voxel_transport", "me_voxel_transport", B));
    const VdRows &R = B.R;
    const long long nx = B.tot[0], ny = B.tot[1];
    VtRed::Totals h;
    std::memset(&h, 0, sizeof(h));
    double *res_host_src[4] = {nullptr, nullptr, nullptr, nullptr};  // device: sliced, sinkhorn, per_direction, potentials
    if (solve) {
        DevBuf &xy_d = ctx->tmp[4], &in_d = ctx->tmp[0], &pot_d = ctx->tmp[1], &res_d = ctx->tmp[2];  // (the join's three are done with)
        ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        ME_CHECK(ctx, xy_d.ensure((size_t) (nx + ny) * 24));
        ME_CHECK(ctx, in_d.ensure((size_t) (3 * L + T + 1) * 8));
        ME_CHECK(ctx, pot_d.ensure((size_t) (nx + ny + 1) * 8));
        // w2 [M][L] | ot [M][3] | merr [M] | sliced [M][4] | sink [M][6]
        ME_CHECK(ctx, res_d.ensure((size_t) M * (L + 3 + 1 + 4 + 6) * 8));
        double *X = xy_d.as<double>(), *Y = X + 3 * nx;
        double *dirs_d = in_d.as<double>(), *eps_d = dirs_d + 3 * L;
        double *w2_d = res_d.as<double>(), *ot_d = w2_d + (size_t) M * L, *merr_d = ot_d + (size_t) M * 3, *sliced_d = merr_d + M,
               *sink_d = sliced_d + (size_t) M * 4;
        double *fpot_d = potentials ? pot_d.as<double>() : nullptr, *gpot_d = potentials ? fpot_d + nx : nullptr;
        if (L > 0) ME_TRY(copy_h2d(ctx, dirs_d, directions, (size_t) L * 24));
        if (T > 0) ME_TRY(copy_h2d(ctx, eps_d, eps_schedule, (size_t) T * 8));
        const size_t lds = (size_t) (4 + 8 * p->max_points) * 8;  // the scratch and two sides of max_points records at most
        if (T > 0 && lds > 64 * 1024)
            ME_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_vt_sinkhorn), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        const int nb = (int) std::min<long long>(kVtBlocks, blocks_of(M));
        const VtRed red(ctx, kVtBlocks);
        {
            TimerScope ts(ctx, "voxel_transport");
            vd_gather_launch(ctx, B, M, X, Y);
            if (L > 0)
                hipLaunchKernelGGL(k_vt_sliced, dim3((unsigned int) M, (unsigned int) L), dim3(256), 0, ctx->stream, R, M, (const double *) X,
                                   (const double *) Y, (const double *) dirs_d, L, w2_d);
            if (T > 0)
                hipLaunchKernelGGL(k_vt_sinkhorn, dim3((unsigned int) (3 * M)), dim3(256), lds, ctx->stream, R, M, (const double *) X,
                                   (const double *) Y, (const double *) eps_d, T, ot_d, merr_d, fpot_d, gpot_d);
            hipLaunchKernelGGL(k_vt_row_out, dim3(blocks_of(M)), dim3(256), 0, ctx->stream, M, L, T, (const double *) w2_d, (const double *) ot_d,
                               (const double *) merr_d, sliced_d, sink_d);
            hipLaunchKernelGGL(k_vt_totals, dim3(nb), dim3(256), 0, ctx->stream, R, M, L, T, (const double *) sliced_d, (const double *) sink_d,
                               red.pd, red.pi);
            red.total(ctx, nb, red.tot);
        }
        ME_CHECK(ctx, hipGetLastError());
        {
            MailGuard mg(ctx);
            ME_TRY(mail_post(ctx, &h, red.tot, sizeof(h)));
            ME_TRY(mg.sync());
        }
        res_host_src[0] = sliced_d, res_host_src[1] = sink_d, res_host_src[2] = w2_d, res_host_src[3] = pot_d.as<double>();
    }
    if (keys) ME_TRY(copy_d2h(ctx, keys, B.keys3, (size_t) M * 12));
    if (n_pop) ME_TRY(copy_d2h(ctx, n_pop, R.pop, (size_t) M * 8));
    if (n_used) ME_TRY(copy_d2h(ctx, n_used, R.used, (size_t) M * 8));
    if (sliced && L > 0) ME_TRY(copy_d2h(ctx, sliced, res_host_src[0], (size_t) M * 32));
    if (sinkhorn && T > 0) ME_TRY(copy_d2h(ctx, sinkhorn, res_host_src[1], (size_t) M * 48));
    if (per_direction && L > 0) ME_TRY(copy_d2h(ctx, per_direction, res_host_src[2], (size_t) M * L * 8));
    if (potentials && T > 0) ME_TRY(copy_d2h(ctx, potentials, res_host_src[3], (size_t) (nx + ny) * 8));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the local buffers of B die with this frame: the stream is idle from here on)
    if (out) {
        const double dM = (double) M;
        out->n_rows_subsampled = h.i[0];
        out->n_pairs = h.i[1];
        out->n_used_est = nx;
        out->n_used_gt = ny;
        if (L > 0) out->mean_sw2 = h.d[0] / dM, out->mean_max_sw2 = h.d[1] / dM;
        if (T > 0) {
            out->mean_s = h.d[2] / dM, out->mean_sinkhorn = h.d[3] / dM, out->mean_marginal_err = h.d[4] / dM;
            out->max_marginal_row = h.i[kVtNI + 1];
            if (h.i[kVtNI + 1] >= 0) std::memcpy(&out->max_marginal_err, &h.i[kVtNI], 8);
        }
    }
    return ME_OK;
}

}  // namespace me
