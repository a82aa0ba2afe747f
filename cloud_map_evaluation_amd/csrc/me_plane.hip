// me_plane.hip — RANSAC plane segmentation and multi-plane extraction on a resident single-GPU cloud (Open3D's
// PointCloud::SegmentPlane as the model; the definition is in include/mapeval_hip.h).  Per round r:
//   k_plane_compact  the remaining points (flag = not yet labelled, cloud order -> rem[] by the shared stream compaction) copied into
//                    three contiguous coordinate arrays, padded with NaN to a whole tile: the scoring kernel streams, it never gathers
//                    and never checks a bound (a NaN point is no inlier of any plane)
//   k_plane_hyp      one lane per hypothesis: Philox (h, 5, r, 0) -> three remaining points, the two validity checks, the unit normal
//                    with the sign rule, d.  An invalid hypothesis stores (0, 0, 0, +inf): it counts nothing
//   k_plane_score    THE HOT KERNEL.  A block holds kPlTile = 1024 points in registers (four consecutive points per lane, wide loads) and
//                    walks kPlHyp hypotheses; the plane of a hypothesis is wave-uniform (scalar loads).  Per (point, hypothesis): three
//                    multiplications and three additions in fp64, in the order of the definition, and one compare of |s| against t whose
//                    mask goes through the scalar population count.  The wave's count of hypothesis j is parked in lane j of one
//                    register (a compare and a select: this compiler has no v_writelane builtin), 64 hypotheses later it is added to
//                    the block's LDS counters, and at the end of the block one integer atomic per (block, hypothesis) goes to memory:
//                    exact and independent of the order
//   k_plane_best     the largest score, ties to the smallest h; the scores of the round as int64 (-1 = invalid) for the caller
//   k_plane_label    the winner's inliers get their label (and leave the remaining set); M1, M2 about the winner's p0 and the largest
//                    |p - p0|^2 as per-block partials
//   k_plane_reduce   block partials in block order (256 chunks, then one block): fixed order, bit-identical from run to run
//   k_plane_refit    one thread: C, cyclic Jacobi (me_horn.hpp), the degeneracy test, sign rule, d
//   k_plane_resid    sum s^2, sum |s|, max |s| of the round's inliers against the RETURNED plane, per-block partials
// The file is compiled with -ffp-contract=off: tests/_plane_ref.py restates every expression.
#include <algorithm>
#include <cmath>

#include "me_horn.hpp"
#include "me_internal.hpp"
#include "me_philox.hpp"

namespace me {

namespace {

#ifndef ME_TUNE_PLANE_PTS
#define ME_TUNE_PLANE_PTS 4  // k_plane_score: points per lane (even).  4: 58 VGPRs, 8 waves per SIMD; 8: 82 VGPRs, 5 waves
#endif
constexpr int kPlPts = ME_TUNE_PLANE_PTS;  // points per lane of k_plane_score
constexpr int kPlTile = 256 * kPlPts;    // points per block tile
constexpr int kPlHyp = 256;              // hypotheses per blockIdx.y
constexpr unsigned int kPlMaxBlocksX = 2048;  // point blocks of k_plane_score: above it a block walks several tiles (fewer global atomics)
constexpr long long kPlMaxHyp = 1ll << 24;
constexpr int kPlStage = 256;
constexpr int kPlRows = 10;              // M1 (3), M2 xx xy xz yy yz zz (6), max |p - o|^2

struct PlaneHyp {
    double a, b, c, d;
};

__global__ void __launch_bounds__(256) k_plane_init(long long n, int *__restrict__ labels, unsigned char *__restrict__ flag) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    labels[i] = -1;
    flag[i] = 1;
}

// k < m: the k-th remaining point; m <= k < m_pad: NaN
__global__ void __launch_bounds__(256) k_plane_compact(const double *__restrict__ xyz, const unsigned int *__restrict__ rem, long long m,
                                                       long long m_pad, double *__restrict__ xs, double *__restrict__ ys, double *__restrict__ zs) {
    const long long k = (long long) blockIdx.x * 256 + threadIdx.x;
    if (k >= m_pad) return;
    double x = NAN, y = NAN, z = NAN;
    if (k < m) {
        const size_t i = rem[k];
        x = xyz[3 * i];
        y = xyz[3 * i + 1];
        z = xyz[3 * i + 2];
    }
    xs[k] = x;
    ys[k] = y;
    zs[k] = z;
}

// The sign rule, as one predicate without short-circuit branches and three selects (the nested-branch form was compiled into a flow
// whose flip of the c == 0 cases was empty: found by the lattice test, whose normals are full of signed zeros).
__device__ __forceinline__ void plane_sign(double *nrm) {
    const double a = nrm[0], b = nrm[1], c = nrm[2];
    const bool flip = (c < 0) | ((c == 0) & ((b < 0) | ((b == 0) & (a < 0))));
    nrm[0] = flip ? -a : a;
    nrm[1] = flip ? -b : b;
    nrm[2] = flip ? -c : c;
}

__global__ void __launch_bounds__(256) k_plane_hyp(long long nh, u64 seed, u64 round, u64 m, const double *__restrict__ xs,
                                                   const double *__restrict__ ys, const double *__restrict__ zs, PlaneHyp *__restrict__ hyp,
                                                   unsigned int *__restrict__ k0_out, unsigned char *__restrict__ valid,
                                                   unsigned int *__restrict__ score) {
    const long long h = (long long) blockIdx.x * 256 + threadIdx.x;
    if (h >= nh) return;
    u64 w[4];
    philox_block(seed, (u64) h, 5, round, w);
    const u64 s0 = mulhi64(w[0], m), s1 = mulhi64(w[1], m), s2 = mulhi64(w[2], m);
    PlaneHyp out = {0.0, 0.0, 0.0, INFINITY};
    bool ok = s0 != s1 && s0 != s2 && s1 != s2;  // (m < 3: two always coincide, and nothing is read)
    if (ok) {
        const double p0[3] = {xs[s0], ys[s0], zs[s0]}, p1[3] = {xs[s1], ys[s1], zs[s1]}, p2[3] = {xs[s2], ys[s2], zs[s2]};
        const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        double cr[3];
        cross3(e1, e2, cr);
        const double cc = dot3(cr, cr);
        if (cc <= (1e-12 * dot3(e1, e1)) * dot3(e2, e2)) ok = false;  // the rule of k_ransac_hyp
        if (ok) {
            const double L = sqrt(cc);
            double nrm[3] = {cr[0] / L, cr[1] / L, cr[2] / L};
            plane_sign(nrm);
            out.a = nrm[0];
            out.b = nrm[1];
            out.c = nrm[2];
            out.d = -((nrm[0] * p0[0] + nrm[1] * p0[1]) + nrm[2] * p0[2]);
        }
    }
    hyp[h] = out;
    k0_out[h] = ok ? (unsigned int) s0 : 0u;
    valid[h] = ok ? 1 : 0;
    score[h] = 0u;
}

// grid (point blocks, hypothesis chunks of kPlHyp).  m_pad is a multiple of kPlTile; block x walks the tiles x * tiles_per_block ...
// 58 VGPRs, 46 SGPRs, no scratch, 1 KB of LDS (the counters), 8 waves per SIMD.  The inner loop is 28 fp64 vector instructions (6 per
// test and the compare) and 3 32-bit ones per four tests of a lane: bound by the fp64 issue rate; the points of a tile are read once
// per kPlHyp hypotheses.
__global__ void __launch_bounds__(256)
k_plane_score(const double *__restrict__ xs, const double *__restrict__ ys, const double *__restrict__ zs, long long m_pad, int tiles_per_block,
              const PlaneHyp *__restrict__ hyp, int nh_total, double t, unsigned int *__restrict__ score) {
    __shared__ unsigned int s_cnt[kPlHyp];
    const int lane = threadIdx.x & 63;
    const int h0 = blockIdx.y * kPlHyp;
    const int nh = nh_total - h0 < kPlHyp ? nh_total - h0 : kPlHyp;
    s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    for (int c = 0; c < tiles_per_block; ++c) {
        const long long base = ((long long) blockIdx.x * tiles_per_block + c) * kPlTile;
        if (base >= m_pad) break;
        const size_t p = (size_t) base + (size_t) threadIdx.x * kPlPts;
        double x[kPlPts], y[kPlPts], z[kPlPts];
#pragma unroll
        for (int q = 0; q < kPlPts; q += 2) {  // (16-byte loads: a lane's points are consecutive)
            const double2 vx = *reinterpret_cast<const double2 *>(xs + p + q), vy = *reinterpret_cast<const double2 *>(ys + p + q),
                          vz = *reinterpret_cast<const double2 *>(zs + p + q);
            x[q] = vx.x, x[q + 1] = vx.y;
            y[q] = vy.x, y[q + 1] = vy.y;
            z[q] = vz.x, z[q + 1] = vz.y;
        }
        for (int j0 = 0; j0 < nh; j0 += 64) {
            const int jn = nh - j0 < 64 ? nh - j0 : 64;
            int acc = 0;  // lane j: this wave's count of hypothesis h0 + j0 + j
            for (int j = 0; j < jn; ++j) {
                const PlaneHyp pl = hyp[h0 + j0 + j];  // wave-uniform address: scalar loads
                int cnt = 0;
#pragma unroll
                for (int q = 0; q < kPlPts; ++q) {
                    const double s = ((pl.a * x[q] + pl.b * y[q]) + pl.c * z[q]) + pl.d;
                    cnt += __popcll(__ballot(fabs(s) < t));  // the compare mask through the scalar population count
                }
                acc = lane == j ? cnt : acc;
            }
            if (lane < jn && acc) atomicAdd(&s_cnt[j0 + lane], (unsigned int) acc);
        }
    }
    __syncthreads();
    if ((int) threadIdx.x < nh && s_cnt[threadIdx.x]) atomicAdd(&score[h0 + threadIdx.x], s_cnt[threadIdx.x]);
}

// one block.  out[0] = the winning h (-1: no valid hypothesis), out[1] = its score, out[2] = the valid hypotheses; win = its plane and
// its p0; scores64[h] = score or -1
__global__ void __launch_bounds__(256)
k_plane_best(const unsigned int *__restrict__ score, const unsigned char *__restrict__ valid, long long nh, const PlaneHyp *__restrict__ hyp,
             const unsigned int *__restrict__ k0, const double *__restrict__ xs, const double *__restrict__ ys, const double *__restrict__ zs,
             long long *__restrict__ scores64, long long *__restrict__ out, double *__restrict__ win) {
    __shared__ long long s_best[256], s_h[256], s_nv[256];
    long long best = -1, bh = -1, nv = 0;
    for (long long h = threadIdx.x; h < nh; h += 256) {  // ascending h per thread: a strict > keeps the smallest h on a tie
        const long long s = valid[h] ? (long long) score[h] : -1;
        if (scores64) scores64[h] = s;
        if (valid[h]) {
            ++nv;
            if (s > best) {
                best = s;
                bh = h;
            }
        }
    }
    s_best[threadIdx.x] = best;
    s_h[threadIdx.x] = bh;
    s_nv[threadIdx.x] = nv;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < 256; ++t) {
            nv += s_nv[t];
            if (s_h[t] >= 0 && (s_best[t] > best || (s_best[t] == best && s_h[t] < bh))) {
                best = s_best[t];
                bh = s_h[t];
            }
        }
        out[0] = bh;
        out[1] = best;
        out[2] = nv;
        if (bh >= 0) {
            const PlaneHyp pl = hyp[bh];
            const size_t k = k0[bh];
            win[0] = pl.a;
            win[1] = pl.b;
            win[2] = pl.c;
            win[3] = pl.d;
            win[4] = xs[k];
            win[5] = ys[k];
            win[6] = zs[k];
        }
    }
}

__device__ __forceinline__ double block_max_256(double v, double *sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    return threadIdx.x == 0 ? fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3])) : 0.0;
}

__global__ void __launch_bounds__(256)
k_plane_label(const double *__restrict__ xs, const double *__restrict__ ys, const double *__restrict__ zs, const unsigned int *__restrict__ rem,
              long long m, const double *__restrict__ win, double t, int label, int *__restrict__ labels, unsigned char *__restrict__ flag,
              double *__restrict__ part, unsigned int nb) {
    __shared__ double sm[4];
    const long long k = (long long) blockIdx.x * 256 + threadIdx.x;
    const double a = win[0], b = win[1], c = win[2], d = win[3], ox = win[4], oy = win[5], oz = win[6];
    double v[kPlRows];
#pragma unroll
    for (int e = 0; e < kPlRows; ++e) v[e] = 0.0;
    if (k < m) {
        const double x = xs[k], y = ys[k], z = zs[k];
        const double s = ((a * x + b * y) + c * z) + d;
        if (fabs(s) < t) {
            const size_t i = rem[k];
            labels[i] = label;
            flag[i] = 0;
            const double dx = x - ox, dy = y - oy, dz = z - oz;
            v[0] = dx;
            v[1] = dy;
            v[2] = dz;
            v[3] = dx * dx;
            v[4] = dx * dy;
            v[5] = dx * dz;
            v[6] = dy * dy;
            v[7] = dy * dz;
            v[8] = dz * dz;
            v[9] = (dx * dx + dy * dy) + dz * dz;
        }
    }
#pragma unroll
    for (int e = 0; e < kPlRows; ++e) {
        const double r = e < 9 ? block_sum_256(v[e], sm) : block_max_256(v[e], sm);
        if (threadIdx.x == 0) part[(size_t) e * nb + blockIdx.x] = r;
    }
}

// residuals of the round's inliers against the returned plane: rows sum s^2, sum |s|, max |s|
__global__ void __launch_bounds__(256)
k_plane_resid(const double *__restrict__ xs, const double *__restrict__ ys, const double *__restrict__ zs, const unsigned int *__restrict__ rem,
              long long m, const double *__restrict__ plane, int label, const int *__restrict__ labels, double *__restrict__ part,
              unsigned int nb) {
    __shared__ double sm[4];
    const long long k = (long long) blockIdx.x * 256 + threadIdx.x;
    double s2 = 0.0, sa = 0.0;
    if (k < m && labels[rem[k]] == label) {
        const double s = ((plane[0] * xs[k] + plane[1] * ys[k]) + plane[2] * zs[k]) + plane[3];
        sa = fabs(s);
        s2 = s * s;
    }
    const double r0 = block_sum_256(s2, sm), r1 = block_sum_256(sa, sm), r2 = block_max_256(sa, sm);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = r0;
        part[(size_t) nb + blockIdx.x] = r1;
        part[2 * (size_t) nb + blockIdx.x] = r2;
    }
}

// row v of `in` ([rows][nb]) -> out[v * gridDim.x + block]: block b takes the chunk [b chunk, (b + 1) chunk) of the row, thread t the
// entries t, t + 256, ... in order.  Rows >= first_max are maxima (of values >= 0), the others sums.
__global__ void __launch_bounds__(256)
k_plane_reduce(const double *__restrict__ in, long long nb, long long chunk, int rows, int first_max, double *__restrict__ out) {
    __shared__ double sm[4];
    const long long b0 = (long long) blockIdx.x * chunk, b1 = b0 + chunk < nb ? b0 + chunk : nb;
    for (int v = 0; v < rows; ++v) {
        const double *row = in + (size_t) v * nb;
        double s = 0.0, r;
        if (v < first_max) {
            for (long long b = b0 + threadIdx.x; b < b1; b += 256) s += row[b];
            r = block_sum_256(s, sm);
        } else {
            for (long long b = b0 + threadIdx.x; b < b1; b += 256) s = fmax(s, row[b]);
            r = block_max_256(s, sm);
        }
        if (threadIdx.x == 0) out[(size_t) v * gridDim.x + blockIdx.x] = r;
    }
}

// one thread.  tot = the kPlRows totals, win = the winner's plane and p0, k = its inlier count.  rec[0..3] = the returned plane,
// rec[4] = 1.0 when the refit was degenerate
__global__ void k_plane_refit(const double *__restrict__ tot, const double *__restrict__ win, long long k, int refit, double *__restrict__ rec) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double pl[4] = {win[0], win[1], win[2], win[3]};
    double deg = 0.0;
    if (refit) {
        const double kd = (double) k;
        const double m1[3] = {tot[0], tot[1], tot[2]};
        double a[9], ev[3], V[9];
        a[0] = (tot[3] - m1[0] * m1[0] / kd) / kd;
        a[4] = (tot[6] - m1[1] * m1[1] / kd) / kd;
        a[8] = (tot[8] - m1[2] * m1[2] / kd) / kd;
        a[1] = a[3] = (tot[4] - m1[0] * m1[1] / kd) / kd;
        a[2] = a[6] = (tot[5] - m1[0] * m1[2] / kd) / kd;
        a[5] = a[7] = (tot[7] - m1[1] * m1[2] / kd) / kd;
        jacobi_sym(3, a, ev, V);
        int i3 = 0;
        if (ev[1] < ev[i3]) i3 = 1;
        if (ev[2] < ev[i3]) i3 = 2;
        const double l3 = ev[i3], l2 = fmin(ev[(i3 + 1) % 3], ev[(i3 + 2) % 3]);
        if (l2 - l3 <= ((8.0 * kd) * 0x1p-53) * tot[9]) {
            deg = 1.0;  // the two smallest eigenvalues are equal to working precision: no normal, the hypothesis plane stays
        } else {
            double nrm[3] = {V[i3], V[3 + i3], V[6 + i3]};
            plane_sign(nrm);
            const double cen[3] = {win[4] + m1[0] / kd, win[5] + m1[1] / kd, win[6] + m1[2] / kd};
            pl[0] = nrm[0];
            pl[1] = nrm[1];
            pl[2] = nrm[2];
            pl[3] = -dot3(nrm, cen);
        }
    }
    rec[0] = pl[0];
    rec[1] = pl[1];
    rec[2] = pl[2];
    rec[3] = pl[3];
    rec[4] = deg;
}

__global__ void __launch_bounds__(256)
k_plane_keep_mask(const int *__restrict__ labels, long long n, int plane, int invert, unsigned char *__restrict__ keep,
                  unsigned long long *__restrict__ kept) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    bool k = false;
    if (i < n) {
        const int l = labels[i];
        k = (plane >= 0 ? l == plane : l >= 0) != (invert != 0);
        keep[i] = k ? 1 : 0;
    }
    const int c = __syncthreads_count(k);
    if (threadIdx.x == 0 && c) atomicAdd(kept, (unsigned long long) c);
}

// [rows][nb] partials in `part` -> totals in tot[rows]; the stage buffer lies between them
void reduce_rows(me_ctx *ctx, const double *part, unsigned int nb, int rows, int first_max, double *stage, double *tot) {
    const long long chunk = ((long long) nb + kPlStage - 1) / kPlStage;
    hipLaunchKernelGGL(k_plane_reduce, dim3(kPlStage), dim3(256), 0, ctx->stream, part, (long long) nb, chunk, rows, first_max, stage);
    hipLaunchKernelGGL(k_plane_reduce, dim3(1), dim3(256), 0, ctx->stream, (const double *) stage, (long long) kPlStage, (long long) kPlStage,
                       rows, first_max, tot);
}

}  // namespace

int segment_planes(me_ctx *ctx, int slot, const me_plane_params *p, me_plane_record *planes_host, int32_t *labels_host, int64_t *scores_host,
                   me_plane_info *info) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_segment_planes"));
    if (!p) return ctx->fail(ME_ERR_ARG, "me_segment_planes: no parameters");
    if (!(p->distance_threshold > 0) || !std::isfinite(p->distance_threshold))
        return ctx->fail(ME_ERR_ARG, "me_segment_planes: distance_threshold must be finite and > 0");
    if (p->num_iterations < 1 || p->num_iterations > kPlMaxHyp)
        return ctx->fail(ME_ERR_ARG, "me_segment_planes: num_iterations must be in [1, 2^24]");
    if (p->max_planes < 1 || p->max_planes > 64) return ctx->fail(ME_ERR_ARG, "me_segment_planes: max_planes must be in [1, 64]");
    if (p->min_inliers < 3) return ctx->fail(ME_ERR_ARG, "me_segment_planes: min_inliers must be >= 3");
    if (p->refit != 0 && p->refit != 1) return ctx->fail(ME_ERR_ARG, "me_segment_planes: refit must be 0 or 1");
    Cloud &c = ctx->cloud[slot];
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = c.n, H = p->num_iterations;
    const int P = p->max_planes;
    const double t = p->distance_threshold;
    const long long n_pad = (n + kPlTile - 1) / kPlTile * kPlTile;
    const unsigned int nb_max = blocks_of(n);
    DevBuf &flag = ctx->plane_tmp[0], &rem = ctx->plane_tmp[1], &soa = ctx->plane_tmp[2], &hyp = ctx->plane_tmp[3], &hyp_aux = ctx->plane_tmp[4],
           &scores64 = ctx->plane_tmp[5], &small = ctx->plane_tmp[6];
    ME_CHECK(ctx, flag.ensure((size_t) n));
    ME_CHECK(ctx, rem.ensure((size_t) n * 4));
    ME_CHECK(ctx, soa.ensure((size_t) n_pad * 24));
    ME_CHECK(ctx, hyp.ensure((size_t) H * sizeof(PlaneHyp)));
    ME_CHECK(ctx, hyp_aux.ensure((size_t) H * 9));  // k0 u32 | score u32 | valid u8
    if (scores_host) ME_CHECK(ctx, scores64.ensure((size_t) H * 8));
    // small: [0] remaining count u32, [8 ..] best (3 x i64), [32 ..] win (7 doubles), [96 ..] rec (5 doubles), [136 ..] residual totals (3),
    // [160 ..] moment totals (kPlRows)
    ME_CHECK(ctx, small.ensure(256));
    // partials: [kPlRows][nb] | stage [kPlRows][kPlStage]
    ME_CHECK(ctx, ctx->red.ensure(((size_t) nb_max + kPlStage) * kPlRows * 8));
    ME_CHECK(ctx, c.plane_labels.ensure((size_t) n * 4));
    c.plane_valid = false;
    c.plane_rec.clear();
    char *sb = small.as<char>();
    unsigned int *d_m = reinterpret_cast<unsigned int *>(sb);
    long long *d_best = reinterpret_cast<long long *>(sb + 8);
    double *d_win = reinterpret_cast<double *>(sb + 32), *d_rec = reinterpret_cast<double *>(sb + 96), *d_res = reinterpret_cast<double *>(sb + 136),
           *d_mom = reinterpret_cast<double *>(sb + 160);
    double *xs = soa.as<double>(), *ys = xs + n_pad, *zs = ys + n_pad;
    PlaneHyp *d_hyp = hyp.as<PlaneHyp>();
    unsigned int *d_k0 = hyp_aux.as<unsigned int>(), *d_score = d_k0 + H;
    unsigned char *d_valid = reinterpret_cast<unsigned char *>(d_score + H);
    int *labels = c.plane_labels.as<int>();
    double *part = ctx->red.as<double>();
    if (scores_host) std::fill(scores_host, scores_host + (size_t) P * H, (int64_t) -1);  // (rows of rounds that are never reached)
    {
        TimerScope ts(ctx, "plane");
        hipLaunchKernelGGL(k_plane_init, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, n, labels, flag.as<unsigned char>());
    }
    long long n_valid_total = 0, n_labelled = 0, rounds = 0;
    std::vector<me_plane_record> recs;
    for (int r = 0; r < P; ++r) {
        ++rounds;
        ME_TRY(select_flagged_u32(ctx, flag.as<unsigned char>(), n, rem.as<unsigned int>(), d_m));
        const long long m = n - n_labelled;  // (what the compaction counts: every labelled point left the flags)
        if (m < 3) break;
        const long long m_pad = (m + kPlTile - 1) / kPlTile * kPlTile;
        const long long tiles = m_pad / kPlTile;
        const int tiles_per_block = (int) ((tiles + kPlMaxBlocksX - 1) / kPlMaxBlocksX);
        const unsigned int gx = (unsigned int) ((tiles + tiles_per_block - 1) / tiles_per_block), gy = (unsigned int) ((H + kPlHyp - 1) / kPlHyp);
        {
            TimerScope ts(ctx, "plane");
            hipLaunchKernelGGL(k_plane_compact, dim3(blocks_of(m_pad)), dim3(256), 0, ctx->stream, c.xyz.as<double>(), rem.as<unsigned int>(), m,
                               m_pad, xs, ys, zs);
            hipLaunchKernelGGL(k_plane_hyp, dim3(blocks_of(H)), dim3(256), 0, ctx->stream, H, (u64) p->seed, (u64) r, (u64) m, xs, ys, zs, d_hyp,
                               d_k0, d_valid, d_score);
        }
        {
            TimerScope ts(ctx, "plane_score");
            hipLaunchKernelGGL(k_plane_score, dim3(gx, gy), dim3(256), 0, ctx->stream, xs, ys, zs, m_pad, tiles_per_block, d_hyp, (int) H, t,
                               d_score);
        }
        {
            TimerScope ts(ctx, "plane");
            hipLaunchKernelGGL(k_plane_best, dim3(1), dim3(256), 0, ctx->stream, d_score, d_valid, H, d_hyp, d_k0, xs, ys, zs,
                               scores_host ? scores64.as<long long>() : (long long *) nullptr, d_best, d_win);
        }
        ME_CHECK(ctx, hipGetLastError());
        long long h_best[3] = {-1, -1, 0};
        {
            MailGuard mg(ctx);
            ME_TRY(mail_post(ctx, h_best, d_best, sizeof(h_best)));
            ME_TRY(mg.sync());
        }
        if (scores_host) ME_TRY(copy_d2h(ctx, scores_host + (size_t) r * H, scores64.p, (size_t) H * 8));
        n_valid_total += h_best[2];
        if (h_best[0] < 0 || h_best[1] < p->min_inliers) break;
        const long long cnt = h_best[1];
        const unsigned int nb = blocks_of(m);
        double *stage = part + (size_t) nb * kPlRows;
        {
            TimerScope ts(ctx, "plane");
            hipLaunchKernelGGL(k_plane_label, dim3(nb), dim3(256), 0, ctx->stream, xs, ys, zs, rem.as<unsigned int>(), m, d_win, t, r, labels,
                               flag.as<unsigned char>(), part, nb);
            reduce_rows(ctx, part, nb, kPlRows, 9, stage, d_mom);
            hipLaunchKernelGGL(k_plane_refit, dim3(1), dim3(64), 0, ctx->stream, d_mom, d_win, cnt, p->refit, d_rec);
            hipLaunchKernelGGL(k_plane_resid, dim3(nb), dim3(256), 0, ctx->stream, xs, ys, zs, rem.as<unsigned int>(), m, d_rec, r, labels, part, nb);
            reduce_rows(ctx, part, nb, 3, 2, stage, d_res);
        }
        ME_CHECK(ctx, hipGetLastError());
        double h_rec[5], h_res[3];
        {
            MailGuard mg(ctx);
            ME_TRY(mail_post(ctx, h_rec, d_rec, sizeof(h_rec)));
            ME_TRY(mail_post(ctx, h_res, d_res, sizeof(h_res)));
            ME_TRY(mg.sync());
        }
        me_plane_record rec{};
        rec.count = cnt;
        rec.h = h_best[0];
        rec.score = h_best[1];
        for (int e = 0; e < 4; ++e) rec.plane[e] = h_rec[e];
        rec.rms = std::sqrt(h_res[0] / (double) cnt);
        rec.mean_abs = h_res[1] / (double) cnt;
        rec.max_abs = h_res[2];
        rec.refit_degenerate = h_rec[4] != 0.0 ? 1 : 0;
        recs.push_back(rec);
        n_labelled += cnt;
    }
    if (labels_host) ME_TRY(copy_d2h(ctx, labels_host, c.plane_labels.p, (size_t) n * 4));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (planes_host) std::copy(recs.begin(), recs.end(), planes_host);
    c.plane_rec = recs;
    c.plane_valid = true;
    ++c.plane_serial;
    if (info) {
        info->n_in = n;
        info->n_planes = (int64_t) recs.size();
        info->n_labelled = n_labelled;
        info->n_valid_hypotheses = n_valid_total;
        info->rounds = rounds;
    }
    return ME_OK;
}

int plane_fetch(me_ctx *ctx, int slot, me_plane_record *planes_host, long long capacity, long long *n_planes, int32_t *labels_host) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_plane_fetch"));
    Cloud &c = ctx->cloud[slot];
    if (!c.plane_valid) return ctx->fail(ME_ERR_STATE, "me_plane_fetch: the slot has no plane labels (me_segment_planes)");
    const long long np = (long long) c.plane_rec.size();
    if (n_planes) *n_planes = np;
    if (planes_host) {
        if (capacity < np) return ctx->fail(ME_ERR_CAPACITY, "me_plane_fetch: capacity below the number of planes");
        std::copy(c.plane_rec.begin(), c.plane_rec.end(), planes_host);
    }
    if (labels_host) {
        ME_CHECK(ctx, hipSetDevice(ctx->device));
        ME_TRY(copy_d2h(ctx, labels_host, c.plane_labels.p, (size_t) c.n * 4));
        ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ME_OK;
}

int plane_keep(me_ctx *ctx, int slot, int plane, int invert, uint8_t *keep_host, me_outlier_info *info) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_plane_keep"));
    Cloud &c = ctx->cloud[slot];
    if (!c.plane_valid) return ctx->fail(ME_ERR_STATE, "me_plane_keep: the slot has no plane labels (me_segment_planes)");
    if (plane < -1 || plane >= (long long) c.plane_rec.size())
        return ctx->fail(ME_ERR_ARG, "me_plane_keep: plane must be -1 or the index of an extracted plane");
    if (invert != 0 && invert != 1) return ctx->fail(ME_ERR_ARG, "me_plane_keep: invert must be 0 or 1");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = c.n;
    DevBuf &small = ctx->plane_tmp[6];
    ME_CHECK(ctx, small.ensure(256));
    ME_CHECK(ctx, c.outlier_keep.ensure((size_t) n));
    c.outlier_keep_valid = false;
    unsigned long long *kept = small.as<unsigned long long>();
    ME_CHECK(ctx, hipMemsetAsync(kept, 0, 8, ctx->stream));
    {
        TimerScope ts(ctx, "plane");
        hipLaunchKernelGGL(k_plane_keep_mask, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, c.plane_labels.as<int>(), n, plane, invert,
                           c.outlier_keep.as<unsigned char>(), kept);
    }
    ME_CHECK(ctx, hipGetLastError());
    unsigned long long h_kept = 0;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h_kept, kept, 8));
        ME_TRY(mg.sync());
    }
    if (keep_host) ME_TRY(copy_d2h(ctx, keep_host, c.outlier_keep.p, (size_t) n));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    c.outlier_keep_valid = true;
    if (info) {
        info->n_in = n;
        info->n_kept = (int64_t) h_kept;
        info->n_fallback = 0;
        info->mean = 0.0;
        info->std_dev = 0.0;
        info->threshold = (double) plane;
    }
    return ME_OK;
}

}  // namespace me
