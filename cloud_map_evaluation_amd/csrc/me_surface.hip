// me_surface.hip — the normal-aware error of a direction's resident 1-NN pairs: the point-to-plane distance, its tangential
// remainder and the normal consistency (the definitions are in include/mapeval_hip.h).  It refines the
// nearest-point distances of getDiffRegResultWithCorrespondence (map_eval.cpp:1069-1145) and computeChamferDistance
// (map_eval.cpp:1398-1431) with the reference cloud's normals.
//   k_sf_stat      a fixed grid of at most kSfBlocks blocks strides over the sorted queries: the pair's use, e, t2 and c (kept on the
//                  slot in SORTED order, -1 where unused), the counts, the sums, the (largest e, smallest original index) pair and the
//                  threshold counts; the block's partial record and the one-block total over the records are me_reduce.hpp's
//                                                                                                          (me_nn_surface_error, "surface")
//   k_sf_unpermute e and c back in cloud order                                                             (me_nn_surface_fetch)
// The file is compiled with -ffp-contract=off: tests/_surface_ref.py restates the three expressions.
#include <cmath>
#include <cstring>

#include "me_internal.hpp"
#include "me_reduce.hpp"
#include "me_stat.hpp"

namespace me {

namespace {

typedef unsigned long long u64;

constexpr int kSfT = ME_ERRDIST_MAX_THRESHOLDS, kSfA = ME_SURFACE_MAX_ANGLES;
constexpr unsigned int kSfBlocks = 1024;  // above 256 x 1024 queries a block strides over the array
constexpr int kSfD = 4 + kSfT;            // double sums per block: sum_e, sum_e2, sum_t2, sum_c, sum_e2_within[8]
constexpr int kSfNI = 3 + kSfT + kSfA;    // integer sums: n_query, n_used, n_normal_used, n_within[8], n_angle[8]; then max key, argmax
typedef RedBufs<kSfD, kSfNI> SfRed;

struct SfThr {
    double tau[kSfT], cos_min[kSfA];
    int nt, na;
};

// ref_xyz / ref_nrm / q_nrm are in CLOUD order (q_nrm may be nullptr); d2s / idxs / e_s / c_s in the query's SORTED order.  Every
// gather is guarded by 0 <= j < n_ref; the query's original index is a permutation of [0, n).
__global__ void __launch_bounds__(256)
k_sf_stat(const SPoint *__restrict__ qsp, const double *__restrict__ d2s, const int *__restrict__ idxs, long long n,
          const double *__restrict__ ref_xyz, const double *__restrict__ ref_nrm, long long n_ref, const double *__restrict__ q_nrm,
          StatParams gp, SfThr thr, double *__restrict__ e_s, double *__restrict__ c_s, double *__restrict__ pd, long long *__restrict__ pi) {
    long long arg = -1, ci[kSfNI];  // n_query, n_used, n_normal_used, n_within[8], n_angle[8]
    u64 mx = 0ull;
    double sd[kSfD];                // sum_e, sum_e2, sum_t2, sum_c, sum_e2_within[8]
    long long *const nw = ci + 3, *const na = ci + 3 + kSfT;
    double *const sw = sd + 4;
#pragma unroll
    for (int k = 0; k < kSfNI; ++k) ci[k] = 0;
#pragma unroll
    for (int k = 0; k < kSfD; ++k) sd[k] = 0.0;
    const long long S = (long long) gridDim.x * 256;
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += S) {
        const double d2 = d2s[i];
        const long long j = idxs[i];
        double e = -1.0, c = -1.0;
        if (d2 >= 0.0) ci[0] += 1;
        if (d2 >= 0.0 && gate_pass(gp, d2) && j >= 0 && j < n_ref) {
            const double nx = ref_nrm[3 * j], ny = ref_nrm[3 * j + 1], nz = ref_nrm[3 * j + 2];
            if (!(nx == 0.0 && ny == 0.0 && nz == 0.0)) {
                const SPoint p = qsp[i];
                const double dx = p.x - ref_xyz[3 * j], dy = p.y - ref_xyz[3 * j + 1], dz = p.z - ref_xyz[3 * j + 2];
                e = fabs((nx * dx + ny * dy) + nz * dz);
                const double e2 = e * e;
                ci[1] += 1;
                sd[0] += e;
                sd[1] += e2;
                sd[2] += fmax(d2 - e2, 0.0);
                const u64 key = (u64) __double_as_longlong(e);  // (e >= +0.0: the order of the bit patterns is the numeric order)
                take_max(mx, arg, key, p.idx);
#pragma unroll
                for (int k = 0; k < kSfT; ++k)
                    if (k < thr.nt && e <= thr.tau[k]) nw[k] += 1, sw[k] += e2;
                if (q_nrm) {
                    const double m0 = q_nrm[3 * p.idx], m1 = q_nrm[3 * p.idx + 1], m2 = q_nrm[3 * p.idx + 2];
                    if (!(m0 == 0.0 && m1 == 0.0 && m2 == 0.0)) {
                        c = fabs((m0 * nx + m1 * ny) + m2 * nz);
                        ci[2] += 1;
                        sd[3] += c;
#pragma unroll
                        for (int k = 0; k < kSfA; ++k)
                            if (k < thr.na && c >= thr.cos_min[k]) na[k] += 1;
                    }
                }
            }
        }
        e_s[i] = e;
        c_s[i] = c;
    }
    red_store_partial<kSfD, kSfNI, false>(sd, ci, mx, arg, 0ull, pd + (size_t) blockIdx.x * kSfD, pi + (size_t) blockIdx.x * SfRed::Totals::NR);
}

__global__ void __launch_bounds__(256)
k_sf_unpermute(const SPoint *__restrict__ sp, long long n, const double *__restrict__ e_s, const double *__restrict__ c_s,
               double *__restrict__ e_o, double *__restrict__ c_o) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long o = sp[i].idx;
    if (e_o) e_o[o] = e_s[i];
    if (c_o) c_o[o] = c_s[i];
}

}  // namespace

int nn_surface_error(me_ctx *ctx, int qslot, const me_surface_params *p, me_surface_out *out) {
    ME_TRY(need_single_gpu_cloud(ctx, qslot, "me_nn_surface_error"));
    if (!p || !out) return ctx->fail(ME_ERR_ARG, "me_nn_surface_error: NULL argument");
    if (p->gate != p->gate || (p->gate_mode != ME_GATE_LE_UNSQUARED && p->gate_mode != ME_GATE_LT_SQUARED))
        return ctx->fail(ME_ERR_ARG, "me_nn_surface_error: bad gate or gate_mode");
    if (p->n_thresholds < 0 || p->n_thresholds > kSfT) return ctx->fail(ME_ERR_ARG, "me_nn_surface_error: n_thresholds must be in [0, 8]");
    for (int k = 0; k < p->n_thresholds; ++k)
        if (!(p->tau[k] >= 0.0) || p->tau[k] == INFINITY) return ctx->fail(ME_ERR_ARG, "me_nn_surface_error: every tau must be finite and >= 0");
    if (p->n_angles < 0 || p->n_angles > kSfA) return ctx->fail(ME_ERR_ARG, "me_nn_surface_error: n_angles must be in [0, 8]");
    for (int k = 0; k < p->n_angles; ++k)
        if (!(p->cos_min[k] >= 0.0 && p->cos_min[k] <= 1.0)) return ctx->fail(ME_ERR_ARG, "me_nn_surface_error: every cos_min must be in [0, 1]");
    Cloud &q = ctx->cloud[qslot];
    if (q.nn_ref_slot < 0) return ctx->fail(ME_ERR_STATE, "no NN result for this slot (call me_nn1 first)");
    Cloud &r = ctx->cloud[q.nn_ref_slot];
    if (!r.have_normals)
        return ctx->fail(ME_ERR_STATE, "me_nn_surface_error: the reference cloud has no normals (me_set_normals / me_estimate_normals / me_radius_normals)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = q.n;
    q.surf_have = false;
    ME_CHECK(ctx, q.surf_e.ensure((size_t) n * 8));
    ME_CHECK(ctx, q.surf_c.ensure((size_t) n * 8));
    const int nb = (int) std::min<long long>(kSfBlocks, blocks_of(n));
    ME_CHECK(ctx, ctx->red.ensure(SfRed::bytes(kSfBlocks)));
    const SfRed red(ctx, kSfBlocks);
    SfThr thr{};
    thr.nt = p->n_thresholds;
    thr.na = p->n_angles;
    for (int k = 0; k < thr.nt; ++k) thr.tau[k] = p->tau[k];
    for (int k = 0; k < thr.na; ++k) thr.cos_min[k] = p->cos_min[k];
    {
        TimerScope ts(ctx, "surface");
        hipLaunchKernelGGL(k_sf_stat, dim3(nb), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), q.nn_d2.as<double>(), q.nn_idx.as<int>(), n,
                           r.xyz.as<double>(), r.normals.as<double>(), r.n, q.have_normals ? q.normals.as<double>() : nullptr,
                           make_params(p->gate, p->gate_mode, nullptr), thr, q.surf_e.as<double>(), q.surf_c.as<double>(), red.pd, red.pi);
        red.total(ctx, nb, red.tot);
    }
    ME_CHECK(ctx, hipGetLastError());
    SfRed::Totals h;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h, red.tot, sizeof(h)));
        ME_TRY(mg.sync());
    }
    q.surf_have = true;
    std::memset(out, 0, sizeof(*out));
    out->n_query = h.i[0];
    out->n_used = h.i[1];
    out->n_normal_used = h.i[2];
    out->argmax = -1;
    if (h.i[1] > 0) {
        out->sum_e = h.d[0];
        out->sum_e2 = h.d[1];
        out->sum_t2 = h.d[2];
        out->sum_c = h.d[3];
        std::memcpy(&out->max_e, &h.i[kSfNI], 8);
        out->argmax = h.i[kSfNI + 1];
        for (int k = 0; k < p->n_thresholds; ++k) out->n_within[k] = h.i[3 + k], out->sum_e2_within[k] = h.d[4 + k];
        for (int k = 0; k < p->n_angles; ++k) out->n_angle[k] = h.i[3 + kSfT + k];
    }
    return ME_OK;
}

int nn_surface_fetch(me_ctx *ctx, int qslot, double *plane_d, double *cos_n) {
    ME_TRY(need_single_gpu_cloud(ctx, qslot, "me_nn_surface_fetch"));
    Cloud &q = ctx->cloud[qslot];
    if (q.nn_ref_slot < 0 || !q.surf_have)
        return ctx->fail(ME_ERR_STATE, "me_nn_surface_fetch: no result for this slot (run me_nn_surface_error; it is discarded with the 1-NN result)");
    if (!plane_d && !cos_n) return ME_OK;
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = q.n;
    DevBuf &eo = ctx->tmp[2], &co = ctx->tmp[3];
    if (plane_d) ME_CHECK(ctx, eo.ensure((size_t) n * 8));
    if (cos_n) ME_CHECK(ctx, co.ensure((size_t) n * 8));
    hipLaunchKernelGGL(k_sf_unpermute, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, q.surf_e.as<double>(),
                       q.surf_c.as<double>(), plane_d ? eo.as<double>() : nullptr, cos_n ? co.as<double>() : nullptr);
    ME_CHECK(ctx, hipGetLastError());
    if (plane_d) ME_TRY(copy_d2h(ctx, plane_d, eo.p, (size_t) n * 8));
    if (cos_n) ME_TRY(copy_d2h(ctx, cos_n, co.p, (size_t) n * 8));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

}  // namespace me
