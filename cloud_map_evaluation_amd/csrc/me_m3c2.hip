// me_m3c2.hip — M3C2 (Lague, Brodu, Leroux 2013): the signed distance between two resident clouds along the query cloud's normals,
// averaged inside a cylinder, with a per-point level of detection.  The definition is in include/mapeval_hip.h, DESIGN.md section 4.15.
//   k_m3_stream<OTHER>  one body, launched once per streamed cloud.  Every lane holds a core point q (a sorted point of the query
//                  cloud) and its stored normal N, gathered through sp[i].idx, and streams a cloud's 27-cell neighbourhood through the
//                  wave's LDS tile (me_wave_stream.hpp): a candidate p is inside iff fabs(t) < L && d2 - t*t < rp*rp with
//                  t = N.(p - q), d2 = |p - q|^2 (both strict); n, S = sum t and Q = sum t*t per lane in stream order — moments about
//                  the core point, so that no term exceeds L^2.  <false> streams the query's own cloud (the cell of stream_query),
//                  <true> the other cloud: the cell of q in THAT cloud's Morton frame (fine_coord, as k_nn_grid places a query),
//                  clamped per axis into [0, cell_lim).  The cell edge of both indexes is >= R = sqrt(L*L + rp*rp), the radius of the
//                  cylinder's bounding ball: a point inside the cylinder lies within R of q on every axis, i.e. in a cell at most one
//                  away from q's.  A core point whose cell is -1 or cell_lim on an axis (less than one cell outside the frame) can only
//                  reach the frame's border cell on that axis, which the clamped cell's 3x3x3 block holds; one further out on any axis
//                  has no cell of the frame within reach and is settled with n = 0 without streaming.  Masked-out lanes are not pending.
//   k_m3_final     a fixed grid of at most kM3Blocks blocks strides over the sorted core points: validity, dist, the two variances,
//                  lod and the significance bit, kept on the slot in SORTED order; counts, sums and the (largest |dist|, smallest
//                  original index) pair per block; the block's partial record and the one-block total over the records are
//                  me_reduce.hpp's                                                                                   (me_m3c2, "m3c2")
//   k_m3_unpermute the per-point results back in cloud order                                                         (me_m3c2_fetch)
// The search visits the ball of radius R, not the cylinder: the work per core point grows like (R / spacing)^2 on a surface.  The
// remedy for long cylinders on dense clouds is the core mask (M3C2's core points); a stepped walk along the axis is not built.
// The file is compiled with -ffp-contract=off: tests/_m3c2_ref.py restates the membership test.
#include <cmath>
#include <cstring>

#include "me_internal.hpp"
#include "me_reduce.hpp"
#include "me_wave_stream.hpp"

namespace me {

namespace {

typedef unsigned long long u64;

constexpr unsigned int kM3Blocks = 1024;  // above 256 x 1024 core points a block of k_m3_final strides over the array
constexpr int kM3D = 4;                   // double sums per block: sum_dist, sum_abs_dist, sum_dist2, sum_lod
constexpr int kM3NI = 6;                  // integer sums: n_core, n_no_normal, n_valid, n_significant, sum_n_own, sum_n_other; then max key, argmax
typedef RedBufs<kM3D, kM3NI> M3Red;

// qsp / qcodes / nq / qshift: the query cloud's sorted points; ssp / g / fr: the streamed cloud (the query's own when !OTHER).
// nrm (double[nq][3]) and mask (uint8[nq] or nullptr) are in the query's CLOUD order; cnt_s / S_s / Q_s in its SORTED order.
template <bool OTHER>
__global__ void __launch_bounds__(256)
k_m3_stream(const SPoint *__restrict__ qsp, const unsigned long long *__restrict__ qcodes, long long nq, int qshift,
            const SPoint *__restrict__ ssp, GridView g, FrameView fr, const double *__restrict__ nrm, const unsigned char *__restrict__ mask,
            double L, double rp2, int *__restrict__ cnt_s, double *__restrict__ S_s, double *__restrict__ Q_s) {
    __shared__ WaveTile s_tile[4];
    __shared__ int2 s_tab[4][kGroupTab + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const StreamQuery q = stream_query(qsp, qcodes, i, nq, qshift);
    double nx = 0, ny = 0, nz = 0;
    bool pending = q.active;
    int cx = q.cx, cy = q.cy, cz = q.cz;
    if (q.active) {  // q.idx is a permutation of [0, nq)
        if (mask && !mask[q.idx]) pending = false;
        nx = nrm[3 * q.idx];
        ny = nrm[3 * q.idx + 1];
        nz = nrm[3 * q.idx + 2];
    }
    if (OTHER) {
        cx = cy = cz = 0;
        if (pending) {
            const int cell_lim = 1 << (kMortonBits - g.shift);
            const double sc = ldexp(1.0, -g.shift), lim = (double) cell_lim;
            // the cell as a double first: a far core point's coordinate does not fit an int
            const double ux = floor(fine_coord(q.qx, fr.ox, fr.fine_h) * sc), uy = floor(fine_coord(q.qy, fr.oy, fr.fine_h) * sc),
                         uz = floor(fine_coord(q.qz, fr.oz, fr.fine_h) * sc);
            if (ux < -1.0 || uy < -1.0 || uz < -1.0 || ux > lim || uy > lim || uz > lim) {
                pending = false;  // more than one cell outside the frame: nothing within R
            } else {
                cx = min(max((int) ux, 0), cell_lim - 1);
                cy = min(max((int) uy, 0), cell_lim - 1);
                cz = min(max((int) uz, 0), cell_lim - 1);
            }
        }
    }
    int cnt = 0;
    double S = 0.0, Q = 0.0;
    wave_stream(pending, cx, cy, cz, ssp, g, lane, s_tab[w], &s_tile[w], [&](double px, double py, double pz, int, int) {
        const double dx = px - q.qx, dy = py - q.qy, dz = pz - q.qz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const double t = (nx * dx + ny * dy) + nz * dz;
        if (fabs(t) < L && d2 - t * t < rp2) {
            ++cnt;
            S += t;
            Q += t * t;
        }
    });
    if (q.active) {
        cnt_s[i] = cnt;
        S_s[i] = S;
        Q_s[i] = Q;
    }
}

// cnt: int[2][n] (own, other), mom: double[4][n] (S_own, Q_own, S_other, Q_other), res: double[4][n] (dist, lod, var_own, var_other),
// all in the query's SORTED order; nrm / mask in cloud order.
__global__ void __launch_bounds__(256)
k_m3_final(const SPoint *__restrict__ sp, long long n, const double *__restrict__ nrm, const unsigned char *__restrict__ mask,
           int *__restrict__ cnt, const double *__restrict__ mom, int min_points, double reg, double *__restrict__ res,
           unsigned char *__restrict__ flags, double *__restrict__ pd, long long *__restrict__ pi) {
    long long arg = -1, ci[kM3NI] = {0, 0, 0, 0, 0, 0};  // n_core, n_no_normal, n_valid, n_significant, sum_n_own, sum_n_other
    u64 mx = 0ull;
    double sd[kM3D] = {0.0, 0.0, 0.0, 0.0};              // sum_dist, sum_abs_dist, sum_dist2, sum_lod
    const long long stride = (long long) gridDim.x * 256;
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const long long o = sp[i].idx;
        const bool in = !mask || mask[o];
        int n_own = cnt[i], n_oth = cnt[n + i];
        double dist = 0.0, lod = 0.0, vo = 0.0, vt = 0.0;
        unsigned char fl = 0;
        if (in) {
            ci[0] += 1;
            const bool zero = nrm[3 * o] == 0.0 && nrm[3 * o + 1] == 0.0 && nrm[3 * o + 2] == 0.0;
            if (zero) ci[1] += 1;
            if (!zero && n_own >= min_points && n_oth >= min_points) {
                const double no = (double) n_own, nt = (double) n_oth;
                const double S0 = mom[i], Q0 = mom[n + i], S1 = mom[2 * n + i], Q1 = mom[3 * n + i];
                dist = S1 / nt - S0 / no;
                vo = fmax((Q0 - S0 * S0 / no) / (no - 1.0), 0.0);
                vt = fmax((Q1 - S1 * S1 / nt) / (nt - 1.0), 0.0);
                lod = 1.96 * (sqrt(vo / no + vt / nt) + reg);
                const double ad = fabs(dist);
                fl = 1;
                if (ad > lod) fl |= 2, ci[3] += 1;
                ci[2] += 1;
                sd[0] += dist;
                sd[1] += ad;
                sd[2] += dist * dist;
                sd[3] += lod;
                ci[4] += n_own;
                ci[5] += n_oth;
                take_max(mx, arg, (u64) __double_as_longlong(ad), o);  // (ad >= +0.0: the order of the bit patterns is the numeric order)
            }
        } else {
            n_own = n_oth = 0;
        }
        cnt[i] = n_own;
        cnt[n + i] = n_oth;
        res[i] = dist;
        res[n + i] = lod;
        res[2 * n + i] = vo;
        res[3 * n + i] = vt;
        flags[i] = fl;
    }
    red_store_partial<kM3D, kM3NI, false>(sd, ci, mx, arg, 0ull, pd + (size_t) blockIdx.x * kM3D, pi + (size_t) blockIdx.x * M3Red::Totals::NR);
}

// every output is nullable; cnt_s / res_s / fl_s as k_m3_final leaves them
__global__ void __launch_bounds__(256)
k_m3_unpermute(const SPoint *__restrict__ sp, long long n, const int *__restrict__ cnt_s, const double *__restrict__ res_s,
               const unsigned char *__restrict__ fl_s, double *__restrict__ dist, double *__restrict__ lod, double *__restrict__ var_own,
               double *__restrict__ var_other, int *__restrict__ n_own, int *__restrict__ n_other, unsigned char *__restrict__ fl) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long o = sp[i].idx;
    if (dist) dist[o] = res_s[i];
    if (lod) lod[o] = res_s[n + i];
    if (var_own) var_own[o] = res_s[2 * n + i];
    if (var_other) var_other[o] = res_s[3 * n + i];
    if (n_own) n_own[o] = cnt_s[i];
    if (n_other) n_other[o] = cnt_s[n + i];
    if (fl) fl[o] = fl_s[i];
}

}  // namespace

int m3c2(me_ctx *ctx, int qslot, const me_m3c2_params *p, const uint8_t *core_mask, me_m3c2_out *out) {
    if (qslot < 0 || qslot > 1) return ctx->fail(ME_ERR_ARG, "me_m3c2: bad slot");
    if (!p || !out) return ctx->fail(ME_ERR_ARG, "me_m3c2: NULL argument");
    const double rp = p->projection_radius, L = p->max_depth;
    if (!(rp > 0) || !std::isfinite(rp)) return ctx->fail(ME_ERR_ARG, "me_m3c2: projection_radius must be finite and > 0");
    if (!(L > 0) || !std::isfinite(L)) return ctx->fail(ME_ERR_ARG, "me_m3c2: max_depth must be finite and > 0");
    if (p->min_points < 2) return ctx->fail(ME_ERR_ARG, "me_m3c2: min_points must be >= 2 (the variance divides by n - 1)");
    if (!(p->reg_error >= 0) || !std::isfinite(p->reg_error)) return ctx->fail(ME_ERR_ARG, "me_m3c2: reg_error must be finite and >= 0");
    const double R = std::sqrt(L * L + rp * rp);
    if (!std::isfinite(R)) return ctx->fail(ME_ERR_ARG, "me_m3c2: sqrt(max_depth^2 + projection_radius^2) is not finite");
    ME_TRY(need_single_gpu_cloud(ctx, qslot, "me_m3c2"));
    ME_TRY(need_single_gpu_cloud(ctx, 1 - qslot, "me_m3c2"));
    Cloud &q = ctx->cloud[qslot], &r = ctx->cloud[1 - qslot];
    if (!q.have_normals)
        return ctx->fail(ME_ERR_STATE, "me_m3c2: the query cloud has no normals (me_set_normals / me_estimate_normals / me_radius_normals)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    // both indexes at the level of the cylinder's bounding ball (run_local_geom's test): the 27-cell stencil is exact when the cell
    // edge is >= R.  A rebuild re-sorts the slot and drops the 1-NN results of both slots and the slot's local-geometry result.
    // A refused R (more than 2^21 cells per axis) leaves that slot's index and everything resident on it as they were: the cell size
    // asked for at the upload is put back before the error returns, and the query's earlier result is discarded only below.
    const double want_h = R * (1.0 + 0x1p-20);
    for (int s = 0; s < 2; ++s) {
        Cloud &c = ctx->cloud[s];
        if (!c.index_valid || c.cell_h < want_h || c.cell_h > 1.5 * want_h) {
            const double req = c.cell_size_req;
            const int rc = cloud_build_index(ctx, s, R);
            c.cell_size_req = req;
            if (rc != ME_OK) return rc;
        }
    }
    q.m3c2_have = false;  // (from here on the slot's result buffers are rewritten)
    const long long n = q.n;
    ME_CHECK(ctx, q.m3_cnt.ensure((size_t) n * 2 * 4));
    ME_CHECK(ctx, q.m3_mom.ensure((size_t) n * 4 * 8));
    ME_CHECK(ctx, q.m3_res.ensure((size_t) n * 4 * 8));
    ME_CHECK(ctx, q.m3_flags.ensure((size_t) n));
    const unsigned char *mask = nullptr;
    if (core_mask) {
        DevBuf &mb = ctx->tmp[5];
        ME_CHECK(ctx, mb.ensure((size_t) n));
        ME_TRY(copy_h2d(ctx, mb.p, core_mask, (size_t) n));
        mask = mb.as<unsigned char>();
    }
    const int nb = (int) std::min<long long>(kM3Blocks, blocks_of(n));
    ME_CHECK(ctx, ctx->red.ensure(M3Red::bytes(kM3Blocks)));
    const M3Red red(ctx, kM3Blocks);
    int *cnt = q.m3_cnt.as<int>();
    double *mom = q.m3_mom.as<double>();
    {
        TimerScope ts(ctx, "m3c2");
        const FrameView fq{q.origin[0], q.origin[1], q.origin[2], q.fine_h}, fr{r.origin[0], r.origin[1], r.origin[2], r.fine_h};
        hipLaunchKernelGGL(k_m3_stream<false>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), q.codes.as<unsigned long long>(), n,
                           q.grid.shift, q.sp.as<SPoint>(), q.grid, fq, q.normals.as<double>(), mask, L, rp * rp, cnt, mom, mom + n);
        hipLaunchKernelGGL(k_m3_stream<true>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), q.codes.as<unsigned long long>(), n,
                           q.grid.shift, r.sp.as<SPoint>(), r.grid, fr, q.normals.as<double>(), mask, L, rp * rp, cnt + n, mom + 2 * n, mom + 3 * n);
        hipLaunchKernelGGL(k_m3_final, dim3(nb), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, q.normals.as<double>(), mask, cnt,
                           (const double *) mom, (int) p->min_points, p->reg_error, q.m3_res.as<double>(), q.m3_flags.as<unsigned char>(), red.pd, red.pi);
        red.total(ctx, nb, red.tot);
    }
    ME_CHECK(ctx, hipGetLastError());
    M3Red::Totals h;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h, red.tot, sizeof(h)));
        ME_TRY(mg.sync());
    }
    q.m3c2_have = true;
    std::memset(out, 0, sizeof(*out));
    out->n_core = h.i[0];
    out->n_no_normal = h.i[1];
    out->n_valid = h.i[2];
    out->n_significant = h.i[3];
    out->argmax = -1;
    if (h.i[2] > 0) {
        out->sum_dist = h.d[0];
        out->sum_abs_dist = h.d[1];
        out->sum_dist2 = h.d[2];
        out->sum_lod = h.d[3];
        out->sum_n_own = h.i[4];
        out->sum_n_other = h.i[5];
        std::memcpy(&out->max_abs_dist, &h.i[kM3NI], 8);
        out->argmax = h.i[kM3NI + 1];
    }
    return ME_OK;
}

int m3c2_fetch(me_ctx *ctx, int qslot, double *dist, double *lod, double *var_own, double *var_other, int32_t *n_own, int32_t *n_other,
               uint8_t *flags) {
    ME_TRY(need_single_gpu_cloud(ctx, qslot, "me_m3c2_fetch"));
    Cloud &q = ctx->cloud[qslot];
    if (!q.m3c2_have || !q.index_valid)
        return ctx->fail(ME_ERR_STATE, "me_m3c2_fetch: no result for this slot (run me_m3c2; a changed cloud or a new index discards it)");
    if (!dist && !lod && !var_own && !var_other && !n_own && !n_other && !flags) return ME_OK;
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = q.n;
    // one scratch block: the double arrays asked for, then the int arrays, then the flags
    double *hd[4] = {dist, lod, var_own, var_other};
    int32_t *hi[2] = {n_own, n_other};
    DevBuf &buf = ctx->tmp[2];
    ME_CHECK(ctx, buf.ensure((size_t) n * (4 * 8 + 2 * 4 + 1)));
    double *dd = buf.as<double>();
    int *di = reinterpret_cast<int *>(dd + 4 * n);
    unsigned char *df = reinterpret_cast<unsigned char *>(di + 2 * n);
    hipLaunchKernelGGL(k_m3_unpermute, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, q.m3_cnt.as<int>(),
                       q.m3_res.as<double>(), q.m3_flags.as<unsigned char>(), hd[0] ? dd : nullptr, hd[1] ? dd + n : nullptr,
                       hd[2] ? dd + 2 * n : nullptr, hd[3] ? dd + 3 * n : nullptr, hi[0] ? di : nullptr, hi[1] ? di + n : nullptr,
                       flags ? df : nullptr);
    ME_CHECK(ctx, hipGetLastError());
    for (int k = 0; k < 4; ++k)
        if (hd[k]) ME_TRY(copy_d2h(ctx, hd[k], dd + (size_t) k * n, (size_t) n * 8));
    for (int k = 0; k < 2; ++k)
        if (hi[k]) ME_TRY(copy_d2h(ctx, hi[k], di + (size_t) k * n, (size_t) n * 4));
    if (flags) ME_TRY(copy_d2h(ctx, flags, df, (size_t) n));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

}  // namespace me
