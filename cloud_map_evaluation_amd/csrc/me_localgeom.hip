// me_localgeom.hip — mean plane variance (MPV) and the eigenvalue shape features of every point's radius neighbourhood, on a resident
// single-GPU cloud.  DESIGN.md section 4.10.
//   k_local_geom   per point: the neighbours j with d2 < r^2 (strict, the library's radius convention, the query itself removed once)
//                  streamed through the wave's LDS tile (me_wave_stream.hpp) over the radius grid (cell >= r); k, sum(d) and
//                  sum(d d^T) with d = p_j - q in fp64 — moments about the QUERY, so that no term exceeds r^2 and the smallest
//                  eigenvalue keeps its digits on every point (k_mme3 takes them about the round leader's point: me_mme.hip) —
//                  then C = (sum(d d^T) - sum(d) sum(d)^T / k) / (k - 1), its eigenvalues by jacobi_sym (me_horn.hpp), clamped at 0
//                  and ordered l1 >= l2 >= l3.  The point is valid iff k >= min_k and l1 > 0; an invalid point stores zeros.
//                  Per block: the partial sums of l3, linearity, planarity, sphericity, surface variation, k and the valid count.
//                  The rows of block partials are added in block order by me_reduce.hpp's row_sum_device
//                                                                                                     (me_local_geometry, "local_geom")
//   k_lg_unpermute the per-point results, kept in SORTED order on the cloud, back in cloud order           (me_local_geometry_fetch)
//   k_local_geom_normals  the same pass (one body, a template flag) for me_radius_normals ("radius_normals"): it also keeps the column of Jacobi's V that belongs
//                  to the smallest eigenvalue, scaled to unit length and optionally turned towards a viewpoint, and stores it in the
//                  cloud's normals (CLOUD order) — three more stores per point, no second pass over the moments
// The file is compiled with -ffp-contract=off: tests/_localgeom_ref.py and tests/_surface_ref.py restate the neighbour test.
#include <algorithm>
#include <cmath>

#include "me_horn.hpp"
#include "me_internal.hpp"
#include "me_reduce.hpp"
#include "me_wave_stream.hpp"

namespace me {

namespace {

constexpr int kLgSums = 7;  // rows of block partials: l3, linearity, planarity, sphericity, surface variation (double); k, valid points (int64)
constexpr unsigned long long kLgIntRows = 0x60ull;

// what k_local_geom_normals needs beyond the eigenvalues (unused by k_local_geom)
struct LgNormalArgs {
    double *normals;  // double[n][3], cloud order
    double vx, vy, vz;
    int have_view, invalid_z;
};

// One kernel: the streaming loop alone needs 76 VGPRs (the 9 fp64 sums, the query, d and its products next to the stream's own
// state), the eigen-solve epilogue brings the kernel to 78 — 6 waves per SIMD either way, no scratch — so a second launch for the
// epilogue would only add 152 bytes of traffic per point (measured at compile time both ways: DESIGN.md section 4.10).
// NORMALS: the eigenvector of the smallest eigenvalue goes to na.normals; the eigenvalue path is the same code, and k_local_geom, the
// <false> instantiation, is the kernel as it was (78 VGPRs, no scratch, 6 waves per SIMD).
template <bool NORMALS>
__device__ __forceinline__ void
local_geom_body(const SPoint *__restrict__ sp, const unsigned long long *__restrict__ codes, long long n, const GridView &g, double r2, int min_k,
                double *__restrict__ eig_s, int *__restrict__ k_s, unsigned char *__restrict__ valid_s, RedWord *__restrict__ part,
                unsigned int nb, const LgNormalArgs &na) {
    __shared__ WaveTile s_tile[4];
    __shared__ int2 s_tab[4][kGroupTab + 1];
    __shared__ double smd[4];
    __shared__ long long smi[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const StreamQuery q = stream_query(sp, codes, i, n, g.shift);
    int cnt = 0;
    double sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    wave_stream(q.active, q.cx, q.cy, q.cz, sp, g, lane, s_tab[w], &s_tile[w], [&](double px, double py, double pz, int, int) {
        // d2 is dist2_exact(q, p) up to the sign of d, which the squares drop: the set is the library's
        const double dx = px - q.qx, dy = py - q.qy, dz = pz - q.qz;
        if ((dx * dx + dy * dy) + dz * dz < r2) {
            ++cnt;
            sx += dx;
            sy += dy;
            sz += dz;
            sxx += dx * dx;
            sxy += dx * dy;
            sxz += dx * dz;
            syy += dy * dy;
            syz += dy * dz;
            szz += dz * dz;
        }
    });
    // the query itself (d = 0: it added nothing to the sums) is removed once; its coincident duplicates stay
    const int k = q.active ? cnt - 1 : 0;
    double l1 = 0, l2 = 0, l3 = 0;
    bool ok = false;
    double nx = 0, ny = 0, nz = 0;
    if (q.active && k >= min_k) {
        const double kd = (double) k, km = (double) (k - 1);
        double a[9], d[3], V[9];
        a[0] = (sxx - sx * sx / kd) / km;
        a[4] = (syy - sy * sy / kd) / km;
        a[8] = (szz - sz * sz / kd) / km;
        a[1] = a[3] = (sxy - sx * sy / kd) / km;
        a[2] = a[6] = (sxz - sx * sz / kd) / km;
        a[5] = a[7] = (syz - sy * sz / kd) / km;
        jacobi_sym(3, a, d, V);
        double e0 = fmax(d[0], 0.0), e1 = fmax(d[1], 0.0), e2 = fmax(d[2], 0.0);
        double t;
        if (e0 < e1) t = e0, e0 = e1, e1 = t;
        if (e1 < e2) t = e1, e1 = e2, e2 = t;
        if (e0 < e1) t = e0, e0 = e1, e1 = t;
        ok = e0 > 0.0;
        if (ok) l1 = e0, l2 = e1, l3 = e2;
        if (NORMALS && ok) {
            // the column of the smallest eigenvalue before the clamp, the lowest index among equal ones (selects, not a
            // dynamic index: V stays in registers)
            const bool b1 = d[1] < d[0];
            const double dm = b1 ? d[1] : d[0];
            const bool b2 = d[2] < dm;
            nx = b2 ? V[2] : (b1 ? V[1] : V[0]);
            ny = b2 ? V[5] : (b1 ? V[4] : V[3]);
            nz = b2 ? V[8] : (b1 ? V[7] : V[6]);
            const double len = sqrt((nx * nx + ny * ny) + nz * nz);
            nx /= len;
            ny /= len;
            nz /= len;
            if (na.have_view) {
                // the query is read AGAIN here and below (volatile: the compiler may not keep the first copy), so that neither its
                // coordinates nor its index stay in registers across the eigen-solve: that is what keeps this kernel within 80 VGPRs
                // without scratch
                const volatile double *qv = &sp[i].x;
                const double vx = na.vx - qv[0], vy = na.vy - qv[1], vz = na.vz - qv[2];
                if ((nx * vx + ny * vy) + nz * vz < 0.0) nx = -nx, ny = -ny, nz = -nz;
            }
        }
    }
    if (q.active) {
        eig_s[3 * i] = l1;
        eig_s[3 * i + 1] = l2;
        eig_s[3 * i + 2] = l3;
        k_s[i] = k;
        valid_s[i] = ok ? 1 : 0;
        if (NORMALS) {  // the point's place in the cloud: a permutation of [0, n)
            const long long o = *(const volatile long long *) &sp[i].idx;
            na.normals[3 * o] = nx;
            na.normals[3 * o + 1] = ny;
            na.normals[3 * o + 2] = (!ok && na.invalid_z) ? 1.0 : nz;
        }
    }
    // (the denominators are > 0 on a valid point; every other lane adds zeros)
    const double lin = ok ? (l1 - l2) / l1 : 0.0, pla = ok ? (l2 - l3) / l1 : 0.0, sph = ok ? l3 / l1 : 0.0;
    const double sv = ok ? l3 / ((l1 + l2) + l3) : 0.0;
    const double b0 = block_sum_256(l3, smd);
    const double b1 = block_sum_256(lin, smd);
    const double b2 = block_sum_256(pla, smd);
    const double b3 = block_sum_256(sph, smd);
    const double b4 = block_sum_256(sv, smd);
    const long long b5 = block_sum_256_ll(ok ? (long long) k : 0, smi);
    const long long b6 = block_sum_256_ll(ok ? 1 : 0, smi);
    if (threadIdx.x == 0) {
        part[0 * (size_t) nb + blockIdx.x].d = b0;
        part[1 * (size_t) nb + blockIdx.x].d = b1;
        part[2 * (size_t) nb + blockIdx.x].d = b2;
        part[3 * (size_t) nb + blockIdx.x].d = b3;
        part[4 * (size_t) nb + blockIdx.x].d = b4;
        part[5 * (size_t) nb + blockIdx.x].i = b5;
        part[6 * (size_t) nb + blockIdx.x].i = b6;
    }
}

__global__ void __launch_bounds__(256)
k_local_geom(const SPoint *__restrict__ sp, const unsigned long long *__restrict__ codes, long long n, GridView g, double r2, int min_k,
             double *__restrict__ eig_s, int *__restrict__ k_s, unsigned char *__restrict__ valid_s, RedWord *__restrict__ part,
             unsigned int nb) {
    local_geom_body<false>(sp, codes, n, g, r2, min_k, eig_s, k_s, valid_s, part, nb, LgNormalArgs{});
}

// the sibling of me_radius_normals: keeping V through the eigen-solve costs registers the eigenvalue kernel does not pay, so this one
// alone is held to six waves per SIMD (80 VGPRs) by the attribute — the resource lines of both are in DESIGN.md section 4.14
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 6)))
k_local_geom_normals(const SPoint *__restrict__ sp, const unsigned long long *__restrict__ codes, long long n, GridView g, double r2, int min_k,
                     double *__restrict__ eig_s, int *__restrict__ k_s, unsigned char *__restrict__ valid_s, RedWord *__restrict__ part,
                     unsigned int nb, LgNormalArgs na) {
    local_geom_body<true>(sp, codes, n, g, r2, min_k, eig_s, k_s, valid_s, part, nb, na);
}

__global__ void __launch_bounds__(256)
k_lg_unpermute(const SPoint *__restrict__ sp, long long n, const double *__restrict__ eig_s, const int *__restrict__ k_s,
               const unsigned char *__restrict__ valid_s, double *__restrict__ eig_o, int *__restrict__ k_o,
               unsigned char *__restrict__ valid_o) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long o = sp[i].idx;
    if (eig_o) {
        eig_o[3 * o] = eig_s[3 * i];
        eig_o[3 * o + 1] = eig_s[3 * i + 1];
        eig_o[3 * o + 2] = eig_s[3 * i + 2];
    }
    if (k_o) k_o[o] = k_s[i];
    if (valid_o) valid_o[o] = valid_s[i];
}

}  // namespace

namespace {

// the pass of me_local_geometry (nrm == nullptr) and of me_radius_normals: the per-point results on the slot, the seven totals in h
int run_local_geom(me_ctx *ctx, int slot, double radius, int min_k, const LgNormalArgs *nrm, const char *who, RedWord h[7]) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, who));
    if (!(radius > 0) || !std::isfinite(radius)) return ctx->fail(ME_ERR_ARG, std::string(who) + ": radius must be finite and > 0");
    if (min_k < 2) return ctx->fail(ME_ERR_ARG, std::string(who) + ": min_k must be >= 2 (the covariance divides by k - 1)");
    Cloud &c = ctx->cloud[slot];
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    // the radius grid, rebuilt as me_mme / me_radius_outlier do: the 27-cell stencil is exact when the cell edge is >= r
    const double want_h = radius * (1.0 + 0x1p-20);
    if (!c.index_valid || c.cell_h < want_h || c.cell_h > 1.5 * want_h) {
        const double req = c.cell_size_req;
        ME_TRY(cloud_build_index(ctx, slot, radius));
        c.cell_size_req = req;
    }
    const long long n = c.n;
    c.lg_have = false;
    ME_CHECK(ctx, c.lg_eig.ensure((size_t) n * 24));
    ME_CHECK(ctx, c.lg_k.ensure((size_t) n * 4));
    ME_CHECK(ctx, c.lg_val.ensure((size_t) n));
    const unsigned int nb = blocks_of(n);
    ME_CHECK(ctx, ctx->red.ensure(row_sum_bytes(kLgSums, nb)));
    RedWord *part = row_sum_part(ctx), *tot;
    {
        TimerScope ts(ctx, nrm ? "radius_normals" : "local_geom");
        if (nrm) {
            c.have_normals = false;  // (the pass overwrites them: whatever was there is gone even if the call fails afterwards)
            c.orient_have = false;
            ME_CHECK(ctx, c.normals.ensure((size_t) n * 24));
            LgNormalArgs na = *nrm;
            na.normals = c.normals.as<double>();
            hipLaunchKernelGGL(k_local_geom_normals, dim3(nb), dim3(256), 0, ctx->stream, c.sp.as<SPoint>(), c.codes.as<unsigned long long>(), n,
                               c.grid, radius * radius, min_k, c.lg_eig.as<double>(), c.lg_k.as<int>(), c.lg_val.as<unsigned char>(), part, nb, na);
        } else {
            hipLaunchKernelGGL(k_local_geom, dim3(nb), dim3(256), 0, ctx->stream, c.sp.as<SPoint>(), c.codes.as<unsigned long long>(), n,
                               c.grid, radius * radius, min_k, c.lg_eig.as<double>(), c.lg_k.as<int>(), c.lg_val.as<unsigned char>(), part, nb);
        }
        tot = row_sum_device<kLgIntRows>(ctx, kLgSums, nb);
    }
    ME_CHECK(ctx, hipGetLastError());
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, h, tot, kLgSums * sizeof(RedWord)));
        ME_TRY(mg.sync());
    }
    c.lg_have = true;
    ++c.lg_serial;
    return ME_OK;
}

}  // namespace

int local_geometry(me_ctx *ctx, int slot, double radius, int min_k, me_local_geom_out *out) {
    RedWord h[7];
    ME_TRY(run_local_geom(ctx, slot, radius, min_k, nullptr, "me_local_geometry", h));
    const long long n = ctx->cloud[slot].n;
    if (out) {
        out->n = n;
        out->n_valid = h[6].i;
        out->sum_l3 = h[0].d;
        out->sum_linearity = h[1].d;
        out->sum_planarity = h[2].d;
        out->sum_sphericity = h[3].d;
        out->sum_surface_variation = h[4].d;
        out->sum_k = h[5].i;
    }
    return ME_OK;
}

int radius_normals(me_ctx *ctx, int slot, double radius, int min_k, const double *viewpoint, int invalid_z, me_radius_normals_out *out) {
    if (!out) return ctx->fail(ME_ERR_ARG, "me_radius_normals: out is NULL");
    LgNormalArgs na{};
    if (viewpoint) {
        if (!std::isfinite(viewpoint[0]) || !std::isfinite(viewpoint[1]) || !std::isfinite(viewpoint[2]))
            return ctx->fail(ME_ERR_ARG, "me_radius_normals: the viewpoint must be finite");
        na.vx = viewpoint[0], na.vy = viewpoint[1], na.vz = viewpoint[2];
        na.have_view = 1;
    }
    na.invalid_z = invalid_z != 0;
    RedWord h[7];
    ME_TRY(run_local_geom(ctx, slot, radius, min_k, &na, "me_radius_normals", h));
    Cloud &c = ctx->cloud[slot];
    c.have_normals = true;
    c.have_cov = false;
    c.fpfh_valid = false;
    out->n = c.n;
    out->n_valid = h[6].i;
    out->sum_k = h[5].i;
    return ME_OK;
}

int local_geometry_fetch(me_ctx *ctx, int slot, double *eig, int32_t *k, uint8_t *valid) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_local_geometry_fetch"));
    Cloud &c = ctx->cloud[slot];
    if (!c.lg_have || !c.index_valid)
        return ctx->fail(ME_ERR_STATE, "me_local_geometry_fetch: no result for this slot (run me_local_geometry; a changed cloud or a new index discards it)");
    if (!eig && !k && !valid) return ME_OK;
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = c.n;
    DevBuf &eo = ctx->tmp[2], &ko = ctx->tmp[3], &vo = ctx->tmp[4];
    if (eig) ME_CHECK(ctx, eo.ensure((size_t) n * 24));
    if (k) ME_CHECK(ctx, ko.ensure((size_t) n * 4));
    if (valid) ME_CHECK(ctx, vo.ensure((size_t) n));
    hipLaunchKernelGGL(k_lg_unpermute, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, c.sp.as<SPoint>(), n, c.lg_eig.as<double>(),
                       c.lg_k.as<int>(), c.lg_val.as<unsigned char>(), eig ? eo.as<double>() : nullptr, k ? ko.as<int>() : nullptr,
                       valid ? vo.as<unsigned char>() : nullptr);
    ME_CHECK(ctx, hipGetLastError());
    if (eig) ME_TRY(copy_d2h(ctx, eig, eo.p, (size_t) n * 24));
    if (k) ME_TRY(copy_d2h(ctx, k, ko.p, (size_t) n * 4));
    if (valid) ME_TRY(copy_d2h(ctx, valid, vo.p, (size_t) n));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

}  // namespace me
