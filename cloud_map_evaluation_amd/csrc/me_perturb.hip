// me_perturb.hip — the reference's simulation mode (evaluate_noised_gt): a perturbed copy of a resident cloud, made on the device.
//
// me_perturb_cloud runs the four generators of MapEval in one fixed order, each switchable:
//   1. addLocalDeformation  (map_eval.cpp:1808-1829)  no randomness
//   2. addNonUniformDensity (:1757-1784)              on the deformed point; stable compaction (the reference's push_back loop)
//   3. addGaussianNoise     (:1745-1755)              on every survivor
//   4. addSparseOutliers    (:1786-1806)              appended after the survivors, gathered from the noised, compacted cloud
// Randomness is counter-based (Philox4x64-10, Random123, key (seed, 0)): every random block is a pure function of (seed, counter),
// so the result depends neither on the launch shape nor on the other stages' settings.  Word assignment (include/mapeval_hip.h):
//   density,  source point i : counter (i, 1, 0, 0)  w0 -> u
//   noise,    source point i : counter (i, 2, 0, 0)  Box-Muller (w0, w1) -> x, y;  (w2, w3) -> z
//   outlier j                : counter (j, 3, 0, 0)  w0 -> base index;  Box-Muller (w1, w2) -> x, y
//                              counter (j, 3, 1, 0)  Box-Muller (w0, w1) -> z
// u = (w >> 11) 2^-53 in [0, 1); the Box-Muller radius word gives ((w >> 11) + 1) 2^-53 in (0, 1]; n = sqrt(-2 ln u1) cos / sin(2 pi u2).
//
// Three passes, as me_voxel_downsample: A keep flags (deform + density draw), exclusive scan, B deform again + noise + scatter to the
// scanned slot (recomputing the deform is cheaper than writing and re-reading 24 B per point), C outliers; then cloud_finish(dst).
#include <cmath>
#include <utility>

#include "me_internal.hpp"
#include "me_philox.hpp"

namespace me {

namespace {

struct PerturbK {
    double cx, cy, cz, radius, strength;  // deform (radius <= 0 or strength == 0: off)
    double sparse, dense, region;         // density (region <= 0: off)
    double sigma;                         // noise (0: off)
    double range;                         // outlier offset scale
    u64 seed;
    int deform, density, noise;
};

// Box-Muller: two N(0, 1) from the words (a, b); a gives the radius, b the angle
__device__ __forceinline__ void box_muller(u64 a, u64 b, double &n0, double &n1) {
    const double r = sqrt(-2.0 * log(u01_open0(a)));
    double s, c;
    sincos((2.0 * M_PI) * u01(b), &s, &c);
    n0 = r * c;
    n1 = r * s;
}

// addLocalDeformation (:1808-1825): d = (p - c).norm() as Eigen computes it, sqrt((dx^2 + dy^2) + dz^2) (-ffp-contract=off: no FMA);
// strict d < R; direction.normalize() divides by the same norm and leaves a zero vector unchanged (Eigen 3.3)
__device__ __forceinline__ void deform_point(const PerturbK &k, double &x, double &y, double &z) {
    const double dx = x - k.cx, dy = y - k.cy, dz = z - k.cz;
    const double d = sqrt((dx * dx + dy * dy) + dz * dz);
    if (!(d < k.radius) || !(d > 0.0)) return;
    const double w = 0.5 * (1.0 + cos(M_PI * d / k.radius));
    x += dx / d * k.strength * w;
    y += dy / d * k.strength * w;
    z += dz / d * k.strength * w;
}

// addNonUniformDensity (:1766-1780) on the (deformed) point: keep iff u < sparse_ratio where sin(x / region pi) sin(y / region pi) > 0,
// u < dense_ratio elsewhere
__device__ __forceinline__ bool keep_point(const PerturbK &k, long long i, double x, double y) {
    const double xn = sin(x / k.region * M_PI), yn = sin(y / k.region * M_PI);
    const double keep = xn * yn > 0 ? k.sparse : k.dense;
    u64 w[4];
    philox_block(k.seed, (u64) i, 1, 0, w);
    return u01(w[0]) < keep;
}

// pass A: keep flag per source point
__global__ void __launch_bounds__(256) k_perturb_keep(const double *__restrict__ src, long long n, PerturbK k,
                                                      unsigned int *__restrict__ flags) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
    if (k.deform) deform_point(k, x, y, z);
    flags[i] = keep_point(k, i, x, y) ? 1u : 0u;
}

// pass B: deform again, add the noise of source index i, write to the survivor's slot (pos == nullptr: density off, slot i)
__global__ void __launch_bounds__(256) k_perturb_scatter(const double *__restrict__ src, long long n, PerturbK k,
                                                         const unsigned int *__restrict__ flags, const unsigned int *__restrict__ pos,
                                                         double *__restrict__ dst) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (pos && !flags[i]) return;
    double x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
    if (k.deform) deform_point(k, x, y, z);
    if (k.noise) {  // addGaussianNoise (:1750-1754): point(a) += N(0, sigma^2)
        u64 w[4];
        philox_block(k.seed, (u64) i, 2, 0, w);
        double nx, ny, nz, unused;
        box_muller(w[0], w[1], nx, ny);
        box_muller(w[2], w[3], nz, unused);
        x += k.sigma * nx;
        y += k.sigma * ny;
        z += k.sigma * nz;
    }
    const long long o = pos ? (long long) pos[i] : i;
    dst[3 * o] = x;
    dst[3 * o + 1] = y;
    dst[3 * o + 2] = z;
}

// pass C, addSparseOutliers (:1795-1805): outlier j = point b of the noised, compacted cloud + N(0, range^2) per axis, appended at
// n_kept + j.  b = (int64)(u n_kept), clamped to n_kept - 1: a guard, since with a 53-bit u < 1 the product stays below n_kept for any
// n_kept < 2^53, where the reference's draw may round to 1.0 and index one past the end
__global__ void __launch_bounds__(256) k_perturb_outliers(double *__restrict__ pts, long long n_kept, long long m, PerturbK k) {
    const long long j = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    u64 w[4], v[4];
    philox_block(k.seed, (u64) j, 3, 0, w);
    philox_block(k.seed, (u64) j, 3, 1, v);
    long long b = (long long) (u01(w[0]) * (double) n_kept);
    if (b > n_kept - 1) b = n_kept - 1;
    double nx, ny, nz, unused;
    box_muller(w[1], w[2], nx, ny);
    box_muller(v[0], v[1], nz, unused);
    const double x = pts[3 * b] + k.range * nx, y = pts[3 * b + 1] + k.range * ny, z = pts[3 * b + 2] + k.range * nz;
    pts[3 * (n_kept + j)] = x;
    pts[3 * (n_kept + j) + 1] = y;
    pts[3 * (n_kept + j) + 2] = z;
}


inline bool unit_interval(double v) { return v >= 0.0 && v <= 1.0; }

}  // namespace

int perturb_cloud(me_ctx *ctx, int dst_slot, int src_slot, const me_perturb_params *p, long long *n_out) {
    if (dst_slot < 0 || dst_slot > 1 || src_slot < 0 || src_slot > 1) return ctx->fail(ME_ERR_ARG, "me_perturb_cloud: bad slot");
    if (!p) return ctx->fail(ME_ERR_ARG, "me_perturb_cloud: params is NULL");
    if (ctx->shard_world != 1 || ctx->slab.axis >= 0 || ctx->cloud[src_slot].slab.axis >= 0 || ctx->cloud[dst_slot].slab.axis >= 0)
        return ctx->fail(ME_ERR_ARG, "me_perturb_cloud: single GPU only (no slab or shard mode)");
    if (!(p->noise_std >= 0) || !std::isfinite(p->noise_std))
        return ctx->fail(ME_ERR_ARG, "me_perturb_cloud: noise_std must be finite and >= 0");
    if (!unit_interval(p->sparse_ratio) || !unit_interval(p->dense_ratio) || !unit_interval(p->outlier_ratio))
        return ctx->fail(ME_ERR_ARG, "me_perturb_cloud: sparse_ratio, dense_ratio and outlier_ratio must lie in [0, 1]");
    if (!(p->outlier_range >= 0) || !std::isfinite(p->outlier_range))
        return ctx->fail(ME_ERR_ARG, "me_perturb_cloud: outlier_range must be finite and >= 0");
    const bool deform_on = p->deform_radius > 0 && p->deform_strength != 0;
    if (deform_on && (!std::isfinite(p->deform_strength) || !std::isfinite(p->deform_center[0]) || !std::isfinite(p->deform_center[1]) ||
                      !std::isfinite(p->deform_center[2])))  // (radius = +inf stays legal: w = 1, a rigid push by strength)
        return ctx->fail(ME_ERR_ARG, "me_perturb_cloud: deform_strength and deform_center must be finite while the deform stage is on");
    Cloud &S = ctx->cloud[src_slot];
    if (!S.uploaded) return ctx->fail(ME_ERR_STATE, "me_perturb_cloud: source cloud not uploaded");
    if (S.n == 0)  // (a me_mesh_scan without a hit leaves this, as need_single_gpu_cloud notes: nothing to scan, no pos[n - 1] to read)
        return ctx->fail(ME_ERR_STATE, "me_perturb_cloud: the slot's cloud is empty");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = S.n;
    PerturbK k{};
    k.deform = deform_on;
    k.cx = p->deform_center[0];
    k.cy = p->deform_center[1];
    k.cz = p->deform_center[2];
    k.radius = p->deform_radius;
    k.strength = p->deform_strength;
    k.density = p->region_size > 0;
    k.sparse = p->sparse_ratio;
    k.dense = p->dense_ratio;
    k.region = p->region_size;
    k.noise = p->noise_std != 0;
    k.sigma = p->noise_std;
    k.range = p->outlier_range;
    k.seed = p->seed;
    DevBuf &flags = ctx->tmp[0], &pos = ctx->tmp[1];
    long long n_kept = n;
    TimerScope ts(ctx, "perturb");
    if (k.density) {
        ME_CHECK(ctx, flags.ensure((size_t) n * 4));
        ME_CHECK(ctx, pos.ensure((size_t) n * 4));
        hipLaunchKernelGGL(k_perturb_keep, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, S.xyz.as<double>(), n, k,
                           flags.as<unsigned int>());
        ME_TRY(exclusive_scan_u32(ctx, flags.as<unsigned int>(), pos.as<unsigned int>(), n));
        unsigned int last_pos = 0, last_flag = 0;
        {
            MailGuard mg(ctx);  // (one synchronisation for the pair; destinations are locals of this frame)
            ME_TRY(mail_post(ctx, &last_pos, pos.as<unsigned int>() + (n - 1), 4));
            ME_TRY(mail_post(ctx, &last_flag, flags.as<unsigned int>() + (n - 1), 4));
            ME_TRY(mg.sync());
        }
        n_kept = (long long) last_pos + last_flag;
    }
    const long long m = p->outlier_ratio > 0 ? (long long) ((double) n_kept * p->outlier_ratio) : 0;  // (int)(size * ratio) (:1792)
    const long long total = n_kept + m;
    if (n_kept == 0) return ctx->fail(ME_ERR_ARG, "me_perturb_cloud: the density stage kept no point");
    if (total >= (1LL << 31)) return ctx->fail(ME_ERR_ARG, "me_perturb_cloud: the output must hold < 2^31 points (the upload's limit)");
    // nothing of dst has changed up to here.  In place, the passes write a scratch buffer that is then swapped in.
    Cloud &D = ctx->cloud[dst_slot];
    const bool in_place = dst_slot == src_slot;
    DevBuf scratch;
    DevBuf &out = in_place ? scratch : D.xyz;
    ME_CHECK(ctx, out.ensure((size_t) total * 24));  // (a borrowed dst buffer is the caller's: ensure() replaces it by an own one)
    hipLaunchKernelGGL(k_perturb_scatter, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, S.xyz.as<double>(), n, k,
                       k.density ? flags.as<unsigned int>() : nullptr, k.density ? pos.as<unsigned int>() : nullptr,
                       out.as_mut<double>());
    if (m > 0)
        hipLaunchKernelGGL(k_perturb_outliers, dim3(blocks_of(m)), dim3(256), 0, ctx->stream, out.as_mut<double>(), n_kept, m, k);
    ME_CHECK(ctx, hipGetLastError());
    ts.end();
    if (in_place) {
        std::swap(D.xyz.p, scratch.p);
        std::swap(D.xyz.bytes, scratch.bytes);
        std::swap(D.xyz.owned, scratch.owned);
        ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the old buffer is freed with `scratch`)
    }
    // the upload-time reset of dst (cloud_upload): index, NN, MME, voxel state and per-point attributes are gone
    D.uploaded = false;
    D.index_valid = false;
    D.vox_size = 0;
    drop_point_results(ctx, dst_slot);
    D.n = total;
    D.n_total = total;
    D.have_normals = D.have_cov = false;
    D.slab = ctx->slab;
    D.n_unres = 0;
    D.slab_identity = true;
    D.cell_size_req = S.cell_size_req;
    if (n_out) *n_out = total;
    return cloud_finish(ctx, dst_slot);
}

}  // namespace me
