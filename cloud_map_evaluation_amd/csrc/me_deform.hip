// me_deform.hip — the per-voxel rigid deformation field from the resident 1-NN pairs (me_voxel_deformation; no reference counterpart:
// map_eval.cpp reports scalars only).  DESIGN.md section 4.22.
//
// Which way has this part of the map moved, and by how much: the pair moments me_icp_p2p_sums forms for the whole cloud, formed per
// voxel of the AWD lattice (the rows of me_voxel_gaussians: voxel_key_of, ascending keys), a rigid fit per voxel (me_horn.hpp) and
// what the fit leaves of the squared error.
//   pass 0  k_point_order      THE ORDER OF THE SUMS IS THE POINTS' OWN: every point's voxel key, filed under its ORIGINAL index, and a
//                              stable sort by key: the points grouped by voxel, inside a voxel in ascending original index.  The
//                              sorted (Hilbert) order of the cloud, which changes with the index's cell size, decides nothing:
//                              the rows are bit-identical after any re-sort of the same points.
//   pass 1  k_deform_records   ONE pass over that order, a row of 64 points reduced run by run exactly as k_voxm_records does
//                              it (me_voxel.hip): wave_sum_to_lane0 when the row is one run, seg_sum_to_head otherwise, two record
//                              slots per row, the further runs in the overflow regions, the retry when a region overflows.  A
//                              record: the pair count and 23 doubles about the voxel's CENTRE (|a| <= half a voxel diagonal).
//   pass 2  k_deform_reduce    the records sorted by (row, run), then stably by voxel key (vox_record_segments); one wavefront per
//                              voxel adds them in that fixed order.  No floating-point atomics anywhere.
//   pass 3  k_deform_fit       one lane per voxel, plain arithmetic only (+ - * /, sqrt, fabs, jacobi_sym, horn_rotation): the
//                              numpy model of tests/_deform_ref.py restates it operation by operation (-ffp-contract=off).
//   pass 4  k_deform_totals    the totals over the rows in key order by the shared fixed-order reduction (me_reduce.hpp).
// A lane forms each of its 23 terms right before that term's reduction and the head lane stores the sum at once (the record's slot
// depends on the keys alone and is known before the first sum): the pass never holds 23 accumulators.
#include <cmath>
#include <cstring>

#include "me_horn.hpp"
#include "me_internal.hpp"
#include "me_point_order.hpp"
#include "me_reduce.hpp"
#include "me_vox_rows.hpp"

namespace me {
namespace {

constexpr int kDfD = ME_DEFORM_SUMS;  // sum a (3), sum b (3), sum a b^T (9), sum a a^T (6), sum |b|^2, sum d2
constexpr int kDfBlocks = 1024;       // blocks of the totals pass at most; part of the order
constexpr int kDfND = 6, kDfNI = 4;   // totals: n|t0|, n|t0|^2, e0, e_t, e0_fit, e_R | with pairs, FIT, ROT_OK, pairs
typedef RedBufs<kDfND, kDfNI> DfRed;

// term k of a pair (a, b, d2); a non-pair passes zeros
template <int K>
__device__ __forceinline__ double deform_term(const double (&a)[3], const double (&b)[3], double d2) {
    if (K < 3) return a[K];
    if (K < 6) return b[K - 3];
    if (K < 15) return a[(K - 6) / 3] * b[(K - 6) % 3];
    if (K == 15) return a[0] * a[0];
    if (K == 16) return a[0] * a[1];
    if (K == 17) return a[0] * a[2];
    if (K == 18) return a[1] * a[1];
    if (K == 19) return a[1] * a[2];
    if (K == 20) return a[2] * a[2];
    if (K == 21) return (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    return d2;
}

template <int K, bool ONE>
__device__ __forceinline__ void deform_sum_store(const double (&a)[3], const double (&b)[3], double d2, int seg, int lane, bool store,
                                                 double *__restrict__ dst) {
    double v = deform_term<K>(a, b, d2);
    v = ONE ? wave_sum_to_lane0(v) : seg_sum_to_head(v, seg, lane);
    if (store) dst[K] = v;
    if constexpr (K + 1 < kDfD) deform_sum_store<K + 1, ONE>(a, b, d2, seg, lane, store, dst);
}

// lane = entry i of the points' own order: skey[i] its voxel key, spos[i] its position in the sorted cloud (where d2 and idx lie)
__global__ void __launch_bounds__(256)
k_deform_records(const unsigned long long *__restrict__ skey, const unsigned int *__restrict__ spos, const SPoint *__restrict__ sp,
                 const double *__restrict__ d2s, const int *__restrict__ idxs, const double *__restrict__ ref_xyz, long long n_ref,
                 long long n, double vs, double gate2, unsigned long long *__restrict__ rec_pos, unsigned long long *__restrict__ rec_vkey,
                 unsigned int *__restrict__ rec_c, double *__restrict__ rec_d, unsigned int *__restrict__ region_count, unsigned int n_rows,
                 unsigned int region_size) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < n;
    unsigned long long key = ~0ULL;
    bool pair = false;
    double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, d2 = 0.0;
    if (valid) {
        key = skey[i];
        const long long s = spos[i];
        const double d = s < n ? d2s[s] : -1.0;
        const long long j = s < n ? idxs[s] : -1;
        // SearchHybrid(q, max, 1): d2 < max^2 [Open3D, upstream], as k_icp_p2p; j names a reference point (me_set_nn_result leaves -1)
        pair = d >= 0.0 && d < gate2 && j >= 0 && j < n_ref;
        if (pair) {
            const SPoint p = sp[s];
            int kx, ky, kz;
            unpack_key(key, kx, ky, kz);
            const double ox = (double) kx * vs + 0.5 * vs, oy = (double) ky * vs + 0.5 * vs, oz = (double) kz * vs + 0.5 * vs;
            a[0] = p.x - ox, a[1] = p.y - oy, a[2] = p.z - oz;
            b[0] = ref_xyz[3 * j] - ox, b[1] = ref_xyz[3 * j + 1] - oy, b[2] = ref_xyz[3 * j + 2] - oz;
            d2 = d;
        }
    }
    const unsigned long long prev = __shfl_up(key, 1, 64);
    const bool head = valid && (lane == 0 || key != prev);
    const unsigned long long hm = __ballot(head);
    if (!hm) return;  // (a row past the end)
    const int run_local = __popcll(hm & ((2ULL << lane) - 1ULL)) - 1;
    // record slots as vox_emit_row (me_vox_rows.hpp): two per row, the further runs of a row in the overflow region r mod kVoxRegions
    unsigned int base = 0;
    const int extra = __popcll(hm) - 2;
    const unsigned int region = (unsigned int) (i >> 6) & (kVoxRegions - 1);
    if (extra > 0) {
        if (lane == 0) base = atomicAdd(region_count + region, (unsigned int) extra);
        base = (unsigned int) __builtin_amdgcn_readfirstlane((int) base);
    }
    const bool fits = run_local < 2 || base + (unsigned int) (run_local - 2) < region_size;
    const unsigned long long r = run_local < 2 ? 2ULL * (unsigned long long) (i >> 6) + (unsigned long long) run_local
                                               : 2ULL * n_rows + (unsigned long long) region * region_size + base + (unsigned long long) (run_local - 2);
    const bool store = head && fits;
    double *dst = rec_d + (size_t) kDfD * (store ? r : 0ULL);
    int cnt;
    if (hm == 1ULL) {  // the row is one run: plain sums on the vector unit
        cnt = __popcll(__ballot(pair));
        deform_sum_store<0, true>(a, b, d2, 0, lane, store, dst);
    } else {
        const int seg = valid ? run_local : 64 + lane;
        cnt = seg_sum_to_head_i(pair ? 1 : 0, seg, lane);
        deform_sum_store<0, false>(a, b, d2, seg, lane, store, dst);
    }
    if (store) {
        rec_pos[r] = ((unsigned long long) (i >> 6) << 6) | (unsigned long long) run_local;
        rec_vkey[r] = key;
        rec_c[r] = (unsigned int) cnt;
    }
}

// one wavefront per voxel: its records in sorted order (= the points' own order) -> one row
__global__ void __launch_bounds__(256)
k_deform_reduce(const unsigned int *__restrict__ perm, const unsigned int *__restrict__ seg_start, const unsigned long long *__restrict__ vkey,
                long long n_vox, const unsigned int *__restrict__ rec_c, const double *__restrict__ rec_d, int *__restrict__ keys3,
                long long *__restrict__ n_pairs, double *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const long long v = (long long) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= n_vox) return;
    const long long b = seg_start[v], e = seg_start[v + 1];
    long long c = 0;
    double s[kDfD];
#pragma unroll
    for (int k = 0; k < kDfD; ++k) s[k] = 0.0;
    for (long long j = b + lane; j < e; j += 64) {
        const long long r = perm[j];
        c += (long long) rec_c[r];
#pragma unroll
        for (int k = 0; k < kDfD; ++k) s[k] += rec_d[kDfD * r + k];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
#pragma unroll
    for (int k = 0; k < kDfD; ++k) s[k] = wave_allsum(s[k]);
    if (lane != 0) return;
    int kx, ky, kz;
    unpack_key(vkey[v], kx, ky, kz);
    keys3[3 * v] = kx;
    keys3[3 * v + 1] = ky;
    keys3[3 * v + 2] = kz;
    n_pairs[v] = c;
#pragma unroll
    for (int k = 0; k < kDfD; ++k) sums[kDfD * v + k] = s[k];
}

// one lane per voxel: the fit from the sums (the header's FIT paragraph, in this order of operations)
__global__ void __launch_bounds__(256)
k_deform_fit(const long long *__restrict__ n_pairs, const double *__restrict__ sums, long long n_vox, int min_pairs, double min_spread,
             unsigned char *__restrict__ flags, double *__restrict__ t0_o, double *__restrict__ u_o, double *__restrict__ R_o,
             double *__restrict__ e_o) {
    const long long v = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vox) return;
    const long long n = n_pairs[v];
    const double *s = sums + kDfD * v;
    double t0[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double e0 = 0.0, et = 0.0, eR = 0.0;
    unsigned char fl = 0;
    if (n > 0) {
        const double dn = (double) n;
        const double sa[3] = {s[0], s[1], s[2]}, sb[3] = {s[3], s[4], s[5]};
        double ab[3], bb[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ab[k] = sa[k] / dn;
            bb[k] = sb[k] / dn;
            t0[k] = bb[k] - ab[k];
            u[k] = t0[k];
        }
        const double tt = dot3(t0, t0);
        e0 = s[22];
        const double rt = s[22] - dn * tt;
        et = rt > 0.0 ? rt : 0.0;
        eR = et;
        if (n >= (long long) min_pairs) {
            fl = ME_DEFORM_FIT;
            const double cxx = s[15] - (sa[0] * sa[0]) / dn, cxy = s[16] - (sa[0] * sa[1]) / dn, cxz = s[17] - (sa[0] * sa[2]) / dn,
                         cyy = s[18] - (sa[1] * sa[1]) / dn, cyz = s[19] - (sa[1] * sa[2]) / dn, czz = s[20] - (sa[2] * sa[2]) / dn;
            double Cm[9] = {cxx, cxy, cxz, cxy, cyy, cyz, cxz, cyz, czz}, d[3], V[9];
            jacobi_sym(3, Cm, d, V);
            // the middle one of the three eigenvalues
            const double lo01 = d[0] < d[1] ? d[0] : d[1], hi01 = d[0] < d[1] ? d[1] : d[0];
            const double mid = d[2] < lo01 ? lo01 : (d[2] < hi01 ? d[2] : hi01);
            if (mid >= dn * (min_spread * min_spread)) {
                fl |= ME_DEFORM_ROT_OK;
                double S[9];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) S[3 * r + c] = s[6 + 3 * r + c] - (sa[r] * sb[c]) / dn;
                horn_rotation(S, R);
#pragma unroll
                for (int r = 0; r < 3; ++r) u[r] = bb[r] - dot3(R + 3 * r, ab);
                const double trC = (cxx + cyy) + czz;
                const double vb = s[21] - dot3(sb, sb) / dn;
                // sum b'^T R a' = tr(R S) = sum_rc R_rc S_cr, row by row of R
                const double sc0[3] = {S[0], S[3], S[6]}, sc1[3] = {S[1], S[4], S[7]}, sc2[3] = {S[2], S[5], S[8]};
                const double trRS = (dot3(R, sc0) + dot3(R + 3, sc1)) + dot3(R + 6, sc2);
                const double rr = (trC + vb) - 2.0 * trRS;
                eR = rr > 0.0 ? rr : 0.0;
            }
        }
    }
    flags[v] = fl;
#pragma unroll
    for (int k = 0; k < 3; ++k) t0_o[3 * v + k] = t0[k], u_o[3 * v + k] = u[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) R_o[9 * v + k] = R[k];
    e_o[3 * v] = e0;
    e_o[3 * v + 1] = et;
    e_o[3 * v + 2] = eR;
}

// the totals over the rows: thread (b, t) takes the rows 256 b + t, + the grid's size, ... in order (me_reduce.hpp)
__global__ void __launch_bounds__(256)
k_deform_totals(const long long *__restrict__ n_pairs, const unsigned char *__restrict__ flags, const double *__restrict__ t0,
                const double *__restrict__ e, long long n_vox, double *__restrict__ pd, long long *__restrict__ pi) {
    double sd[kDfND];
    long long ci[kDfNI];
#pragma unroll
    for (int k = 0; k < kDfND; ++k) sd[k] = 0.0;
#pragma unroll
    for (int k = 0; k < kDfNI; ++k) ci[k] = 0;
    unsigned long long mx = 0ULL;
    long long arg = -1;
    for (long long v = (long long) blockIdx.x * 256 + threadIdx.x; v < n_vox; v += (long long) gridDim.x * 256) {
        const long long n = n_pairs[v];
        const unsigned char fl = flags[v];
        const double dn = (double) n;
        const double tt = dot3(t0 + 3 * v, t0 + 3 * v), tn = sqrt(tt);
        sd[0] += dn * tn;
        sd[1] += dn * tt;
        sd[2] += e[3 * v];
        sd[3] += e[3 * v + 1];
        ci[0] += n > 0 ? 1 : 0;
        ci[3] += n;
        if (fl & ME_DEFORM_FIT) {
            sd[4] += e[3 * v];
            sd[5] += e[3 * v + 2];
            ci[1] += 1;
            ci[2] += (fl & ME_DEFORM_ROT_OK) ? 1 : 0;
            take_max(mx, arg, (unsigned long long) __double_as_longlong(tn), v);  // (|t0| >= 0: its bit pattern orders as it does)
        }
    }
    red_store_partial<kDfND, kDfNI, false>(sd, ci, mx, arg, ~0ULL, pd + (size_t) blockIdx.x * kDfND,
                                           pi + (size_t) blockIdx.x * DfRed::Totals::NR);
}

}  // namespace

int voxel_deformation(me_ctx *ctx, int qslot, double voxel_size, double max_distance, int min_pairs, double min_spread,
                      me_deform_summary *out) {
    if (qslot < 0 || qslot > 1 || !out) return ctx->fail(ME_ERR_ARG, "me_voxel_deformation: bad argument");
    if (!(voxel_size > 0)) return ctx->fail(ME_ERR_ARG, "me_voxel_deformation: voxel_size must be > 0");
    if (!(max_distance > 0)) return ctx->fail(ME_ERR_ARG, "me_voxel_deformation: max_distance must be > 0");
    if (min_pairs < 3) return ctx->fail(ME_ERR_ARG, "me_voxel_deformation: min_pairs must be >= 3");
    if (!(min_spread >= 0)) return ctx->fail(ME_ERR_ARG, "me_voxel_deformation: min_spread must be >= 0");
    Cloud &q = ctx->cloud[qslot];
    if (q.slab.axis >= 0 || ctx->slab.axis >= 0 || ctx->shard_world > 1)
        return ctx->fail(ME_ERR_STATE, "me_voxel_deformation: single GPU only (no slab or shard mode)");
    if (!q.uploaded) return ctx->fail(ME_ERR_STATE, "me_voxel_deformation: cloud not uploaded");
    if (q.nn_ref_slot < 0)
        return ctx->fail(ME_ERR_STATE, "me_voxel_deformation: no me_nn1 with this slot as the query since the last upload or transform of either slot");
    Cloud &ref = ctx->cloud[q.nn_ref_slot];
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    q.dfm_have = false;
    const long long n = q.n;
    const long long n_rows = (n + 63) / 64;
    long long rsize = vox_region_size(n), cap = 0;
    DevBuf &pbuf = ctx->tmp[0], &cbuf = ctx->tmp[1], &dbuf = ctx->tmp[2];  // (tmp[3] - tmp[5]: vox_record_segments)
    ME_CHECK(ctx, ctx->red.ensure(kVoxCounterBytes));
    unsigned int *cnt = ctx->red.as<unsigned int>();  // [range error, fullest region, the regions' counters]
    // the points' own order: by voxel key, inside a voxel by original index (a stable sort of the keys filed by original index)
    DevBuf okey_d, opos_d, skey_d, spos_d;
    ME_CHECK(ctx, hipMemsetAsync(cnt, 0, kVoxCounterBytes, ctx->stream));
    ME_TRY(points_own_order(ctx, q, voxel_size, reinterpret_cast<int *>(cnt), "voxel_deformation", "me_voxel_deformation", okey_d, opos_d,
                            skey_d, spos_d));  // (me_point_order.hpp)
    for (int attempt = 0;; ++attempt) {
        cap = 2 * n_rows + (long long) kVoxRegions * rsize;
        ME_CHECK(ctx, pbuf.ensure((size_t) cap * 16));  // rec_pos | rec_vkey
        ME_CHECK(ctx, cbuf.ensure((size_t) cap * 4));
        ME_CHECK(ctx, dbuf.ensure((size_t) cap * 8 * kDfD));
        ME_CHECK(ctx, hipMemsetAsync(pbuf.p, 0xFF, (size_t) cap * 8, ctx->stream));  // kVoxEmptySlot
        ME_CHECK(ctx, hipMemsetAsync(cnt, 0, kVoxCounterBytes, ctx->stream));
        {
            TimerScope ts(ctx, "voxel_deformation");
            hipLaunchKernelGGL(k_deform_records, dim3(blocks_of(n)), dim3(256), 0, ctx->stream,
                               (const unsigned long long *) skey_d.as<unsigned long long>(), (const unsigned int *) spos_d.as<unsigned int>(),
                               q.sp.as<SPoint>(), q.nn_d2.as<double>(), q.nn_idx.as<int>(), ref.xyz.as<double>(), ref.n, n, voxel_size,
                               max_distance * max_distance, pbuf.as<unsigned long long>(), pbuf.as<unsigned long long>() + cap,
                               cbuf.as<unsigned int>(), dbuf.as<double>(), cnt + 2, (unsigned int) n_rows, (unsigned int) rsize);
        }
        unsigned int h2[2] = {0, 0};
        ME_TRY(vox_region_fill(ctx, cnt, h2));
        if ((long long) h2[1] <= rsize) break;
        if (attempt > 0) return ctx->fail(ME_ERR_HIP, "me_voxel_deformation: overflow regions still too small");
        rsize = (long long) h2[1];  // (a region overflowed: once more with regions as large as the fullest one needs; the same records)
    }
    DevBuf vkey_d, seg_d;
    const unsigned int *perm = nullptr;
    long long V = 0;
    ME_TRY(vox_record_segments(ctx, cap, pbuf.as<unsigned long long>(), pbuf.as<unsigned long long>() + cap, vkey_d, seg_d, &perm, &V));
    ME_CHECK(ctx, q.dfm_keys.ensure((size_t) V * 12));
    ME_CHECK(ctx, q.dfm_n.ensure((size_t) V * 8));
    ME_CHECK(ctx, q.dfm_flags.ensure((size_t) V));
    ME_CHECK(ctx, q.dfm_sums.ensure((size_t) V * 8 * kDfD));
    ME_CHECK(ctx, q.dfm_fit.ensure((size_t) V * 8 * 18));  // t0 [V][3] | u [V][3] | R [V][9] | e [V][3]
    double *fit = q.dfm_fit.as<double>();
    const int nb = (int) std::min<long long>(kDfBlocks, blocks_of(V));
    ME_CHECK(ctx, ctx->red.ensure(DfRed::bytes(kDfBlocks)));  // (the counters of pass 1 are done with)
    const DfRed red(ctx, kDfBlocks);
    {
        TimerScope ts(ctx, "voxel_deformation");
        hipLaunchKernelGGL(k_deform_reduce, dim3((unsigned int) ((V + 3) / 4)), dim3(256), 0, ctx->stream, perm,
                           (const unsigned int *) seg_d.as<unsigned int>(), (const unsigned long long *) vkey_d.as<unsigned long long>(), V,
                           (const unsigned int *) cbuf.as<unsigned int>(), (const double *) dbuf.as<double>(), q.dfm_keys.as<int>(),
                           q.dfm_n.as<long long>(), q.dfm_sums.as<double>());
        hipLaunchKernelGGL(k_deform_fit, dim3(blocks_of(V)), dim3(256), 0, ctx->stream, (const long long *) q.dfm_n.as<long long>(),
                           (const double *) q.dfm_sums.as<double>(), V, min_pairs, min_spread, q.dfm_flags.as<unsigned char>(), fit, fit + 3 * V,
                           fit + 6 * V, fit + 15 * V);
        hipLaunchKernelGGL(k_deform_totals, dim3(nb), dim3(256), 0, ctx->stream, (const long long *) q.dfm_n.as<long long>(),
                           (const unsigned char *) q.dfm_flags.as<unsigned char>(), (const double *) fit, (const double *) (fit + 15 * V), V,
                           red.pd, red.pi);
        red.total(ctx, nb, red.tot);
    }
    ME_CHECK(ctx, hipGetLastError());
    DfRed::Totals h;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h, red.tot, sizeof(h)));
        ME_TRY(mg.sync());  // (the local buffers die with this frame: the stream is idle from here on)
    }
    std::memset(out, 0, sizeof(*out));
    out->n_voxels = V;
    out->n_with_pairs = h.i[0];
    out->n_fit = h.i[1];
    out->n_rot = h.i[2];
    out->n_pairs = h.i[3];
    out->sum_n_t0 = h.d[0];
    out->sum_n_t0sq = h.d[1];
    out->sum_e0 = h.d[2];
    out->sum_e_t = h.d[3];
    out->sum_e0_fit = h.d[4];
    out->sum_e_R = h.d[5];
    out->max_row = h.i[kDfNI + 1];
    if (out->max_row >= 0) {
        std::memcpy(&out->max_t0, &h.i[kDfNI], 8);
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, out->max_key, q.dfm_keys.as<int>() + 3 * out->max_row, 12));
        ME_TRY(mg.sync());
    }
    q.dfm_V = V;
    q.dfm_have = true;
    return ME_OK;
}

int voxel_deformation_fetch(me_ctx *ctx, int qslot, int32_t *keys, int64_t *n_pairs, uint8_t *flags, double *sums, double *t0, double *u,
                            double *R, double *e, int64_t *n_voxels) {
    if (qslot < 0 || qslot > 1 || !n_voxels) return ctx->fail(ME_ERR_ARG, "me_voxel_deformation_fetch: bad argument");
    Cloud &q = ctx->cloud[qslot];
    if (!q.uploaded || q.nn_ref_slot < 0 || !q.dfm_have)
        return ctx->fail(ME_ERR_STATE, "me_voxel_deformation_fetch: no result for this slot (run me_voxel_deformation; it is discarded with the 1-NN result)");
    const long long V = q.dfm_V, capacity = *n_voxels;
    *n_voxels = V;
    if (!(keys || n_pairs || flags || sums || t0 || u || R || e)) return ME_OK;
    if (capacity < V) return ctx->fail(ME_ERR_CAPACITY, "me_voxel_deformation_fetch: capacity too small");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const double *fit = q.dfm_fit.as<double>();
    if (keys) ME_TRY(copy_d2h(ctx, keys, q.dfm_keys.p, (size_t) V * 12));
    if (n_pairs) ME_TRY(copy_d2h(ctx, n_pairs, q.dfm_n.p, (size_t) V * 8));
    if (flags) ME_TRY(copy_d2h(ctx, flags, q.dfm_flags.p, (size_t) V));
    if (sums) ME_TRY(copy_d2h(ctx, sums, q.dfm_sums.p, (size_t) V * 8 * kDfD));
    if (t0) ME_TRY(copy_d2h(ctx, t0, fit, (size_t) V * 24));
    if (u) ME_TRY(copy_d2h(ctx, u, fit + 3 * V, (size_t) V * 24));
    if (R) ME_TRY(copy_d2h(ctx, R, fit + 6 * V, (size_t) V * 72));
    if (e) ME_TRY(copy_d2h(ctx, e, fit + 15 * V, (size_t) V * 24));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

}  // namespace me
