// me_point_order.hpp — THE POINTS' OWN ORDER of a resident cloud on a voxel lattice, shared by me_deform.hip and me_voxdist.hip: every
// point's voxel key (voxel_key_of) filed under its ORIGINAL index, and a stable sort by key.  The result lists the points grouped by
// voxel in ascending key order, inside a voxel in ascending original index.  The sorted (Hilbert) order of the cloud, which changes
// with the index's cell size, decides nothing: what is summed in this order is bit-identical after any re-sort of the same points.
#pragma once

#include "me_internal.hpp"
#include "me_vox_rows.hpp"

#ifdef __HIPCC__
namespace me {

// okey[o] = the voxel key of the point with original index o, opos[o] = its position in the sorted cloud
static __global__ void __launch_bounds__(256)
k_point_order(const SPoint *__restrict__ sp, long long n, double vs, SlabView slab, unsigned long long *__restrict__ okey,
              unsigned int *__restrict__ opos, int *__restrict__ err) {
    const long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const SPoint p = sp[s];
    if (p.idx < 0 || p.idx >= n) {  // (never: the sorted cloud is a permutation of the uploaded one)
        *err = 1;
        return;
    }
    okey[p.idx] = voxel_key_of(p.x, p.y, p.z, vs, slab, err);
    opos[p.idx] = (unsigned int) s;
}

// HOST: skey_d[i] / spos_d[i] = the voxel key and the sorted-cloud position of entry i of the points' own order (n entries).  `err`: a
// device int the caller has zeroed on the stream; the kernel runs under the device timer `timer`, the sort under "sort".  ME_ERR_ARG
// (in `who`'s name) when a voxel index is out of range.  The stream is synchronised once (the range check).
static inline int points_own_order(me_ctx *ctx, const Cloud &q, double voxel_size, int *err, const char *timer, const char *who,
                                   DevBuf &okey_d, DevBuf &opos_d, DevBuf &skey_d, DevBuf &spos_d) {
    const long long n = q.n;
    ME_CHECK(ctx, okey_d.ensure((size_t) n * 8));
    ME_CHECK(ctx, opos_d.ensure((size_t) n * 4));
    ME_CHECK(ctx, skey_d.ensure((size_t) n * 8));
    ME_CHECK(ctx, spos_d.ensure((size_t) n * 4));
    ME_CHECK(ctx, hipMemsetAsync(opos_d.p, 0xFF, (size_t) n * 4, ctx->stream));  // (an entry no point files: no position, no pair)
    ME_CHECK(ctx, hipMemsetAsync(okey_d.p, 0, (size_t) n * 8, ctx->stream));
    {
        TimerScope ts(ctx, timer);
        hipLaunchKernelGGL(k_point_order, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, voxel_size, q.slab,
                           okey_d.as<unsigned long long>(), opos_d.as<unsigned int>(), err);
    }
    {
        unsigned int h_err = 0;
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h_err, err, 4));
        ME_TRY(mg.sync());
        if (h_err) return ctx->fail(ME_ERR_ARG, std::string(who) + ": voxel index out of range (|floor(p/voxel_size)| must be < 2^20)");
    }
    return sort_pairs_u64_u32(ctx, okey_d.as<unsigned long long>(), skey_d.as<unsigned long long>(), opos_d.as<unsigned int>(),
                              spos_d.as<unsigned int>(), n, 0, 64);  // (a radix sort: stable)
}

}  // namespace me
#endif
