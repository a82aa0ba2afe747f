// me_mom.hip — MOM, the plane variance on mutually orthogonal planes aggregated by exact medians, and the grouped order statistic it
// needs (the definitions are in include/mapeval_hip.h).
// Grouped order statistics of n (key, group byte) pairs — key = the bits of a non-negative double, group in [-1, n_groups):
//   k_gs_init    the counters, extremes and histograms of the state block zeroed
//   k_gs_stat    one tile of kGsTile entries per block: count, smallest and largest key per group through LDS integer atomics and one
//                integer atomic per (block, group) to memory; the group's sum of the tile by a fixed tree (each thread its eight
//                entries in order, then block_sum_256), stored as the block's partial.  A group absent from the tile stores 0.0
//                The rows of block partials are added in block order by me_reduce.hpp's row_sum_device
//   k_gs_start   per group: live = count > 0, the ranks (count - 1) / 2 and count / 2, an empty prefix
//   k_gs_hist    THE HOT KERNEL, once per pass (eight passes of eight bits, from the top) and slice of kGsSlice groups: the entries
//                whose key carries the prefix of a rank found so far add one to the LDS histogram (group, rank slot, digit); a wave whose
//                entries all fall into one bin — the rule in the upper passes, where the keys of a smooth quantity share their exponent
//                — adds its population with one atomic.  At the end one integer atomic per non-empty (block, group, slot, digit)
//   k_gs_narrow  one thread per group: the digit in which each rank falls, the prefix extended, the rank reduced by what lies
//                below.  The lower and the upper rank differ by at most one: they share slot 0 until their digits differ
//   k_gs_out     me_group_stats per group from the counters, the totals and the two finished prefixes
// MOM on a resident cloud:
//   k_mom_gather the points in sorted order: label[sp[i].idx] -> axis through a 2-bit table in two scalar arguments; key = bits of
//                l3 + 0.0, group = the axis when the point is labelled, its direction chosen and its validity byte set, else -1; the
//                same byte into the slot's axis array in cloud order
// The file is compiled with -ffp-contract=off: tests/_mom_ref.py restates the dot product of the axis choice.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "me_internal.hpp"
#include "me_reduce.hpp"

namespace me {

namespace {

typedef unsigned long long u64;

constexpr int kGsMaxGroups = 64;
constexpr int kGsBits = 8;                   // digit width: 2 slots x 256 counters x 4 B = 2 KB of LDS per group
constexpr int kGsBins = 1 << kGsBits;
constexpr int kGsPasses = 64 / kGsBits;
constexpr int kGsSlice = 16;                 // groups per k_gs_hist launch: 32 KB of LDS, five blocks per CU; 64 groups take four slices
constexpr int kGsPts = 8;                    // k_gs_stat: entries per thread
constexpr int kGsTile = 256 * kGsPts;        // ... and per block: the unit of the block-order sum
constexpr unsigned int kGsMaxBlocks = 2048;  // k_gs_hist: above it a block strides over the array (fewer global atomics)

struct GsState {
    u64 prefix[2];       // the digits found so far, in place (the lower bits zero): [0] the lower rank's, [1] the upper rank's
    long long rank[2];   // rank among the entries that carry the prefix
    int same;            // both ranks still carry one prefix: slot 0 counts for both
    int live;            // the group has entries
};

struct GsBlock {
    unsigned int hist[kGsMaxGroups * 2 * kGsBins];
    GsState st[kGsMaxGroups];
    u64 cnt[kGsMaxGroups], mn[kGsMaxGroups], mx[kGsMaxGroups];
    double tot[kGsMaxGroups];
    unsigned int err, pad;
    me_group_stats out[kGsMaxGroups];
};

__global__ void __launch_bounds__(256) k_gs_init(GsBlock *__restrict__ b) {
    for (int t = threadIdx.x; t < kGsMaxGroups * 2 * kGsBins; t += 256) b->hist[t] = 0u;
    if (threadIdx.x < kGsMaxGroups) {
        b->cnt[threadIdx.x] = 0ull;
        b->mn[threadIdx.x] = ~0ull;
        b->mx[threadIdx.x] = 0ull;
    }
}

// the direct entry's inputs -> (key, group byte); an entry outside the contract raises the flag and is ignored
__global__ void __launch_bounds__(256) k_gs_prep(const double *__restrict__ values, const int *__restrict__ group, long long n, int n_groups,
                                                 u64 *__restrict__ keys, signed char *__restrict__ grp, unsigned int *__restrict__ err) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = values[i];
    int g = group[i];
    if (g < -1 || g >= n_groups || (g >= 0 && (!(v >= 0.0) || v == INFINITY))) {
        atomicOr(err, 1u);
        g = -1;
    }
    keys[i] = (u64) __double_as_longlong(v + 0.0);  // (-0.0 + 0.0 = +0.0)
    grp[i] = (signed char) g;
}

__global__ void __launch_bounds__(256)
k_gs_stat(const u64 *__restrict__ keys, const signed char *__restrict__ grp, long long n, int n_groups, GsBlock *__restrict__ b,
          RedWord *__restrict__ part, unsigned int nb) {
    __shared__ unsigned int s_cnt[kGsMaxGroups];
    __shared__ u64 s_mn[kGsMaxGroups], s_mx[kGsMaxGroups];
    __shared__ double sm[4];
    if (threadIdx.x < kGsMaxGroups) {
        s_cnt[threadIdx.x] = 0u;
        s_mn[threadIdx.x] = ~0ull;
        s_mx[threadIdx.x] = 0ull;
    }
    __syncthreads();
    const long long base = (long long) blockIdx.x * kGsTile + threadIdx.x;
    double v[kGsPts];
    int g[kGsPts];
#pragma unroll
    for (int q = 0; q < kGsPts; ++q) {
        const long long i = base + (long long) q * 256;
        v[q] = 0.0;
        g[q] = -1;
        if (i < n) {
            const int gi = grp[i];
            if (gi >= 0 && gi < n_groups) {
                const u64 k = keys[i];
                g[q] = gi;
                v[q] = __longlong_as_double((long long) k);
                atomicAdd(&s_cnt[gi], 1u);
                atomicMin(&s_mn[gi], k);
                atomicMax(&s_mx[gi], k);
            }
        }
    }
    __syncthreads();
    for (int gg = 0; gg < n_groups; ++gg) {
        double r = 0.0;
        if (s_cnt[gg] != 0u) {  // (uniform over the block; a group absent from the tile would sum zeros to 0.0 all the same)
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < kGsPts; ++q) s += g[q] == gg ? v[q] : 0.0;
            r = block_sum_256(s, sm);
        }
        if (threadIdx.x == 0) part[(size_t) gg * nb + blockIdx.x].d = r;
    }
    if ((int) threadIdx.x < n_groups && s_cnt[threadIdx.x] != 0u) {
        atomicAdd(&b->cnt[threadIdx.x], (u64) s_cnt[threadIdx.x]);
        atomicMin(&b->mn[threadIdx.x], s_mn[threadIdx.x]);
        atomicMax(&b->mx[threadIdx.x], s_mx[threadIdx.x]);
    }
}

__global__ void __launch_bounds__(64) k_gs_start(GsBlock *__restrict__ b, int n_groups) {
    const int g = threadIdx.x;
    if (g >= n_groups) return;
    const long long c = (long long) b->cnt[g];
    GsState s;
    s.prefix[0] = s.prefix[1] = 0ull;
    s.rank[0] = c > 0 ? (c - 1) / 2 : 0;
    s.rank[1] = c / 2;
    s.same = 1;
    s.live = c > 0 ? 1 : 0;
    b->st[g] = s;
}

// groups [g0, g0 + ng), ng <= kGsSlice.  mask = the key bits above this pass' digit (0 in the first pass), shift = the bits below it.
// 32 KB of LDS for the histograms; every LDS and global index is bounded by the slice test (gi < ng) and the 8-bit digit.
__global__ void __launch_bounds__(256)
k_gs_hist(const u64 *__restrict__ keys, const signed char *__restrict__ grp, long long n, int g0, int ng, u64 mask, int shift,
          GsBlock *__restrict__ b) {
    __shared__ unsigned int s_h[kGsSlice * 2 * kGsBins];
    __shared__ u64 s_pre[kGsSlice][2];
    __shared__ int s_mode[kGsSlice];  // 0: the group is empty, 1: one prefix, 2: two
    for (int t = threadIdx.x; t < kGsSlice * 2 * kGsBins; t += 256) s_h[t] = 0u;
    if ((int) threadIdx.x < kGsSlice) {
        int mode = 0;
        u64 p0 = 0, p1 = 0;
        if ((int) threadIdx.x < ng) {
            const GsState s = b->st[g0 + threadIdx.x];
            mode = s.live ? (s.same ? 1 : 2) : 0;
            p0 = s.prefix[0];
            p1 = s.prefix[1];
        }
        s_mode[threadIdx.x] = mode;
        s_pre[threadIdx.x][0] = p0;
        s_pre[threadIdx.x][1] = p1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long step = (long long) gridDim.x * 256;
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        const int gi = (int) grp[i] - g0;
        int bin = -1;
        if (gi >= 0 && gi < ng) {
            const u64 k = keys[i];
            const int mode = s_mode[gi];
            const int digit = (int) ((k >> shift) & (u64) (kGsBins - 1));
            const u64 top = k & mask;
            if (mode != 0 && top == s_pre[gi][0]) bin = (gi * 2) * kGsBins + digit;
            else if (mode == 2 && top == s_pre[gi][1]) bin = (gi * 2 + 1) * kGsBins + digit;
        }
        const u64 act = __ballot(bin >= 0);
        if (act) {  // (wave-uniform)
            const int leader = __ffsll((long long) act) - 1;
            const int lb = readlane_i(bin, leader);
            if (__ballot(bin == lb) == act) {
                if (lane == leader) atomicAdd(&s_h[lb], (unsigned int) __popcll(act));
            } else if (bin >= 0) {
                atomicAdd(&s_h[bin], 1u);
            }
        }
    }
    __syncthreads();
    unsigned int *hist = b->hist + (size_t) g0 * 2 * kGsBins;
    for (int t = threadIdx.x; t < ng * 2 * kGsBins; t += 256) {
        const unsigned int c = s_h[t];
        if (c) atomicAdd(&hist[t], c);
    }
}

// one block; thread g narrows group g, then the whole block clears the histograms for the next pass
__global__ void __launch_bounds__(256) k_gs_narrow(GsBlock *__restrict__ b, int n_groups, int shift) {
    const int g = threadIdx.x;
    if (g < n_groups) {
        GsState s = b->st[g];
        if (s.live) {
            int dig[2];
#pragma unroll
            for (int slot = 0; slot < 2; ++slot) {
                const unsigned int *h = b->hist + ((size_t) g * 2 + (slot == 1 && !s.same ? 1 : 0)) * kGsBins;
                long long r = s.rank[slot];
                int d = 0;
                for (; d < kGsBins - 1; ++d) {  // (the rank is below the population that carries the prefix: the walk ends inside)
                    const long long c = (long long) h[d];
                    if (r < c) break;
                    r -= c;
                }
                dig[slot] = d;
                s.rank[slot] = r;
                s.prefix[slot] |= (u64) d << shift;
            }
            s.same = (s.same && dig[0] == dig[1]) ? 1 : 0;
            b->st[g] = s;
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < n_groups * 2 * kGsBins; t += 256) b->hist[t] = 0u;
}

__global__ void __launch_bounds__(64) k_gs_out(GsBlock *__restrict__ b, int n_groups) {
    const int g = threadIdx.x;
    if (g >= n_groups) return;
    me_group_stats o;
    o.count = 0;
    o.sum = o.min = o.max = o.lower = o.upper = 0.0;
    if (b->st[g].live) {
        o.count = (long long) b->cnt[g];
        o.sum = b->tot[g];
        o.min = __longlong_as_double((long long) b->mn[g]);
        o.max = __longlong_as_double((long long) b->mx[g]);
        o.lower = __longlong_as_double((long long) b->st[g].prefix[0]);
        o.upper = __longlong_as_double((long long) b->st[g].prefix[1]);
    }
    b->out[g] = o;
}

// 2 bits per plane: the axis of the plane's direction, 3 = none; planes 0 .. 31 in lo, 32 .. 63 in hi
__global__ void __launch_bounds__(256)
k_mom_gather(const SPoint *__restrict__ sp, long long n, const int *__restrict__ labels, const double *__restrict__ eig_s,
             const unsigned char *__restrict__ valid_s, u64 lo, u64 hi, u64 *__restrict__ keys, signed char *__restrict__ grp,
             signed char *__restrict__ axis_o) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long o = sp[i].idx;
    const int lab = labels[o];
    int a = -1;
    if (lab >= 0 && lab < 64) {
        const int code = (int) (((lab < 32 ? lo : hi) >> (2 * (lab & 31))) & 3ull);
        if (code != 3 && valid_s[i]) a = code;
    }
    keys[i] = (u64) __double_as_longlong(eig_s[3 * i + 2] + 0.0);
    grp[i] = (signed char) a;
    axis_o[o] = (signed char) a;
}

int ensure_gs(me_ctx *ctx, long long n, int n_groups, unsigned int *nb_out) {
    const unsigned int nb = blocks_of(n, kGsTile);
    ME_CHECK(ctx, ctx->mom_tmp[0].ensure((size_t) std::max<long long>(n, 1) * 8));
    ME_CHECK(ctx, ctx->mom_tmp[1].ensure((size_t) std::max<long long>(n, 1)));
    ME_CHECK(ctx, ctx->mom_tmp[2].ensure(sizeof(GsBlock)));
    ME_CHECK(ctx, ctx->red.ensure(row_sum_bytes(n_groups, nb)));
    *nb_out = nb;
    return ME_OK;
}

// The (key, group byte) pairs are in mom_tmp[0] / mom_tmp[1]; the result is left in the state block's `out` (device), queued on the
// context's stream.  1 <= n_groups <= 64, every group byte in [-1, n_groups).
int group_stats_device(me_ctx *ctx, long long n, int n_groups, unsigned int nb) {
    const u64 *keys = ctx->mom_tmp[0].as<u64>();
    const signed char *grp = ctx->mom_tmp[1].as<signed char>();
    GsBlock *blk = ctx->mom_tmp[2].as<GsBlock>();
    TimerScope ts(ctx, "group_select");
    hipLaunchKernelGGL(k_gs_init, dim3(1), dim3(256), 0, ctx->stream, blk);
    hipLaunchKernelGGL(k_gs_stat, dim3(nb), dim3(256), 0, ctx->stream, keys, grp, n, n_groups, blk, row_sum_part(ctx), nb);
    row_sum_device<0ull>(ctx, n_groups, nb, reinterpret_cast<RedWord *>(blk->tot));
    hipLaunchKernelGGL(k_gs_start, dim3(1), dim3(64), 0, ctx->stream, blk, n_groups);
    const unsigned int gx = std::min(blocks_of(n), kGsMaxBlocks);
    for (int pass = 0; pass < kGsPasses; ++pass) {
        const int shift = 64 - kGsBits * (pass + 1);
        const u64 mask = pass == 0 ? 0ull : ~0ull << (shift + kGsBits);
        for (int g0 = 0; g0 < n_groups; g0 += kGsSlice)
            hipLaunchKernelGGL(k_gs_hist, dim3(gx), dim3(256), 0, ctx->stream, keys, grp, n, g0, std::min(kGsSlice, n_groups - g0), mask, shift,
                               blk);
        hipLaunchKernelGGL(k_gs_narrow, dim3(1), dim3(256), 0, ctx->stream, blk, n_groups, shift);
    }
    hipLaunchKernelGGL(k_gs_out, dim3(1), dim3(64), 0, ctx->stream, blk, n_groups);
    ts.end();
    ME_CHECK(ctx, hipGetLastError());
    return ME_OK;
}

inline double dot_host(const double *u, const double *v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

int check_mom_params(const me_mom_params *p) {
    if (!p) return ME_ERR_ARG;
    if (!(p->cos_orthogonal >= 0.0) || !(p->cos_orthogonal < p->cos_parallel) || !(p->cos_parallel <= 1.0)) return ME_ERR_ARG;
    if (p->min_axis_points < 1) return ME_ERR_ARG;
    return ME_OK;
}

}  // namespace

int group_order_stats(me_ctx *ctx, const double *values_host, const int32_t *group_host, long long n, int n_groups, me_group_stats *out) {
    if (n_groups < 1 || n_groups > kGsMaxGroups) return ctx->fail(ME_ERR_ARG, "me_group_order_stats: n_groups must be in [1, 64]");
    if (n < 0) return ctx->fail(ME_ERR_ARG, "me_group_order_stats: n must be >= 0");
    if (!out || (n > 0 && (!values_host || !group_host))) return ctx->fail(ME_ERR_ARG, "me_group_order_stats: NULL argument");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    unsigned int nb = 0;
    ME_TRY(ensure_gs(ctx, n, n_groups, &nb));
    DevBuf &dv = ctx->tmp[2], &dg = ctx->tmp[3];
    ME_CHECK(ctx, dv.ensure((size_t) n * 8));
    ME_CHECK(ctx, dg.ensure((size_t) n * 4));
    ME_TRY(copy_h2d(ctx, dv.p, values_host, (size_t) n * 8));
    ME_TRY(copy_h2d(ctx, dg.p, group_host, (size_t) n * 4));
    GsBlock *blk = ctx->mom_tmp[2].as<GsBlock>();
    ME_CHECK(ctx, hipMemsetAsync(&blk->err, 0, 8, ctx->stream));
    {
        TimerScope ts(ctx, "group_select");
        hipLaunchKernelGGL(k_gs_prep, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, dv.as<double>(), dg.as<int>(), n, n_groups,
                           ctx->mom_tmp[0].as<u64>(), ctx->mom_tmp[1].as<signed char>(), &blk->err);
    }
    ME_TRY(group_stats_device(ctx, n, n_groups, nb));
    unsigned int h_err[2] = {0, 0};
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, out, blk->out, sizeof(me_group_stats) * (size_t) n_groups));
        ME_TRY(mail_post(ctx, h_err, &blk->err, 8));
        ME_TRY(mg.sync());
    }
    if (h_err[0])
        return ctx->fail(ME_ERR_ARG, "me_group_order_stats: a group id outside [-1, n_groups), or a value that is negative or not finite");
    return ME_OK;
}

int mom_select_axes(const me_plane_record *planes, int n_planes, const me_mom_params *p, int32_t *dir_of_plane, me_mom_axes *axes) {
    if (check_mom_params(p) != ME_OK || !axes || n_planes < 0 || n_planes > 64) return ME_ERR_ARG;
    if (n_planes > 0 && (!planes || !dir_of_plane)) return ME_ERR_ARG;
    std::memset(axes, 0, sizeof(*axes));
    int nd = 0, founder[64], members[64];
    long long W[64];
    for (int r = 0; r < n_planes; ++r) {
        int g = 0;
        for (; g < nd; ++g)
            if (std::fabs(dot_host(planes[r].plane, planes[founder[g]].plane)) >= p->cos_parallel) break;
        if (g == nd) {
            founder[nd] = r;
            members[nd] = 0;
            W[nd] = 0;
            ++nd;
        }
        dir_of_plane[r] = g;
        members[g] += 1;
        W[g] += planes[r].count;
    }
    axes->n_directions = nd;
    auto eligible = [&](int g) { return W[g] >= p->min_axis_points; };
    auto orth = [&](int g, int h) { return std::fabs(dot_host(planes[founder[g]].plane, planes[founder[h]].plane)) <= p->cos_orthogonal; };
    int best[3] = {-1, -1, -1}, s_best = 0;
    long long best_min = -1, best_sum = -1;
    // ascending tuples in lexicographic order: only a strictly better (min W, sum W) replaces the one found first
    for (int s = 3; s >= 1 && s_best == 0; --s) {
        for (int a = 0; a < nd; ++a) {
            if (!eligible(a)) continue;
            if (s == 1) {
                if (W[a] > best_min) best_min = best_sum = W[a], best[0] = a, s_best = 1;
                continue;
            }
            for (int b = a + 1; b < nd; ++b) {
                if (!eligible(b) || !orth(a, b)) continue;
                if (s == 2) {
                    const long long mn = std::min(W[a], W[b]), sm = W[a] + W[b];
                    if (mn > best_min || (mn == best_min && sm > best_sum)) best_min = mn, best_sum = sm, best[0] = a, best[1] = b, s_best = 2;
                    continue;
                }
                for (int c = b + 1; c < nd; ++c) {
                    if (!eligible(c) || !orth(a, c) || !orth(b, c)) continue;
                    const long long mn = std::min(W[a], std::min(W[b], W[c])), sm = W[a] + W[b] + W[c];
                    if (mn > best_min || (mn == best_min && sm > best_sum))
                        best_min = mn, best_sum = sm, best[0] = a, best[1] = b, best[2] = c, s_best = 3;
                }
            }
        }
    }
    axes->n_axes = s_best;
    for (int k = 0; k < s_best; ++k) {
        me_mom_axis_choice &ax = axes->axis[k];
        ax.direction = best[k];
        ax.n_planes = members[best[k]];
        ax.weight = W[best[k]];
        for (int e = 0; e < 3; ++e) ax.rep[e] = planes[founder[best[k]]].plane[e];
    }
    return ME_OK;
}

int mom(me_ctx *ctx, int slot, const me_mom_params *p, me_mom_out *out) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_mom"));
    if (check_mom_params(p) != ME_OK)
        return ctx->fail(ME_ERR_ARG, "me_mom: needs 0 <= cos_orthogonal < cos_parallel <= 1 and min_axis_points >= 1");
    Cloud &c = ctx->cloud[slot];
    if (!c.lg_have || !c.index_valid)
        return ctx->fail(ME_ERR_STATE, "me_mom: the slot has no current eigenvalues (run me_local_geometry; a changed cloud or a new index discards them)");
    if (!c.plane_valid) return ctx->fail(ME_ERR_STATE, "me_mom: the slot has no plane labels (me_segment_planes)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = c.n;
    const int np = (int) c.plane_rec.size();
    int32_t dir_of_plane[64];
    me_mom_axes axes;
    if (mom_select_axes(c.plane_rec.data(), np, p, dir_of_plane, &axes) != ME_OK) return ctx->fail(ME_ERR_ARG, "me_mom: bad plane records");
    u64 tab[2] = {~0ull, ~0ull};
    for (int r = 0; r < np; ++r)
        for (int k = 0; k < axes.n_axes; ++k)
            if (dir_of_plane[r] == axes.axis[k].direction) tab[r >> 5] = (tab[r >> 5] & ~(3ull << (2 * (r & 31)))) | ((u64) k << (2 * (r & 31)));
    c.mom_have = false;
    ME_CHECK(ctx, c.mom_axis.ensure((size_t) n));
    const int n_groups = std::max(1, (int) axes.n_axes);
    unsigned int nb = 0;
    ME_TRY(ensure_gs(ctx, n, n_groups, &nb));
    {
        TimerScope ts(ctx, "mom");
        hipLaunchKernelGGL(k_mom_gather, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, c.sp.as<SPoint>(), n, c.plane_labels.as<int>(),
                           c.lg_eig.as<double>(), c.lg_val.as<unsigned char>(), tab[0], tab[1], ctx->mom_tmp[0].as<u64>(),
                           ctx->mom_tmp[1].as<signed char>(), c.mom_axis.as<signed char>());
    }
    ME_CHECK(ctx, hipGetLastError());
    me_group_stats gs[3];
    std::memset(gs, 0, sizeof(gs));
    if (axes.n_axes > 0) {
        ME_TRY(group_stats_device(ctx, n, n_groups, nb));
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, gs, ctx->mom_tmp[2].as<GsBlock>()->out, sizeof(me_group_stats) * (size_t) n_groups));
        ME_TRY(mg.sync());
    } else {
        ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    c.mom_have = true;
    c.mom_lg_serial = c.lg_serial;
    c.mom_plane_serial = c.plane_serial;
    if (out) {
        std::memset(out, 0, sizeof(*out));
        out->n_axes = axes.n_axes;
        out->n_directions = axes.n_directions;
        double med = 0.0, mean = 0.0;
        for (int k = 0; k < axes.n_axes; ++k) {
            me_mom_axis &a = out->axis[k];
            a.direction = axes.axis[k].direction;
            a.n_planes = axes.axis[k].n_planes;
            for (int e = 0; e < 3; ++e) a.rep[e] = axes.axis[k].rep[e];
            a.n_points = axes.axis[k].weight;
            a.n_valid = gs[k].count;
            a.sum_l3 = gs[k].sum;
            a.min = gs[k].min;
            a.max = gs[k].max;
            a.lower = gs[k].lower;
            a.upper = gs[k].upper;
            a.median = (gs[k].lower + gs[k].upper) / 2;
            med += a.median;
            if (a.n_valid > 0) mean += a.sum_l3 / (double) a.n_valid;
        }
        out->mom_median = med;
        out->mom_mean = mean;
    }
    return ME_OK;
}

int mom_fetch(me_ctx *ctx, int slot, int8_t *axis_host) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_mom_fetch"));
    Cloud &c = ctx->cloud[slot];
    if (!c.mom_have || !c.lg_have || !c.index_valid || !c.plane_valid || c.mom_lg_serial != c.lg_serial || c.mom_plane_serial != c.plane_serial)
        return ctx->fail(ME_ERR_STATE, "me_mom_fetch: no current me_mom result for this slot (it is dropped with the plane labels and the eigenvalues)");
    if (!axis_host) return ME_OK;
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    ME_TRY(copy_d2h(ctx, axis_host, c.mom_axis.p, (size_t) c.n));
    return ME_OK;
}

}  // namespace me
