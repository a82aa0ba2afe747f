// me_search.hip — the neighbour LISTS themselves, between the two resident clouds in either direction or inside one: Open3D's
// KDTreeFlann::SearchKNN / SearchHybrid / SearchRadius (map_eval.cpp:1213-1218, 1448-1454, 1670) for every point of a query slot in
// a reference slot.  The definition is in include/mapeval_hip.h, DESIGN.md section 4.16.
//   k_knn_cross     k-NN and hybrid in one body.  One lane per SORTED query point (neighbouring lanes walk neighbouring paths), the
//                   stackless nearest-first walk of the REFERENCE cloud's octree (oct_walk_nearest); the k best so far in LDS, element j
//                   of lane t at [j * blockDim + t] (k_knn_normals' conflict-free layout), sorted ascending by (d2, original index).
//                   A box is admitted with lb <= worst: worst = the k-th best once the list is full (<=: a tie may hold a smaller
//                   index), until then +inf (k-NN) or r^2 (hybrid, whose candidates also need d < r^2).        ("knn_search")
//   k_radius_walk   <false> counts, <true> fills: the same walk with admit(lb) = lb < r^2 and membership d < r^2 (strict).  The count
//                   pass writes one int per query in CLOUD order; an exclusive scan (me_prims.hip) gives the int64 row offsets; the
//                   fill pass walks again and writes (d2, idx) at offsets[q] + running position, in walk order.
//                                                                                                    ("radius_count", "radius_fill")
//   k_row_sort_tile one wave per row of at most kSearchSortTile entries: the row's 96-bit keys (bits of d2, idx) — d2 >= +0.0, so the
//                   bit pattern orders as an unsigned integer, and a reference point occurs once per row, so the keys are unique —
//                   through a bitonic network in LDS.
//   k_row_sort_long one block per longer row, the same network on the row in global memory.             (both "radius_sort")
// The network is the all-ascending form of the bitonic sort (per block size s a "flip" step that pairs i with i ^ (s - 1), then "disperse" steps
// i ^ s/4 ... i ^ 1): every compare-exchange puts the smaller key at the smaller position, so the +inf padding of a row whose length is no power
// of two would never move and is not stored — a pair whose upper position lies beyond the row is skipped.
// The searches run on the octree, which every index carries: no slot is re-indexed for a radius, and nothing resident is touched.
// The file is compiled with -ffp-contract=off: tests/_search_ref.py restates the distance and the order.
#include <cmath>
#include <cstring>

#include "me_internal.hpp"
#include "me_oct_walk.hpp"

namespace me {

namespace {

typedef unsigned long long u64;

constexpr int kSearchBlock = 128;  // k_knn_cross: k = 40 x 128 lanes x 12 B = 60 KB of LDS (me_reg.hip's figure)
static_assert(kKnnMax * kSearchBlock * 12 + kMaxLevels * 8 <= 64 * 1024, "the k-best lists and the level offsets fit one workgroup's LDS");
constexpr int kSortWaves = 4;      // rows per block of k_row_sort_tile
static_assert(kSearchSortTile * 12 * kSortWaves <= 64 * 1024, "the row tiles of one block fit its LDS");
constexpr unsigned int kLongBlocks = 1024;  // k_row_sort_long: a fixed grid strides over the rows

// mask: uint8[nq] in the query's CLOUD order or nullptr.  idx / d2: [nq][k] in cloud order, -1 / +inf past the entries found;
// counts (nullable): [nq] entries used.  r2 = +inf: plain k-NN.
__global__ void __launch_bounds__(kSearchBlock)
k_knn_cross(const SPoint *__restrict__ qsp, long long nq, const SPoint *__restrict__ rsp, OctView oct, int k, double r2,
            const unsigned char *__restrict__ mask, int *__restrict__ idx, double *__restrict__ d2, int *__restrict__ counts) {
    extern __shared__ double s_dyn[];
    double *s_d = s_dyn;                                            // [k][kSearchBlock]
    int *s_i = reinterpret_cast<int *>(s_dyn + k * kSearchBlock);  // [k][kSearchBlock]
    __shared__ long long s_off[kMaxLevels];
    if (threadIdx.x < kMaxLevels) s_off[threadIdx.x] = oct.off[threadIdx.x];
    __syncthreads();
    const int tid = threadIdx.x;
    const long long i = (long long) blockIdx.x * kSearchBlock + tid;
    if (i >= nq) return;
    const SPoint q = qsp[i];
    const long long qi = q.idx;  // a permutation of [0, nq)
    int cnt = 0;
    if (!mask || mask[qi]) {
        const ONode *__restrict__ nodes = oct.nodes;
        const double qx = q.x, qy = q.y, qz = q.z;
        double worst = r2;
        auto consider = [&](double d, int pi) {
            if (!(d < r2)) return;  // (hybrid: strict; k-NN: every finite distance)
            if (cnt == k) {
                if (!(d < worst || (d == worst && pi < s_i[(k - 1) * kSearchBlock + tid]))) return;
            }
            int pos = cnt < k ? cnt : k - 1;
            while (pos > 0) {
                const double pd = s_d[(pos - 1) * kSearchBlock + tid];
                const int pidx = s_i[(pos - 1) * kSearchBlock + tid];
                if (d < pd || (d == pd && pi < pidx)) {
                    s_d[pos * kSearchBlock + tid] = pd;
                    s_i[pos * kSearchBlock + tid] = pidx;
                    --pos;
                } else {
                    break;
                }
            }
            s_d[pos * kSearchBlock + tid] = d;
            s_i[pos * kSearchBlock + tid] = pi;
            if (cnt < k) ++cnt;
            if (cnt == k) worst = s_d[(k - 1) * kSearchBlock + tid];
        };
        oct_walk_nearest(
            nodes, s_off, oct.n_levels - 1, qx, qy, qz, [&](double lb) { return lb <= worst; },
            [&](long long leaf) {
                const long long jb = nodes[leaf].begin, je = nodes[leaf + 1].begin;
                for (long long j = jb; j < je; ++j) {
                    const SPoint p = rsp[j];
                    consider(dist2_exact(qx, qy, qz, p.x, p.y, p.z), (int) p.idx);
                }
            });
    }
    for (int j = 0; j < k; ++j) {
        idx[qi * k + j] = j < cnt ? s_i[j * kSearchBlock + tid] : -1;
        d2[qi * k + j] = j < cnt ? s_d[j * kSearchBlock + tid] : INFINITY;
    }
    if (counts) counts[qi] = cnt;
}

// FILL = false: cnt[q] = the row length (cloud order; 0 for a masked-out query).  FILL = true: the row's entries at off[q] .. in
// walk order (off = the exclusive scan of cnt; the walk is the same, so a row receives exactly cnt[q] entries).
template <bool FILL>
__global__ void __launch_bounds__(256)
k_radius_walk(const SPoint *__restrict__ qsp, long long nq, const SPoint *__restrict__ rsp, OctView oct, double r2,
              const unsigned char *__restrict__ mask, int *__restrict__ cnt, const long long *__restrict__ off,
              unsigned int *__restrict__ idx, u64 *__restrict__ d2b) {
    __shared__ long long s_off[kMaxLevels];
    if (threadIdx.x < kMaxLevels) s_off[threadIdx.x] = oct.off[threadIdx.x];
    __syncthreads();
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const SPoint q = qsp[i];
    const long long qi = q.idx;
    int c = 0;
    if (!mask || mask[qi]) {
        const ONode *__restrict__ nodes = oct.nodes;
        const double qx = q.x, qy = q.y, qz = q.z;
        long long w = 0;
        if (FILL) w = off[qi];
        oct_walk_nearest(
            nodes, s_off, oct.n_levels - 1, qx, qy, qz, [&](double lb) { return lb < r2; },
            [&](long long leaf) {
                const long long jb = nodes[leaf].begin, je = nodes[leaf + 1].begin;
                for (long long j = jb; j < je; ++j) {
                    const SPoint p = rsp[j];
                    const double d = dist2_exact(qx, qy, qz, p.x, p.y, p.z);
                    if (d < r2) {
                        if (FILL) {
                            idx[w + c] = (unsigned int) p.idx;
                            d2b[w + c] = (u64) __double_as_longlong(d);  // (d >= +0.0: the bit pattern is the sort key)
                        }
                        ++c;
                    }
                }
            });
    }
    if (!FILL) cnt[qi] = c;
}

__device__ __forceinline__ bool key_less(u64 ad, unsigned int ai, u64 bd, unsigned int bi) { return ad < bd || (ad == bd && ai < bi); }

// One step of the network for position pairs (i, l), l = i ^ x > i, over a row of `len` entries: thread t of T takes the pairs
// whose lower position is i = t, t + T, ...  SYNC() separates the steps.
template <class SYNC>
__device__ __forceinline__ void row_sort_network(u64 *kd, unsigned int *ki, int len, int t, int T, SYNC &&sync) {
    int m = 1;
    while (m < len) m <<= 1;
    for (int s = 2; s <= m; s <<= 1) {
        for (int j = s; j > 0;) {
            const int x = j == s ? s - 1 : j;  // the flip step (mask s - 1) first, then the disperse steps (masks s/4 ... 1)
            for (int i = t; i < len; i += T) {
                const int l = i ^ x;
                if (l > i && l < len) {
                    const u64 ad = kd[i], bd = kd[l];
                    const unsigned int ai = ki[i], bi = ki[l];
                    if (key_less(bd, bi, ad, ai)) {
                        kd[i] = bd;
                        ki[i] = bi;
                        kd[l] = ad;
                        ki[l] = ai;
                    }
                }
            }
            sync();
            j = j == s ? s >> 2 : j >> 1;
        }
    }
}

// rows of 2 .. kSearchSortTile entries: wave w of a block takes row blockIdx.x * kSortWaves + w
__global__ void __launch_bounds__(64 * kSortWaves)
k_row_sort_tile(const long long *__restrict__ off, long long nq, unsigned int *idx, u64 *d2b) {
    __shared__ u64 s_d[kSortWaves][kSearchSortTile];
    __shared__ unsigned int s_i[kSortWaves][kSearchSortTile];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const long long row = (long long) blockIdx.x * kSortWaves + w;
    if (row >= nq) return;
    const long long b = off[row];
    const long long len64 = off[row + 1] - b;
    if (len64 < 2 || len64 > kSearchSortTile) return;
    const int len = __builtin_amdgcn_readfirstlane((int) len64);
    u64 *kd = s_d[w];
    unsigned int *ki = s_i[w];
    for (int i = lane; i < len; i += 64) {
        kd[i] = d2b[b + i];
        ki[i] = idx[b + i];
    }
    auto sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    sync();
    row_sort_network(kd, ki, len, lane, 64, sync);
    for (int i = lane; i < len; i += 64) {
        d2b[b + i] = kd[i];
        idx[b + i] = ki[i];
    }
}

// rows longer than the tile, in place in global memory: block b takes the rows b, b + gridDim.x, ...  (every thread of a block
// reads the same two offsets, so the test is block-uniform and the barriers inside the network are reached by all or none)
__global__ void __launch_bounds__(256) k_row_sort_long(const long long *__restrict__ off, long long nq, unsigned int *idx, u64 *d2b) {
    for (long long row = blockIdx.x; row < nq; row += gridDim.x) {
        const long long b = off[row];
        const long long len = off[row + 1] - b;
        if (len <= kSearchSortTile) continue;
        // (a row holds at most one entry per reference point: fewer than 2^31)
        row_sort_network(d2b + b, idx + b, (int) len, (int) threadIdx.x, 256, [] { __syncthreads(); });
    }
}

struct SearchPair {
    Cloud *q, *r;
};

// the checks common to the three searches; an index that is missing (the points were replaced on the device) is built at the cell
// size asked for at the upload, and the reference cloud's octree is finished
int search_prepare(me_ctx *ctx, int qslot, int rslot, const char *who, SearchPair &sp) {
    ME_TRY(need_single_gpu_cloud(ctx, qslot, who));
    ME_TRY(need_single_gpu_cloud(ctx, rslot, who));
    sp.q = &ctx->cloud[qslot];
    sp.r = &ctx->cloud[rslot];
    if (sp.q->n <= 0 || sp.r->n <= 0) return ctx->fail(ME_ERR_ARG, std::string(who) + ": empty cloud");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    for (int s : {qslot, rslot}) {
        Cloud &c = ctx->cloud[s];
        if (!c.index_valid) ME_TRY(cloud_build_index(ctx, s, c.cell_size_req));
    }
    ME_TRY(cloud_finish_octree(ctx, rslot));
    return ME_OK;
}

int upload_mask(me_ctx *ctx, const uint8_t *mask_host, long long n, DevBuf &buf, const unsigned char *&mask) {
    mask = nullptr;
    if (!mask_host) return ME_OK;
    ME_CHECK(ctx, buf.ensure((size_t) n));
    ME_TRY(copy_h2d(ctx, buf.p, mask_host, (size_t) n));
    mask = buf.as<unsigned char>();
    return ME_OK;
}

int knn_or_hybrid(me_ctx *ctx, int qslot, int rslot, const char *who, int k, double r2, const uint8_t *mask_host, int32_t *counts_host,
                  int32_t *idx_host, double *d2_host) {
    SearchPair sp;
    ME_TRY(search_prepare(ctx, qslot, rslot, who, sp));
    const Cloud &q = *sp.q, &r = *sp.r;
    const long long n = q.n;
    DevBuf b_mask, b_idx, b_d2, b_cnt;  // released on return (estimate_normals' rule for its list buffers)
    const unsigned char *mask;
    ME_TRY(upload_mask(ctx, mask_host, n, b_mask, mask));
    ME_CHECK(ctx, b_idx.ensure((size_t) n * k * 4));
    ME_CHECK(ctx, b_d2.ensure((size_t) n * k * 8));
    if (counts_host) ME_CHECK(ctx, b_cnt.ensure((size_t) n * 4));
    {
        TimerScope ts(ctx, "knn_search");
        hipLaunchKernelGGL(k_knn_cross, dim3(blocks_of(n, kSearchBlock)), dim3(kSearchBlock), (size_t) k * kSearchBlock * 12, ctx->stream,
                           q.sp.as<SPoint>(), n, r.sp.as<SPoint>(), r.oct, k, r2, mask, b_idx.as<int>(), b_d2.as<double>(),
                           counts_host ? b_cnt.as<int>() : nullptr);
    }
    ME_CHECK(ctx, hipGetLastError());
    ME_TRY(copy_d2h(ctx, idx_host, b_idx.p, (size_t) n * k * 4));
    ME_TRY(copy_d2h(ctx, d2_host, b_d2.p, (size_t) n * k * 8));
    if (counts_host) ME_TRY(copy_d2h(ctx, counts_host, b_cnt.p, (size_t) n * 4));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

}  // namespace

int knn_search(me_ctx *ctx, int qslot, int rslot, int k, const uint8_t *mask, int32_t *idx, double *d2) {
    if (k < 1 || k > kKnnMax) return ctx->fail(ME_ERR_ARG, "me_knn_search: k must be in [1, 40]");
    if (!idx || !d2) return ctx->fail(ME_ERR_ARG, "me_knn_search: idx and d2 must not be NULL");
    return knn_or_hybrid(ctx, qslot, rslot, "me_knn_search", k, (double) INFINITY, mask, nullptr, idx, d2);
}

int hybrid_search(me_ctx *ctx, int qslot, int rslot, double radius, int max_nn, const uint8_t *mask, int32_t *counts, int32_t *idx,
                  double *d2) {
    if (max_nn < 1 || max_nn > kKnnMax) return ctx->fail(ME_ERR_ARG, "me_hybrid_search: max_nn must be in [1, 40]");
    if (!(radius > 0) || !std::isfinite(radius)) return ctx->fail(ME_ERR_ARG, "me_hybrid_search: radius must be finite and > 0");
    if (!idx || !d2) return ctx->fail(ME_ERR_ARG, "me_hybrid_search: idx and d2 must not be NULL");
    return knn_or_hybrid(ctx, qslot, rslot, "me_hybrid_search", max_nn, radius * radius, mask, counts, idx, d2);
}

int radius_search(me_ctx *ctx, int qslot, int rslot, double radius, const uint8_t *mask_host, int64_t *offsets_host, int32_t *idx_host,
                  double *d2_host, long long capacity, int64_t *total_host) {
    if (!(radius > 0) || !std::isfinite(radius)) return ctx->fail(ME_ERR_ARG, "me_radius_search: radius must be finite and > 0");
    if ((idx_host == nullptr) != (d2_host == nullptr)) return ctx->fail(ME_ERR_ARG, "me_radius_search: idx and d2 go together");
    if (!idx_host && !offsets_host && !total_host) return ctx->fail(ME_ERR_ARG, "me_radius_search: no output asked for");
    SearchPair sp;
    ME_TRY(search_prepare(ctx, qslot, rslot, "me_radius_search", sp));
    const Cloud &q = *sp.q, &r = *sp.r;
    const long long n = q.n;
    const double r2 = radius * radius;  // formed once, in fp64
    DevBuf b_mask, b_cnt, b_off, b_idx, b_d2;  // released on return; b_d2 holds the distances as bit patterns, which is what the host gets
    const unsigned char *mask;
    ME_TRY(upload_mask(ctx, mask_host, n, b_mask, mask));
    ME_CHECK(ctx, b_cnt.ensure((size_t) (n + 1) * 4));
    ME_CHECK(ctx, b_off.ensure((size_t) (n + 1) * 8));
    int *cnt = b_cnt.as<int>();
    long long *off = b_off.as<long long>();
    ME_CHECK(ctx, hipMemsetAsync(cnt + n, 0, 4, ctx->stream));  // the scan of n + 1 entries ends with the total
    {
        TimerScope ts(ctx, "radius_count");
        hipLaunchKernelGGL(k_radius_walk<false>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, r.sp.as<SPoint>(), r.oct,
                           r2, mask, cnt, (const long long *) nullptr, (unsigned int *) nullptr, (u64 *) nullptr);
    }
    ME_CHECK(ctx, hipGetLastError());
    ME_TRY(exclusive_scan_i32_i64(ctx, cnt, off, n + 1));
    long long total = 0;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &total, off + n, 8));
        ME_TRY(mg.sync());
    }
    if (idx_host) {
        if (capacity < total)
            return ctx->fail(ME_ERR_ARG, "me_radius_search: capacity " + std::to_string(capacity) + " is below the needed total " +
                                             std::to_string(total) + " (nothing written)");
        if (total > 0) {
            ME_CHECK(ctx, b_idx.ensure((size_t) total * 4));
            ME_CHECK(ctx, b_d2.ensure((size_t) total * 8));
            {
                TimerScope ts(ctx, "radius_fill");
                hipLaunchKernelGGL(k_radius_walk<true>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, r.sp.as<SPoint>(),
                                   r.oct, r2, mask, (int *) nullptr, (const long long *) off, b_idx.as<unsigned int>(), b_d2.as<u64>());
            }
            {
                TimerScope ts(ctx, "radius_sort");
                hipLaunchKernelGGL(k_row_sort_tile, dim3(blocks_of(n, kSortWaves)), dim3(64 * kSortWaves), 0, ctx->stream,
                                   (const long long *) off, n, b_idx.as<unsigned int>(), b_d2.as<u64>());
                hipLaunchKernelGGL(k_row_sort_long, dim3((unsigned int) std::min<long long>(kLongBlocks, n)), dim3(256), 0, ctx->stream,
                                   (const long long *) off, n, b_idx.as<unsigned int>(), b_d2.as<u64>());
            }
            ME_CHECK(ctx, hipGetLastError());
            ME_TRY(copy_d2h(ctx, idx_host, b_idx.p, (size_t) total * 4));
            ME_TRY(copy_d2h(ctx, d2_host, b_d2.p, (size_t) total * 8));
        }
    }
    if (offsets_host) ME_TRY(copy_d2h(ctx, offsets_host, off, (size_t) (n + 1) * 8));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (total_host) *total_host = total;
    return ME_OK;
}

}  // namespace me
