// me_cluster.hip — Open3D's PointCloud::ClusterDBSCAN on a resident cloud, and the cluster-size filter on top.  DESIGN.md section 4.9.
//   k_cluster_count   per point: the points with d2 < eps^2 in the 27-cell stencil of the radius grid (k_radius_count's stream); a core
//                     point (count >= min_points) starts as its own root, parent[i] = i, every other point gets parent[i] = -1
//   k_cluster_union   ONE more stream in which only core lanes work and only core candidates at a smaller sorted position count: a
//                     concurrent union-find over parent[] (the larger root is hooked under the smaller with atomicCAS, path halving with
//                     atomicMin).  parent[] of the candidates is staged in LDS next to x, y, z: a candidate whose staged parent is the
//                     lane's current root costs one LDS read and a compare, global atomics happen only where two sets meet
//   k_cluster_flatten every core point jumps to its root; the root's slot takes the smallest cloud index below it (integer atomicMin)
//   k_cluster_root_keys / k_cluster_root_rank   the roots, compacted and sorted by that smallest index: their ranks are the cluster ids
//   k_cluster_core_labels   labels of the core points (parent[] becomes the label per sorted position, -1 for the rest), sizes
//   k_cluster_border  the non-core points with count >= 2, compacted: the smallest label among their core neighbours, sizes
//   k_cluster_rank_ok / k_cluster_size_ok / k_cluster_keep_mask   me_cluster_keep: the slot's outlier keep-mask from labels and sizes
// Everything is integer arithmetic on the same d2 = ((dx*dx + dy*dy) + dz*dz) (file compiled with -ffp-contract=off): labels, counts and
// sizes do not depend on the order in which the atomics arrive.  tests/_cluster_ref.py restates the contract.                ("cluster")
#include <algorithm>
#include <cmath>
#include <vector>

#include "me_internal.hpp"
#include "me_wave_stream.hpp"

namespace me {

namespace {

// parent[] is read while other workgroups change it.  A value read late is still a member of the same set with a smaller position (a
// pointer only ever moves towards the root), so no load needs to be ordered with anything; the agent-scope load only keeps it from
// being served by this CU's L1 for the rest of the kernel.
__device__ __forceinline__ int uf_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(int *__restrict__ parent, int x) {
    for (;;) {  // (positions strictly decrease along a path: the loop ends)
        const int p = uf_load(parent + x);
        if (p == x) return x;
        const int gp = uf_load(parent + p);
        if (gp == p) return p;
        atomicMin(parent + x, gp);  // path halving; min: a pointer never moves away from the root
        x = gp;
    }
}
// a and b: members of the two sets.  Returns the root of the united set as this thread saw it last.
__device__ __forceinline__ int uf_unite(int *__restrict__ parent, int a, int b) {
    int ra = uf_find(parent, a), rb = uf_find(parent, b);
    while (ra != rb) {
        const int hi = max(ra, rb), lo = min(ra, rb);
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        ra = uf_find(parent, old);  // hi had been hooked by somebody else: go on from where it points (max(ra, rb) has decreased)
        rb = lo;
    }
    return ra;
}

// dst[key] = min(dst[key], v) or dst[key] += v for every valid thread, with the threads of equal key folded first: one atomic per block
// when the whole block has one key (a cluster of millions of points would otherwise send every wave to one address), else one per
// wave and key.  Every thread of the block calls it.  s_key: 1 int, s_red: 4 words of LDS.
template <bool IS_MIN>
__device__ __forceinline__ void block_keyed_atomic(int key, bool valid, unsigned int v, unsigned int *__restrict__ dst, int *s_key,
                                                   unsigned int *s_red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr unsigned int kNeutral = IS_MIN ? 0xffffffffu : 0u;
    auto op = [](unsigned int a, unsigned int b) { return IS_MIN ? min(a, b) : a + b; };
    if (threadIdx.x == 0) *s_key = valid ? key : -2;
    __syncthreads();
    const int k0 = *s_key;
    if (__syncthreads_and(valid && key == k0)) {
        unsigned int r = v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r = op(r, (unsigned int) __shfl_xor((int) r, o, 64));
        if (lane == 0) s_red[w] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned int t = op(op(s_red[0], s_red[1]), op(s_red[2], s_red[3]));
            if (IS_MIN) atomicMin(dst + k0, t);
            else atomicAdd(dst + k0, t);
        }
        return;
    }
    bool todo = valid;
    unsigned long long m;
    while ((m = __ballot(todo)) != 0) {
        const int leader = __ffsll((long long) m) - 1;
        const int k = readlane_i(key, leader);
        const bool same = todo && key == k;
        unsigned int r = same ? v : kNeutral;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r = op(r, (unsigned int) __shfl_xor((int) r, o, 64));
        if (lane == leader) {
            if (IS_MIN) atomicMin(dst + k, r);
            else atomicAdd(dst + k, r);
        }
        if (same) todo = false;
    }
}

// ---- pass 1: counts, core flags, the forest of singletons ----
__global__ void __launch_bounds__(256)
k_cluster_count(const SPoint *__restrict__ sp, const unsigned long long *__restrict__ codes, long long n, GridView g, double r2,
                int min_points, int *__restrict__ counts, int *__restrict__ parent, unsigned int *__restrict__ min_idx,
                unsigned char *__restrict__ bflag, unsigned long long *__restrict__ n_core) {
    __shared__ WaveTile s_tile[4];
    __shared__ int2 s_tab[4][kGroupTab + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const StreamQuery q = stream_query(sp, codes, i, n, g.shift);
    int cnt = 0;
    wave_stream(q.active, q.cx, q.cy, q.cz, sp, g, lane, s_tab[w], &s_tile[w], [&](double px, double py, double pz, int, int) {
        cnt += dist2_exact(q.qx, q.qy, q.qz, px, py, pz) < r2 ? 1 : 0;
    });
    bool core = false;
    if (q.active) {
        core = cnt >= min_points;
        counts[q.idx] = cnt;
        parent[i] = core ? (int) i : -1;
        min_idx[i] = 0xffffffffu;
        bflag[i] = (!core && cnt >= 2) ? 1 : 0;  // (a border point has a core neighbour besides itself)
    }
    const int c = __syncthreads_count(core);
    if (threadIdx.x == 0 && c) atomicAdd(n_core, (unsigned long long) c);
}

// ---- pass 2: connectivity.  my = the root of this lane's set as last seen; a candidate counts when it is core (staged parent >= 0),
// lies at a smaller sorted position (every edge once) and is not known to be in the lane's set already ----
__global__ void __launch_bounds__(256)
k_cluster_union(const SPoint *__restrict__ sp, const unsigned long long *__restrict__ codes, long long n, GridView g, double r2,
                int *__restrict__ parent) {
    __shared__ WaveTile s_tile[4];
    __shared__ int2 s_tab[4][kGroupTab + 1];
    __shared__ int s_par[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const int me_pos = (int) i;
    bool core = false;
    double qx = 0, qy = 0, qz = 0;
    int cx = 0, cy = 0, cz = 0;
    int my = -1;
    if (i < n) {
        my = uf_load(parent + i);
        core = my >= 0;
    }
    if (core) {
        const SPoint q = sp[i];
        qx = q.x;
        qy = q.y;
        qz = q.z;
        cell_of(codes[i], g.shift, cx, cy, cz);
    }
    int *s_p = s_par[w];
    wave_stream_staged(
        core, cx, cy, cz, sp, g, lane, s_tab[w], &s_tile[w], [&](int j, int pos) { s_p[j] = uf_load(parent + pos); },
        [&](double px, double py, double pz, int pos, int j) {
            const int a = s_p[j];
            if (a >= 0 && a != my && pos < me_pos && dist2_exact(qx, qy, qz, px, py, pz) < r2) my = uf_unite(parent, my, a);
        });
}

// ---- pass 3: every core point to its root; the root's slot takes the smallest cloud index of its set ----
__global__ void __launch_bounds__(256)
k_cluster_flatten(const SPoint *__restrict__ sp, long long n, int *__restrict__ parent, unsigned int *__restrict__ min_idx,
                  unsigned char *__restrict__ rflag) {
    __shared__ int s_key;
    __shared__ unsigned int s_red[4];
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    int r = -1;
    unsigned int idx = 0xffffffffu;
    if (i < n) {
        int p = parent[i];
        if (p >= 0) {
            r = (int) i;
            while (p != r) {  // (other threads write roots over the pointers of this chain meanwhile: every value is an ancestor)
                r = p;
                p = uf_load(parent + r);
            }
            if (r != (int) i) parent[i] = r;
            idx = (unsigned int) sp[i].idx;
        }
        rflag[i] = r == (int) i ? 1 : 0;
    }
    block_keyed_atomic<true>(r, r >= 0, idx, min_idx, &s_key, s_red);
}

__global__ void __launch_bounds__(256)
k_cluster_root_keys(const unsigned int *__restrict__ roots, unsigned int m, const unsigned int *__restrict__ min_idx,
                    unsigned long long *__restrict__ keys) {
    const unsigned int t = blockIdx.x * 256 + threadIdx.x;
    if (t < m) keys[t] = min_idx[roots[t]];
}
// (min_idx of a root becomes the cluster id: the rank of its smallest index among the roots')
__global__ void __launch_bounds__(256)
k_cluster_root_rank(const unsigned int *__restrict__ roots_sorted, unsigned int m, unsigned int *__restrict__ min_idx) {
    const unsigned int t = blockIdx.x * 256 + threadIdx.x;
    if (t < m) min_idx[roots_sorted[t]] = t;
}

__global__ void __launch_bounds__(256)
k_cluster_core_labels(const SPoint *__restrict__ sp, long long n, int *__restrict__ parent, const unsigned int *__restrict__ min_idx,
                      int *__restrict__ labels, unsigned int *__restrict__ sizes) {
    __shared__ int s_key;
    __shared__ unsigned int s_red[4];
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    int lab = -1;
    if (i < n) {
        const int r = parent[i];  // own element only: flattened by the kernel before
        if (r >= 0) lab = (int) min_idx[r];
        parent[i] = lab;
        labels[sp[i].idx] = lab;
    }
    block_keyed_atomic<false>(lab, lab >= 0, 1u, sizes, &s_key, s_red);
}

// ---- pass 4: border points.  lab[] = label per sorted position (-1: not core), read only ----
__global__ void __launch_bounds__(256)
k_cluster_border(const SPoint *__restrict__ sp, const unsigned long long *__restrict__ codes, const unsigned int *__restrict__ list,
                 unsigned int m, GridView g, double r2, const int *__restrict__ lab, int *__restrict__ labels,
                 unsigned int *__restrict__ sizes, unsigned long long *__restrict__ n_border) {
    __shared__ WaveTile s_tile[4];
    __shared__ int2 s_tab[4][kGroupTab + 1];
    __shared__ int s_lab[4][64];
    __shared__ int s_key;
    __shared__ unsigned int s_red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned int t = blockIdx.x * 256 + threadIdx.x;
    const bool active = t < m;
    double qx = 0, qy = 0, qz = 0;
    int cx = 0, cy = 0, cz = 0;
    long long qi = 0;
    if (active) {
        const unsigned int i = list[t];
        const SPoint q = sp[i];
        qx = q.x;
        qy = q.y;
        qz = q.z;
        qi = q.idx;
        cell_of(codes[i], g.shift, cx, cy, cz);
    }
    int best = 0x7fffffff;
    int *s_l = s_lab[w];
    wave_stream_staged(
        active, cx, cy, cz, sp, g, lane, s_tab[w], &s_tile[w], [&](int j, int pos) { s_l[j] = lab[pos]; },
        [&](double px, double py, double pz, int, int j) {
            const int a = s_l[j];
            if (a >= 0 && a < best && dist2_exact(qx, qy, qz, px, py, pz) < r2) best = a;
        });
    const bool hit = active && best != 0x7fffffff;
    if (hit) labels[qi] = best;  // (k_cluster_core_labels wrote -1)
    block_keyed_atomic<false>(best, hit, 1u, sizes, &s_key, s_red);
    const int c = __syncthreads_count(hit);
    if (threadIdx.x == 0 && c) atomicAdd(n_border, (unsigned long long) c);
}

__global__ void __launch_bounds__(256)
k_cluster_largest(const unsigned int *__restrict__ sizes, unsigned int m, unsigned int *__restrict__ largest) {
    __shared__ unsigned int sm[4];
    unsigned int v = 0;
    for (unsigned int t = blockIdx.x * 256 + threadIdx.x; t < m; t += gridDim.x * 256) v = max(v, sizes[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned int) __shfl_xor((int) v, o, 64));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(largest, max(max(sm[0], sm[1]), max(sm[2], sm[3])));
}

// ---- me_cluster_keep ----
// descending size, ties by ascending id: ascending (2^32 - 1 - size) << 32 | id
__global__ void __launch_bounds__(256)
k_cluster_rank_keys(const unsigned int *__restrict__ sizes, unsigned int m, unsigned long long *__restrict__ keys) {
    const unsigned int t = blockIdx.x * 256 + threadIdx.x;
    if (t < m) keys[t] = ((unsigned long long) (0xffffffffu - sizes[t]) << 32) | t;
}
__global__ void __launch_bounds__(256)
k_cluster_rank_ok(const unsigned long long *__restrict__ keys_sorted, unsigned int m, long long min_size, long long keep_largest,
                  unsigned char *__restrict__ ok) {
    const unsigned int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const unsigned long long k = keys_sorted[t];
    const long long size = 0xffffffffu - (unsigned int) (k >> 32);
    ok[(unsigned int) k] = (size >= min_size && (long long) t < keep_largest) ? 1 : 0;
}
__global__ void __launch_bounds__(256)
k_cluster_size_ok(const unsigned int *__restrict__ sizes, unsigned int m, long long min_size, unsigned char *__restrict__ ok) {
    const unsigned int t = blockIdx.x * 256 + threadIdx.x;
    if (t < m) ok[t] = (long long) sizes[t] >= min_size ? 1 : 0;
}
__global__ void __launch_bounds__(256)
k_cluster_keep_mask(const int *__restrict__ labels, long long n, const unsigned char *__restrict__ ok, unsigned char *__restrict__ keep,
                    unsigned long long *__restrict__ kept) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    bool k = false;
    if (i < n) {
        const int l = labels[i];
        k = l >= 0 && ok[l];
        keep[i] = k ? 1 : 0;
    }
    const int c = __syncthreads_count(k);
    if (threadIdx.x == 0 && c) atomicAdd(kept, (unsigned long long) c);
}

// scalars of one call: [0] n_core u64, [8] n_border u64, [16] roots u32, [20] border candidates u32, [24] largest u32, [32] kept u64
constexpr size_t kAuxBytes = 64;

}  // namespace

int cluster_dbscan(me_ctx *ctx, int slot, double eps, int min_points, int32_t *labels_host, int32_t *counts_host, me_cluster_info *info) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_cluster_dbscan"));
    if (!(eps > 0) || !std::isfinite(eps)) return ctx->fail(ME_ERR_ARG, "me_cluster_dbscan: eps must be finite and > 0");
    if (min_points < 1) return ctx->fail(ME_ERR_ARG, "me_cluster_dbscan: min_points must be >= 1");
    Cloud &c = ctx->cloud[slot];
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    // the radius grid at eps, rebuilt as me_radius_outlier does (27-cell stencil exact for a cell edge >= eps)
    const double want_h = eps * (1.0 + 0x1p-20);
    if (!c.index_valid || c.cell_h < want_h || c.cell_h > 1.5 * want_h) {
        const double req = c.cell_size_req;
        ME_TRY(cloud_build_index(ctx, slot, eps));
        c.cell_size_req = req;
    }
    const long long n = c.n;
    const double r2 = eps * eps;
    DevBuf &counts = ctx->outlier_tmp[0], &roots = ctx->outlier_tmp[1];
    DevBuf &parent = ctx->cluster_tmp[0], &min_idx = ctx->cluster_tmp[1], &rflag = ctx->cluster_tmp[2], &bflag = ctx->cluster_tmp[3],
           &blist = ctx->cluster_tmp[4];
    DevBuf aux, keys, keys_out, roots_out;
    ME_CHECK(ctx, counts.ensure((size_t) n * 4));
    ME_CHECK(ctx, roots.ensure((size_t) n * 4));
    ME_CHECK(ctx, parent.ensure((size_t) n * 4));
    ME_CHECK(ctx, min_idx.ensure((size_t) n * 4));
    ME_CHECK(ctx, rflag.ensure((size_t) n));
    ME_CHECK(ctx, bflag.ensure((size_t) n));
    ME_CHECK(ctx, blist.ensure((size_t) n * 4));
    ME_CHECK(ctx, aux.ensure(kAuxBytes));
    ME_CHECK(ctx, c.cluster_labels.ensure((size_t) n * 4));
    c.cluster_valid = false;
    char *ax = aux.as<char>();
    unsigned long long *d_core = reinterpret_cast<unsigned long long *>(ax), *d_border = reinterpret_cast<unsigned long long *>(ax + 8);
    unsigned int *d_roots = reinterpret_cast<unsigned int *>(ax + 16), *d_bcand = reinterpret_cast<unsigned int *>(ax + 20);
    unsigned int *d_largest = reinterpret_cast<unsigned int *>(ax + 24);
    const SPoint *sp = c.sp.as<SPoint>();
    const unsigned long long *codes = c.codes.as<unsigned long long>();
    ME_CHECK(ctx, hipMemsetAsync(aux.p, 0, kAuxBytes, ctx->stream));
    {
        TimerScope ts(ctx, "cluster");
        hipLaunchKernelGGL(k_cluster_count, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, sp, codes, n, c.grid, r2, min_points, counts.as<int>(),
                           parent.as<int>(), min_idx.as<unsigned int>(), bflag.as<unsigned char>(), d_core);
        hipLaunchKernelGGL(k_cluster_union, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, sp, codes, n, c.grid, r2, parent.as<int>());
        hipLaunchKernelGGL(k_cluster_flatten, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, sp, n, parent.as<int>(), min_idx.as<unsigned int>(),
                           rflag.as<unsigned char>());
        ME_TRY(select_flagged_u32(ctx, rflag.as<unsigned char>(), n, roots.as<unsigned int>(), d_roots));
        ME_TRY(select_flagged_u32(ctx, bflag.as<unsigned char>(), n, blist.as<unsigned int>(), d_bcand));
    }
    ME_CHECK(ctx, hipGetLastError());
    unsigned long long h_core = 0, h_border = 0;
    unsigned int h_cnt[2] = {0, 0}, h_largest = 0;
    {
        MailGuard mg(ctx);  // (the grids of the numbering and of the border pass need the two list lengths)
        ME_TRY(mail_post(ctx, &h_core, d_core, 8));
        ME_TRY(mail_post(ctx, h_cnt, d_roots, 8));
        ME_TRY(mg.sync());
    }
    const unsigned int m = h_cnt[0], nb = h_cnt[1];
    ME_CHECK(ctx, c.cluster_sizes.ensure((size_t) m * 4));
    unsigned int *sizes = c.cluster_sizes.as<unsigned int>();
    if (m) {
        ME_CHECK(ctx, keys.ensure((size_t) m * 8));
        ME_CHECK(ctx, keys_out.ensure((size_t) m * 8));
        ME_CHECK(ctx, roots_out.ensure((size_t) m * 4));
        ME_CHECK(ctx, hipMemsetAsync(c.cluster_sizes.p, 0, (size_t) m * 4, ctx->stream));
        {
            TimerScope ts(ctx, "cluster");
            hipLaunchKernelGGL(k_cluster_root_keys, dim3(blocks_of(m)), dim3(256), 0, ctx->stream, roots.as<unsigned int>(), m,
                               min_idx.as<unsigned int>(), keys.as<unsigned long long>());
        }
        // (the sort has the timer "sort" of its own)
        ME_TRY(sort_pairs_u64_u32(ctx, keys.as<unsigned long long>(), keys_out.as<unsigned long long>(), roots.as<unsigned int>(),
                                  roots_out.as<unsigned int>(), m, 0, 32));
    }
    {
        TimerScope ts(ctx, "cluster");
        if (m)
            hipLaunchKernelGGL(k_cluster_root_rank, dim3(blocks_of(m)), dim3(256), 0, ctx->stream, roots_out.as<unsigned int>(), m,
                               min_idx.as<unsigned int>());
        hipLaunchKernelGGL(k_cluster_core_labels, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, sp, n, parent.as<int>(),
                           min_idx.as<unsigned int>(), c.cluster_labels.as<int>(), sizes);
        if (m && nb)
            hipLaunchKernelGGL(k_cluster_border, dim3(blocks_of(nb)), dim3(256), 0, ctx->stream, sp, codes, blist.as<unsigned int>(), nb, c.grid,
                               r2, parent.as<int>(), c.cluster_labels.as<int>(), sizes, d_border);
        if (m) hipLaunchKernelGGL(k_cluster_largest, dim3(std::min(1024u, blocks_of(m))), dim3(256), 0, ctx->stream, sizes, m, d_largest);
    }
    ME_CHECK(ctx, hipGetLastError());
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h_border, d_border, 8));
        ME_TRY(mail_post(ctx, &h_largest, d_largest, 4));
        ME_TRY(mg.sync());
    }
    if (labels_host) ME_TRY(copy_d2h(ctx, labels_host, c.cluster_labels.p, (size_t) n * 4));
    if (counts_host) ME_TRY(copy_d2h(ctx, counts_host, counts.p, (size_t) n * 4));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    c.cluster_n = m;
    c.cluster_valid = true;
    if (info) {
        info->n_in = n;
        info->n_clusters = m;
        info->n_core = (int64_t) h_core;
        info->n_border = (int64_t) h_border;
        info->n_noise = n - (int64_t) h_core - (int64_t) h_border;
        info->largest = h_largest;
    }
    return ME_OK;
}

int cluster_sizes(me_ctx *ctx, int slot, int64_t *sizes_host, long long capacity, long long *n_clusters) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_cluster_sizes"));
    Cloud &c = ctx->cloud[slot];
    if (!c.cluster_valid) return ctx->fail(ME_ERR_STATE, "me_cluster_sizes: the slot has no cluster labels (me_cluster_dbscan)");
    if (n_clusters) *n_clusters = c.cluster_n;
    if (!sizes_host) return ME_OK;
    if (capacity < c.cluster_n) return ctx->fail(ME_ERR_CAPACITY, "me_cluster_sizes: capacity below the number of clusters");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    std::vector<unsigned int> h((size_t) c.cluster_n);
    if (c.cluster_n) ME_TRY(copy_d2h(ctx, h.data(), c.cluster_sizes.p, (size_t) c.cluster_n * 4));
    for (long long k = 0; k < c.cluster_n; ++k) sizes_host[k] = h[(size_t) k];
    return ME_OK;
}

int cluster_keep(me_ctx *ctx, int slot, long long min_cluster_size, long long keep_largest, uint8_t *keep_host, me_outlier_info *info) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_cluster_keep"));
    if (min_cluster_size < 1) return ctx->fail(ME_ERR_ARG, "me_cluster_keep: min_cluster_size must be >= 1");
    if (keep_largest < 0) return ctx->fail(ME_ERR_ARG, "me_cluster_keep: keep_largest must be >= 0");
    Cloud &c = ctx->cloud[slot];
    if (!c.cluster_valid) return ctx->fail(ME_ERR_STATE, "me_cluster_keep: the slot has no cluster labels (me_cluster_dbscan)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = c.n;
    const unsigned int m = (unsigned int) c.cluster_n;
    DevBuf aux, ok, keys, keys_out;
    ME_CHECK(ctx, aux.ensure(kAuxBytes));
    ME_CHECK(ctx, ok.ensure((size_t) m));
    ME_CHECK(ctx, c.outlier_keep.ensure((size_t) n));
    c.outlier_keep_valid = false;
    unsigned long long *kept = reinterpret_cast<unsigned long long *>(aux.as<char>() + 32);
    ME_CHECK(ctx, hipMemsetAsync(aux.p, 0, kAuxBytes, ctx->stream));
    const unsigned int *sizes = c.cluster_sizes.as<unsigned int>();
    if (m && keep_largest > 0 && keep_largest < (long long) m) {
        ME_CHECK(ctx, keys.ensure((size_t) m * 8));
        ME_CHECK(ctx, keys_out.ensure((size_t) m * 8));
        hipLaunchKernelGGL(k_cluster_rank_keys, dim3(blocks_of(m)), dim3(256), 0, ctx->stream, sizes, m, keys.as<unsigned long long>());
        ME_TRY(sort_keys_u64(ctx, keys.as<unsigned long long>(), keys_out.as<unsigned long long>(), m, 0, 64));
        TimerScope ts(ctx, "cluster");
        hipLaunchKernelGGL(k_cluster_rank_ok, dim3(blocks_of(m)), dim3(256), 0, ctx->stream, keys_out.as<unsigned long long>(), m,
                           min_cluster_size, keep_largest, ok.as<unsigned char>());
    } else if (m) {
        TimerScope ts(ctx, "cluster");
        hipLaunchKernelGGL(k_cluster_size_ok, dim3(blocks_of(m)), dim3(256), 0, ctx->stream, sizes, m, min_cluster_size, ok.as<unsigned char>());
    }
    {
        TimerScope ts(ctx, "cluster");
        hipLaunchKernelGGL(k_cluster_keep_mask, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, c.cluster_labels.as<int>(), n,
                           ok.as<unsigned char>(), c.outlier_keep.as<unsigned char>(), kept);
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
        info->threshold = (double) min_cluster_size;
    }
    return ME_OK;
}

}  // namespace me
