// me_orient.hip — consistent orientation of the resident normals by propagation over the k-NN graph: Hoppe et al. 1992, Open3D's
// PointCloud::OrientNormalsConsistentTangentPlane without its Delaunay / Euclidean-MST edges.  The definition is in
// include/mapeval_hip.h; tests/_orient_ref.py restates it.
//   k_orient_valid    per point: the validity byte (normal != (0, 0, 0)) and the forest of singletons, word[i] = i << 1
//   k_orient_lists    one lane per SORTED point: the (k+1)-list of the point in its own cloud by (d2, original index) — the walk and the
//                     LDS list of k_knn_cross (me_search.hip) — written as int32[N][k+1] in cloud order with the point itself, the
//                     padding and the invalid neighbours replaced by -1.  The lists never leave the device.          ("orient_walk")
//   k_orient_emit     one thread per list entry (i, j): the undirected edge {i, j} is appended ONCE — by i when j > i, by i when j < i and
//                     j does not list i — with its key, 1 + the bit pattern of |c|
//   Boruvka rounds over the edge array, every step an integer atomic whose result does not depend on the order of arrival:
//   k_orient_best_c   per live edge between two trees: atomicMax of the key into both trees' slots; an edge inside a tree is retired
//                     (key 0) and costs 8 bytes per later round
//   k_orient_best_e   among the edges that hold a tree's maximum: atomicMin of (lo << 32 | hi).  (|c| descending, lo, hi) is a strict
//                     total order, so the pick is the tree's smallest outgoing edge and two trees that pick each other pick the SAME edge
//   k_orient_hook     per tree: hook[r] = (other tree << 1) | relative sign; of a mutual pair the smaller representative stays a root.
//                     The words of the POINTS are not touched here: a representative that hooks at the same time is still read as itself
//   k_orient_chase    per tree, hook -> a second buffer: up to kChaseSteps steps towards the root, XOR-ing the sign bits; a flag asks for
//                     another pass (depth / kChaseSteps per pass; one pass in practice)
//   k_orient_apply    every point composes its word with its representative's chased hook                             ("orient_forest")
//   k_orient_root_a / _b / _c   per tree: size, lowest member, the maximum of an order-preserving integer image of the projection on
//                     `direction`, the lowest index among its holders, that root's flip
//   k_orient_final    component (the exclusive scan of the "lowest member" flags), flipped = flip(root) ^ parity(root) ^ parity(i)
//   k_orient_incons   per edge: (c < 0) ^ flipped[lo] ^ flipped[hi];  k_orient_negate: the flipped normals negated
// The forest is the unique minimum spanning forest under the strict order, and the parity of the path between two points of a tree is a
// property of the tree: nothing above depends on which hooks happened in which round.  No float atomics.  -ffp-contract=off.
#include <cmath>
#include <cstring>

#include "me_internal.hpp"
#include "me_oct_walk.hpp"

namespace me {

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kOrientBlock = 128;  // k_orient_lists: (k + 1) = 40 x 128 lanes x 12 B = 60 KB of LDS (k_knn_cross's figure)
static_assert(kKnnMax * kOrientBlock * 12 + kMaxLevels * 8 <= 64 * 1024, "the lists and the level offsets fit one workgroup's LDS");
constexpr int kChaseSteps = 64;

enum { kCntEdges = 0, kCntHooks, kCntChase, kCntValid, kCntFlipped, kCntIncons, kCntLargest, kCntWords };

// count the set predicates of a 256-thread block into *dst with one atomic
__device__ __forceinline__ void block_count(bool pred, u64 *dst) {
    const int c = __syncthreads_count(pred);
    if (threadIdx.x == 0 && c) atomicAdd(dst, (u64) c);
}

__global__ void __launch_bounds__(256)
k_orient_valid(const double *__restrict__ nrm, long long n, unsigned char *__restrict__ vflag, u32 *__restrict__ word, u64 *__restrict__ cnt) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    bool v = false;
    if (i < n) {
        v = nrm[3 * i] != 0.0 || nrm[3 * i + 1] != 0.0 || nrm[3 * i + 2] != 0.0;
        vflag[i] = v ? 1 : 0;
        word[i] = (u32) i << 1;
    }
    block_count(v, cnt + kCntValid);
}

// lists: int32[n][kk] in cloud order; kk = k + 1
__global__ void __launch_bounds__(kOrientBlock)
k_orient_lists(const SPoint *__restrict__ sp, long long n, OctView oct, int kk, const unsigned char *__restrict__ vflag,
               int *__restrict__ lists) {
    extern __shared__ double s_dyn[];
    double *s_d = s_dyn;                                             // [kk][kOrientBlock]
    int *s_i = reinterpret_cast<int *>(s_dyn + kk * kOrientBlock);  // [kk][kOrientBlock]
    __shared__ long long s_off[kMaxLevels];
    if (threadIdx.x < kMaxLevels) s_off[threadIdx.x] = oct.off[threadIdx.x];
    __syncthreads();
    const int tid = threadIdx.x;
    const long long i = (long long) blockIdx.x * kOrientBlock + tid;
    if (i >= n) return;
    const SPoint q = sp[i];
    const long long qi = q.idx;
    int cnt = 0;
    if (vflag[qi]) {
        const ONode *__restrict__ nodes = oct.nodes;
        const double qx = q.x, qy = q.y, qz = q.z;
        double worst = INFINITY;
        auto consider = [&](double d, int pi) {
            if (cnt == kk) {
                if (!(d < worst || (d == worst && pi < s_i[(kk - 1) * kOrientBlock + tid]))) return;
            }
            int pos = cnt < kk ? cnt : kk - 1;
            while (pos > 0) {
                const double pd = s_d[(pos - 1) * kOrientBlock + tid];
                const int pidx = s_i[(pos - 1) * kOrientBlock + tid];
                if (d < pd || (d == pd && pi < pidx)) {
                    s_d[pos * kOrientBlock + tid] = pd;
                    s_i[pos * kOrientBlock + tid] = pidx;
                    --pos;
                } else {
                    break;
                }
            }
            s_d[pos * kOrientBlock + tid] = d;
            s_i[pos * kOrientBlock + tid] = pi;
            if (cnt < kk) ++cnt;
            if (cnt == kk) worst = s_d[(kk - 1) * kOrientBlock + tid];
        };
        oct_walk_nearest(
            nodes, s_off, oct.n_levels - 1, qx, qy, qz, [&](double lb) { return lb <= worst; },
            [&](long long leaf) {
                const long long jb = nodes[leaf].begin, je = nodes[leaf + 1].begin;
                for (long long j = jb; j < je; ++j) {
                    const SPoint p = sp[j];
                    consider(dist2_exact(qx, qy, qz, p.x, p.y, p.z), (int) p.idx);
                }
            });
    }
    for (int j = 0; j < kk; ++j) {
        int e = -1;
        if (j < cnt) {
            e = s_i[j * kOrientBlock + tid];
            if (e == (int) qi || !vflag[e]) e = -1;  // (an invalid neighbour is skipped, not replaced by the next nearest)
        }
        lists[qi * kk + j] = e;
    }
}

__global__ void __launch_bounds__(256)
k_orient_emit(const int *__restrict__ lists, long long n, int kk, const double *__restrict__ nrm, u64 *__restrict__ e_pair,
              u64 *__restrict__ e_key, u64 *__restrict__ cnt) {
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool emit = false;
    long long i = 0, j = -1;
    if (t < n * kk) {
        i = t / kk;
        j = lists[t];
        if (j >= 0) {
            emit = true;
            if (j < i) {  // the smaller end appends the pair when it lists this point
                const int *__restrict__ lj = lists + j * kk;
                for (int s = 0; s < kk; ++s)
                    if (lj[s] == (int) i) emit = false;
            }
        }
    }
    const u64 m = __ballot(emit);
    if (m == 0) return;
    const int leader = __ffsll((long long) m) - 1;
    u64 base = 0;
    if (lane == leader) base = atomicAdd(cnt + kCntEdges, (u64) __popcll(m));
    const u32 blo = (u32) __shfl((int) (u32) base, leader, 64), bhi = (u32) __shfl((int) (u32) (base >> 32), leader, 64);
    if (!emit) return;
    const u64 pos = (((u64) bhi << 32) | blo) + (u64) __popcll(m & ((1ULL << lane) - 1ULL));
    const long long lo = i < j ? i : j, hi = i < j ? j : i;
    const double c = dot3(nrm + 3 * lo, nrm + 3 * hi);
    e_pair[pos] = ((u64) lo << 32) | (u64) hi;
    e_key[pos] = (u64) __double_as_longlong(fabs(c)) + 1ULL;  // (|c| >= +0.0: the bit pattern orders as an unsigned integer; 0 = retired)
}

__global__ void __launch_bounds__(256)
k_orient_best_c(const u64 *__restrict__ e_pair, u64 *__restrict__ e_key, long long ne, const u32 *__restrict__ word, u64 *__restrict__ best_c) {
    const long long e = (long long) blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const u64 key = e_key[e];
    if (key == 0) return;
    const u64 pr = e_pair[e];
    const u32 ru = word[(u32) (pr >> 32)] >> 1, rv = word[(u32) pr] >> 1;
    if (ru == rv) {
        e_key[e] = 0;
        return;
    }
    atomicMax(best_c + ru, key);
    atomicMax(best_c + rv, key);
}

__global__ void __launch_bounds__(256)
k_orient_best_e(const u64 *__restrict__ e_pair, const u64 *__restrict__ e_key, long long ne, const u32 *__restrict__ word,
                const u64 *__restrict__ best_c, u64 *__restrict__ best_e) {
    const long long e = (long long) blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const u64 key = e_key[e];
    if (key == 0) return;  // (k_orient_best_c has retired every edge inside a tree)
    const u64 pr = e_pair[e];
    const u32 ru = word[(u32) (pr >> 32)] >> 1, rv = word[(u32) pr] >> 1;
    if (best_c[ru] == key) atomicMin(best_e + ru, pr);
    if (best_c[rv] == key) atomicMin(best_e + rv, pr);
}

// hook[i] for EVERY point index: (i << 1) unless i is a representative that hooks
__global__ void __launch_bounds__(256)
k_orient_hook(long long n, const unsigned char *__restrict__ vflag, const u32 *__restrict__ word, const u64 *__restrict__ best_c,
              const u64 *__restrict__ best_e, const double *__restrict__ nrm, u32 *__restrict__ hook, u64 *__restrict__ cnt) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    bool hooked = false;
    if (i < n) {
        u32 h = (u32) i << 1;
        if (vflag[i] && (word[i] >> 1) == (u32) i && best_c[i] != 0) {
            const u64 pr = best_e[i];
            const u32 lo = (u32) (pr >> 32), hi = (u32) pr;
            const u32 wl = word[lo], wh = word[hi];
            const u32 t = (wl >> 1) == (u32) i ? (wh >> 1) : (wl >> 1);
            const bool mutual = best_c[t] != 0 && best_e[t] == pr;
            if (!(mutual && (u32) i < t)) {
                const double c = dot3(nrm + 3 * (long long) lo, nrm + 3 * (long long) hi);
                h = (t << 1) | ((wl ^ wh ^ (c < 0.0 ? 1u : 0u)) & 1u);
                hooked = true;
            }
        }
        hook[i] = h;
    }
    block_count(hooked, cnt + kCntHooks);
}

// src is not written while this kernel runs: dst[i] = an ancestor of i at most kChaseSteps hooks up, with the sign to it
__global__ void __launch_bounds__(256)
k_orient_chase(long long n, const u32 *__restrict__ src, u32 *__restrict__ dst, u64 *__restrict__ cnt) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    bool more = false;
    if (i < n) {
        u32 r = (u32) i, par = 0;
        int s = 0;
        for (;; ++s) {
            const u32 h = src[r];
            if ((h >> 1) == r) break;
            if (s == kChaseSteps) {
                more = true;
                break;
            }
            par ^= h & 1u;
            r = h >> 1;
        }
        dst[i] = (r << 1) | par;
    }
    block_count(more, cnt + kCntChase);
}

__global__ void __launch_bounds__(256)
k_orient_apply(long long n, const u32 *__restrict__ word, const u32 *__restrict__ hook, u32 *__restrict__ word_out) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 w = word[i];
    const u32 h = hook[w >> 1];
    word_out[i] = (h & ~1u) | ((w ^ h) & 1u);
}

// order-preserving image of a double in the unsigned integers (-0.0 is taken as +0.0 first: equal values, equal images)
__device__ __forceinline__ u64 proj_image(const double *__restrict__ xyz, long long i, double dx, double dy, double dz) {
    double v = (xyz[3 * i] * dx + xyz[3 * i + 1] * dy) + xyz[3 * i + 2] * dz;
    if (v == 0.0) v = 0.0;
    const u64 b = (u64) __double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o) {
    const u32 lo = (u32) __shfl_xor((int) (u32) v, o, 64), hi = (u32) __shfl_xor((int) (u32) (v >> 32), o, 64);
    return ((u64) hi << 32) | lo;
}
// true when every active lane of the wave holds the same tree (the usual case: one component spans the cloud); r0 = that tree.
// The per-tree atomics below then fold the wave first: one atomic per wave instead of 64 to one address.
__device__ __forceinline__ bool wave_same_tree(bool act, u32 r, u64 m, u32 &r0) {
    r0 = (u32) __shfl((int) r, __ffsll((long long) m) - 1, 64);
    return __all(!act || r == r0) != 0;
}

// every thread of a wave takes part in the ballots: no early return before them
__global__ void __launch_bounds__(256)
k_orient_root_a(long long n, const unsigned char *__restrict__ vflag, const u32 *__restrict__ word, const double *__restrict__ xyz,
                double dx, double dy, double dz, u64 *__restrict__ best_c, u32 *__restrict__ min_idx, u32 *__restrict__ size) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const bool act = i < n && vflag[i];
    const u64 m = __ballot(act);
    if (m == 0) return;
    const u32 r = act ? word[i] >> 1 : 0u;
    u64 img = act ? proj_image(xyz, i, dx, dy, dz) : 0ULL;
    u32 lowest = act ? (u32) i : 0xffffffffu;
    u32 r0;
    if (wave_same_tree(act, r, m, r0)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 other = shfl_xor_u64(img, o);
            img = other > img ? other : img;
            lowest = min(lowest, (u32) __shfl_xor((int) lowest, o, 64));
        }
        if ((threadIdx.x & 63) == __ffsll((long long) m) - 1) {
            atomicMax(best_c + r0, img);
            atomicMin(min_idx + r0, lowest);
            atomicAdd(size + r0, (u32) __popcll(m));
        }
    } else if (act) {
        atomicMax(best_c + r, img);
        atomicMin(min_idx + r, lowest);
        atomicAdd(size + r, 1u);
    }
}

__global__ void __launch_bounds__(256)
k_orient_root_b(long long n, const unsigned char *__restrict__ vflag, const u32 *__restrict__ word, const double *__restrict__ xyz,
                double dx, double dy, double dz, const u64 *__restrict__ best_c, u64 *__restrict__ best_e) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n && vflag[i];
    const u32 r = valid ? word[i] >> 1 : 0u;
    const bool act = valid && proj_image(xyz, i, dx, dy, dz) == best_c[r];  // (a holder of its tree's maximum)
    const u64 m = __ballot(act);
    if (m == 0) return;
    u32 lowest = act ? (u32) i : 0xffffffffu;
    u32 r0;
    if (wave_same_tree(act, r, m, r0)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lowest = min(lowest, (u32) __shfl_xor((int) lowest, o, 64));
        if ((threadIdx.x & 63) == __ffsll((long long) m) - 1) atomicMin(best_e + r0, (u64) lowest);
    } else if (act) {
        atomicMin(best_e + r, (u64) i);
    }
}

// root_flip[rep] = flip(root) ^ parity(root); first[i] = 1 where i is the lowest member of its tree; the largest tree
__global__ void __launch_bounds__(256)
k_orient_root_c(long long n, const unsigned char *__restrict__ vflag, const u32 *__restrict__ word, const double *__restrict__ nrm,
                double dx, double dy, double dz, int inward, const u64 *__restrict__ best_e, const u32 *__restrict__ min_idx,
                const u32 *__restrict__ size, unsigned char *__restrict__ root_flip, u32 *__restrict__ first, u64 *__restrict__ cnt) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        first[n] = 0;  // (the scan of n + 1 entries ends with the number of components)
        return;
    }
    u32 f = 0;
    if (vflag[i]) {
        const u32 w = word[i], r = w >> 1;
        if (best_e[r] == (u64) i) {
            const double s = (nrm[3 * i] * dx + nrm[3 * i + 1] * dy) + nrm[3 * i + 2] * dz;
            const bool flip = (s < 0.0) != (inward != 0);
            root_flip[r] = (unsigned char) ((flip ? 1u : 0u) ^ (w & 1u));
        }
        f = min_idx[r] == (u32) i ? 1u : 0u;
        if (r == (u32) i) atomicMax(cnt + kCntLargest, (u64) size[i]);
    }
    first[i] = f;
}

__global__ void __launch_bounds__(256)
k_orient_final(long long n, const unsigned char *__restrict__ vflag, const u32 *__restrict__ word, const u32 *__restrict__ min_idx,
               const u32 *__restrict__ rank, const unsigned char *__restrict__ root_flip, int *__restrict__ component,
               unsigned char *__restrict__ flipped, u64 *__restrict__ cnt) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    bool f = false;
    if (i < n) {
        int comp = -1;
        if (vflag[i]) {
            const u32 w = word[i], r = w >> 1;
            comp = (int) rank[min_idx[r]];
            f = ((root_flip[r] ^ w) & 1u) != 0;
        }
        component[i] = comp;
        flipped[i] = f ? 1 : 0;
    }
    block_count(f, cnt + kCntFlipped);
}

__global__ void __launch_bounds__(256)
k_orient_incons(const u64 *__restrict__ e_pair, long long ne, const double *__restrict__ nrm, const unsigned char *__restrict__ flipped,
                u64 *__restrict__ cnt) {
    const long long e = (long long) blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (e < ne) {
        const u64 pr = e_pair[e];
        const long long lo = (long long) (pr >> 32), hi = (long long) (u32) pr;
        const double c = dot3(nrm + 3 * lo, nrm + 3 * hi);
        bad = (c < 0.0) != (flipped[lo] != flipped[hi]);
    }
    block_count(bad, cnt + kCntIncons);
}

__global__ void __launch_bounds__(256)
k_orient_negate(long long n, const unsigned char *__restrict__ flipped, double *__restrict__ nrm) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flipped[i]) return;
    nrm[3 * i] = -nrm[3 * i];
    nrm[3 * i + 1] = -nrm[3 * i + 1];
    nrm[3 * i + 2] = -nrm[3 * i + 2];
}

// the "orient_normals" timer spans the whole device phase, around the scopes of its two parts (scopes themselves do not nest)
struct OuterTimer {
    me_ctx *c;
    hipEvent_t a = nullptr, b = nullptr;
    explicit OuterTimer(me_ctx *ctx) : c(ctx) {
        if (!c->timers_on) return;
        a = c->get_event();
        b = c->get_event();
        (void) hipEventRecord(a, c->stream);
    }
    void end() {
        if (!a) return;
        (void) hipEventRecord(b, c->stream);
        c->pending.push_back({"orient_normals", a, b});
        a = b = nullptr;
    }
    ~OuterTimer() { end(); }
};

}  // namespace

int orient_normals(me_ctx *ctx, int slot, const me_orient_params *p, me_orient_out *out) {
    const char *who = "me_orient_normals";
    if (!p || !out) return ctx->fail(ME_ERR_ARG, "me_orient_normals: p and out must not be NULL");
    ME_TRY(need_single_gpu_cloud(ctx, slot, who));
    if (p->k < 1 || p->k > kKnnMax - 1) return ctx->fail(ME_ERR_ARG, "me_orient_normals: k must be in [1, 39]");
    const double dx = p->direction[0], dy = p->direction[1], dz = p->direction[2];
    if (!std::isfinite(dx) || !std::isfinite(dy) || !std::isfinite(dz) || (dx == 0 && dy == 0 && dz == 0))
        return ctx->fail(ME_ERR_ARG, "me_orient_normals: direction must be finite and not all zero");
    Cloud &c = ctx->cloud[slot];
    if (c.n <= 0) return ctx->fail(ME_ERR_STATE, "me_orient_normals: empty cloud");
    if (!c.have_normals) return ctx->fail(ME_ERR_STATE, "me_orient_normals: the cloud has no normals (me_radius_normals, me_estimate_normals or me_set_normals first)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    if (!c.index_valid) ME_TRY(cloud_build_index(ctx, slot, c.cell_size_req));  // (the one case me_knn_search documents)
    ME_TRY(cloud_finish_octree(ctx, slot));
    const long long n = c.n;
    const int kk = p->k + 1;
    const long long cap = n * kk;  // every list entry appends at most one edge
    c.orient_have = false;
    // buffers of the call, released on return; component and flipped stay with the cloud
    DevBuf b_vflag, b_lists, b_pair, b_key, b_word[2], b_hook[2], b_bc, b_be, b_rflip, b_rank, b_cnt;
    ME_CHECK(ctx, b_vflag.ensure((size_t) n));
    ME_CHECK(ctx, b_lists.ensure((size_t) cap * 4));
    ME_CHECK(ctx, b_pair.ensure((size_t) cap * 8));
    ME_CHECK(ctx, b_key.ensure((size_t) cap * 8));
    for (int s = 0; s < 2; ++s) {
        ME_CHECK(ctx, b_word[s].ensure((size_t) (n + 1) * 4));
        ME_CHECK(ctx, b_hook[s].ensure((size_t) (n + 1) * 4));
    }
    ME_CHECK(ctx, b_bc.ensure((size_t) n * 8));
    ME_CHECK(ctx, b_be.ensure((size_t) n * 8));
    ME_CHECK(ctx, b_rflip.ensure((size_t) n));
    ME_CHECK(ctx, b_rank.ensure((size_t) (n + 1) * 4));
    ME_CHECK(ctx, b_cnt.ensure(kCntWords * 8));
    ME_CHECK(ctx, c.orient_comp.ensure((size_t) n * 4));
    ME_CHECK(ctx, c.orient_flip.ensure((size_t) n));
    unsigned char *vflag = b_vflag.as<unsigned char>();
    u64 *cnt = b_cnt.as<u64>();
    u64 *e_pair = b_pair.as<u64>(), *e_key = b_key.as<u64>();
    u64 *best_c = b_bc.as<u64>(), *best_e = b_be.as<u64>();
    u32 *word = b_word[0].as<u32>(), *word_alt = b_word[1].as<u32>();
    u32 *hook = b_hook[0].as<u32>(), *hook_alt = b_hook[1].as<u32>();
    double *nrm = c.normals.as_mut<double>();
    const dim3 gn(blocks_of(n)), gn1(blocks_of(n + 1)), b256(256);
    hipStream_t st = ctx->stream;
    OuterTimer outer(ctx);
    ME_CHECK(ctx, hipMemsetAsync(cnt, 0, kCntWords * 8, st));
    u64 h_cnt[kCntWords] = {0};
    long long ne = 0;
    {
        TimerScope ts(ctx, "orient_walk");
        hipLaunchKernelGGL(k_orient_valid, gn, b256, 0, st, (const double *) nrm, n, vflag, word, cnt);
        hipLaunchKernelGGL(k_orient_lists, dim3(blocks_of(n, kOrientBlock)), dim3(kOrientBlock), (size_t) kk * kOrientBlock * 12, st,
                           c.sp.as<SPoint>(), n, c.oct, kk, (const unsigned char *) vflag, b_lists.as<int>());
    }
    ME_CHECK(ctx, hipGetLastError());
    int rounds = 0;
    {
        TimerScope ts(ctx, "orient_forest");
        hipLaunchKernelGGL(k_orient_emit, dim3(blocks_of(cap)), b256, 0, st, (const int *) b_lists.as<int>(), n, kk, (const double *) nrm, e_pair,
                           e_key, cnt);
        ME_CHECK(ctx, hipGetLastError());
        {
            MailGuard mg(ctx);
            ME_TRY(mail_post(ctx, h_cnt, cnt, kCntWords * 8));
            ME_TRY(mg.sync());
        }
        ne = (long long) h_cnt[kCntEdges];
        if (ne > cap) return ctx->fail(ME_ERR_HIP, "me_orient_normals: internal error, more edges than list entries");
        const dim3 ge(blocks_of(ne));
        u64 hooks_before = 0;
        while (ne > 0) {
            ++rounds;
            ME_CHECK(ctx, hipMemsetAsync(best_c, 0, (size_t) n * 8, st));
            ME_CHECK(ctx, hipMemsetAsync(best_e, 0xff, (size_t) n * 8, st));
            ME_CHECK(ctx, hipMemsetAsync(cnt + kCntChase, 0, 8, st));
            hipLaunchKernelGGL(k_orient_best_c, ge, b256, 0, st, (const u64 *) e_pair, e_key, ne, (const u32 *) word, best_c);
            hipLaunchKernelGGL(k_orient_best_e, ge, b256, 0, st, (const u64 *) e_pair, (const u64 *) e_key, ne, (const u32 *) word,
                               (const u64 *) best_c, best_e);
            hipLaunchKernelGGL(k_orient_hook, gn, b256, 0, st, n, (const unsigned char *) vflag, (const u32 *) word, (const u64 *) best_c,
                               (const u64 *) best_e, (const double *) nrm, hook, cnt);
            // (the hooks of a round form a forest — a tree's pick is its smallest outgoing edge under a strict order, mutual picks are
            // broken — so a pass shortens every chain 64-fold and a round at least halves the trees: the two bounds only guard the host
            // against looping on a device error)
            if (rounds > 64) return ctx->fail(ME_ERR_HIP, "me_orient_normals: internal error, the forest did not converge");
            for (int pass = 0;; ++pass) {
                if (pass > 8) return ctx->fail(ME_ERR_HIP, "me_orient_normals: internal error, a hook chain did not end");
                hipLaunchKernelGGL(k_orient_chase, gn, b256, 0, st, n, (const u32 *) hook, hook_alt, cnt);
                ME_CHECK(ctx, hipGetLastError());
                std::swap(hook, hook_alt);
                MailGuard mg(ctx);
                ME_TRY(mail_post(ctx, h_cnt, cnt, kCntWords * 8));
                ME_TRY(mg.sync());
                if (h_cnt[kCntChase] == 0) break;
                ME_CHECK(ctx, hipMemsetAsync(cnt + kCntChase, 0, 8, st));
            }
            if (h_cnt[kCntHooks] == hooks_before) break;  // no tree had an outgoing edge: the forest is complete
            hooks_before = h_cnt[kCntHooks];
            hipLaunchKernelGGL(k_orient_apply, gn, b256, 0, st, n, (const u32 *) word, (const u32 *) hook, word_alt);
            std::swap(word, word_alt);
        }
        // roots, components, flips
        u32 *min_idx = hook, *size = hook_alt, *first = word_alt, *rank = b_rank.as<u32>();
        ME_CHECK(ctx, hipMemsetAsync(best_c, 0, (size_t) n * 8, st));
        ME_CHECK(ctx, hipMemsetAsync(best_e, 0xff, (size_t) n * 8, st));
        ME_CHECK(ctx, hipMemsetAsync(min_idx, 0xff, (size_t) n * 4, st));
        ME_CHECK(ctx, hipMemsetAsync(size, 0, (size_t) n * 4, st));
        ME_CHECK(ctx, hipMemsetAsync(b_rflip.p, 0, (size_t) n, st));
        hipLaunchKernelGGL(k_orient_root_a, gn, b256, 0, st, n, (const unsigned char *) vflag, (const u32 *) word, c.xyz.as<double>(), dx, dy,
                           dz, best_c, min_idx, size);
        hipLaunchKernelGGL(k_orient_root_b, gn, b256, 0, st, n, (const unsigned char *) vflag, (const u32 *) word, c.xyz.as<double>(), dx, dy,
                           dz, (const u64 *) best_c, best_e);
        hipLaunchKernelGGL(k_orient_root_c, gn1, b256, 0, st, n, (const unsigned char *) vflag, (const u32 *) word, (const double *) nrm, dx, dy,
                           dz, p->inward, (const u64 *) best_e, (const u32 *) min_idx, (const u32 *) size, b_rflip.as<unsigned char>(), first,
                           cnt);
        ME_CHECK(ctx, hipGetLastError());
        ME_TRY(exclusive_scan_u32(ctx, first, rank, n + 1));
        hipLaunchKernelGGL(k_orient_final, gn, b256, 0, st, n, (const unsigned char *) vflag, (const u32 *) word, (const u32 *) min_idx,
                           (const u32 *) rank, (const unsigned char *) b_rflip.as<unsigned char>(), c.orient_comp.as<int>(),
                           c.orient_flip.as<unsigned char>(), cnt);
        if (ne > 0)
            hipLaunchKernelGGL(k_orient_incons, ge, b256, 0, st, (const u64 *) e_pair, ne, (const double *) nrm,
                               (const unsigned char *) c.orient_flip.as<unsigned char>(), cnt);
        hipLaunchKernelGGL(k_orient_negate, gn, b256, 0, st, n, (const unsigned char *) c.orient_flip.as<unsigned char>(), nrm);
        ME_CHECK(ctx, hipGetLastError());
    }
    outer.end();
    u32 n_comp = 0;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, h_cnt, cnt, kCntWords * 8));
        ME_TRY(mail_post(ctx, &n_comp, b_rank.as<u32>() + n, 4));
        ME_TRY(mg.sync());
    }
    // the normals were replaced in place, as me_set_normals would: covariances and features made from the old ones go
    c.have_cov = false;
    c.fpfh_valid = false;
    c.orient_have = true;
    ctx->orient_rounds = rounds;
    out->n = n;
    out->n_valid = (int64_t) h_cnt[kCntValid];
    out->n_components = (int64_t) n_comp;
    out->largest_component = (int64_t) h_cnt[kCntLargest];
    out->n_tree_edges = (int64_t) h_cnt[kCntHooks];
    out->n_graph_edges = ne;
    out->n_flipped = (int64_t) h_cnt[kCntFlipped];
    out->n_inconsistent_edges = (int64_t) h_cnt[kCntIncons];
    return ME_OK;
}

int orient_fetch(me_ctx *ctx, int slot, int32_t *component_host, uint8_t *flipped_host) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_orient_fetch"));
    Cloud &c = ctx->cloud[slot];
    if (!c.orient_have) return ctx->fail(ME_ERR_STATE, "me_orient_fetch: no current me_orient_normals result on the slot");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    if (component_host) ME_TRY(copy_d2h(ctx, component_host, c.orient_comp.p, (size_t) c.n * 4));
    if (flipped_host) ME_TRY(copy_d2h(ctx, flipped_host, c.orient_flip.p, (size_t) c.n));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

}  // namespace me
