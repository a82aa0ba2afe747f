// me_errdist.hip — the distribution of a direction's 1-NN errors: exact quantiles, the one-sided Hausdorff distance, threshold counts
// for precision / recall / F-score and an error histogram, and the exact multi-rank select they need (the definitions are in
// include/mapeval_hip.h).  It stands beside the reference's only statistics of that kind, the f1 vector of
// calculateMetricsWithInitialMatrix (map_eval.cpp:1245-1253) and the mean of computeChamferDistance (map_eval.cpp:1398-1431).
// One pass over n (value, use byte) pairs — the key of a value is the bit pattern of v + 0.0, its order the numeric order:
//   k_ed_stat    a fixed grid of at most kEdStatBlocks blocks strides over the entries with four loads in flight (k_nn_partial's walk):
//                the use byte (d2 >= 0 and gate_pass; for the direct entry: the caller's byte and the value inside the contract), the
//                counts, the smallest and the largest key, the (largest key, smallest original index) pair, the threshold counts and the
//                two sums; the block's partial record and the one-block total over the records are me_reduce.hpp's
//   k_ed_hist   the bin of every used entry by a binary search of the edge table staged in LDS (4096 x 8 B), an LDS histogram of
//                integer counts, one integer atomic per non-empty (block, bin)
// Multi-rank radix select, most significant digit first, eight passes of eight bits, up to 16 ranks at once:
//   k_rs_start   one slot with an empty prefix that carries every rank; a rank outside [0, count) raises the flag
//   k_rs_hist    THE HOT KERNEL: block b walks the b-th contiguous piece of the current list; an entry that carries the prefix of a
//                slot adds one to the LDS histogram (slot, digit) — a wave whose entries all fall into one bin adds its population
//                with one atomic — and to the block's count of such entries
//   k_rs_narrow  one block: per slot the inclusive scan of its 256 counters, per rank the digit it falls into (binary search) and its
//                rank below it; ranks that part get slots of their own.  Then the compaction rule: when the entries that carried a
//                prefix in this pass are at most 1/8 of the list (and the list is worth it), the block counts are scanned
//   k_rs_scatter ... and block b copies its matching entries, in order, to its place in the next list: later passes read that list
//   k_rs_out     me_rank_stats from the counters, the totals and the finished prefixes
// The file is compiled with -ffp-contract=off like the rest of the library.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "me_internal.hpp"
#include "me_reduce.hpp"
#include "me_stat.hpp"

namespace me {

namespace {

typedef unsigned long long u64;

constexpr int kRsMax = ME_RANK_MAX;
constexpr int kRsBits = 8;                     // digit width: 16 slots x 256 counters x 4 B = 16 KB of LDS, eight blocks per CU
constexpr int kRsBins = 1 << kRsBits;
constexpr int kRsPasses = 64 / kRsBits;
constexpr unsigned int kRsHistBlocks = 2048;   // pieces of the list (k_rs_hist, k_rs_scatter): 256 threads x 8 block counts in the scan
constexpr long long kRsCompactMin = 32768;     // a list of fewer entries is not compacted (one read of it costs less than the launches)
constexpr int kRsCompactDiv = 8;               // compact when the surviving entries are at most 1 / 8 of the list
constexpr unsigned int kEdStatBlocks = 1024;   // k_ed_stat: above 256 x 1024 entries a block strides over the array
constexpr int kEdNI = 2 + ME_ERRDIST_MAX_THRESHOLDS;  // integer sums per block: n_query, n_used, n_within[8]
constexpr int kEdMaxBins = ME_ERRDIST_MAX_BINS;
// a record: d = sum_d, sum_d2; i = the sums, then the largest key, its argmax and the smallest key
typedef RedBufs<2, kEdNI, true> EdRed;
enum { kEdMx = kEdNI, kEdArg, kEdMn };

struct RsList {
    const double *v;
    const unsigned char *use;  // nullptr: every entry is used
    long long n;
};

struct RsBlock {
    u64 hist[kRsMax * kRsBins];
    long long blkcnt[kRsHistBlocks], blkoff[kRsHistBlocks];
    u64 prefix[kRsMax];    // per slot: the digits found so far, in place (the lower bits zero)
    int slot_of[kRsMax];   // per rank
    long long rank[kRsMax];     // per rank: the rank among the entries that carry its slot's prefix
    long long rank_in[kRsMax];  // the ranks asked for (uploaded)
    int n_slots, n_ranks, compact, n_compact;
    long long live_n;      // entries of the current list that carry a live prefix
    RsList cur, src;       // the list the next pass reads; the list a pending k_rs_scatter reads
    double *buf[2];        // the two compacted lists, used in turn
    long long cap[2];
    EdRed::Totals tot;     // stat_device
    unsigned int err, pad;
    me_rank_stats out;
    long long out_compact[2];  // compactions done, entries of the last list
};

struct EdThr {
    double t2[ME_ERRDIST_MAX_THRESHOLDS];
    int n;
};

__device__ __forceinline__ u64 key_of(double v) { return (u64) __double_as_longlong(v + 0.0); }  // (-0.0 + 0.0 = +0.0)

// mode 0: the 1-NN distances of a cloud (used = d2 >= 0 and gate_pass; `sp` gives the original index)
// mode 1: the direct entry (used = the caller's byte; a used value that is negative or not finite raises the flag and is ignored)
template <int MODE>
__global__ void __launch_bounds__(256)
k_ed_stat(const double *__restrict__ v, const unsigned char *__restrict__ use_in, const SPoint *__restrict__ sp, long long n, StatParams gp,
          EdThr thr, unsigned char *__restrict__ use_out, long long *__restrict__ pi, double *__restrict__ pd, unsigned int *__restrict__ err) {
    long long arg = -1, ci[kEdNI];  // n_query, n_used, n_within[8]
    u64 mn = ~0ull, mx = 0ull;
    double sd[2] = {0.0, 0.0};      // sum_d, sum_d2
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kEdNI; ++k) ci[k] = 0;
    auto take = [&](long long i, double d2, unsigned char ub) {
        bool used;
        if (MODE == 0) {
            if (d2 >= 0.0) ci[0] += 1;
            used = d2 >= 0.0 && gate_pass(gp, d2);
        } else {
            used = ub != 0;
            if (used && (!(d2 >= 0.0) || d2 == INFINITY)) {
                bad = true;
                used = false;
            }
            if (used) ci[0] += 1;
        }
        use_out[i] = used ? 1 : 0;
        if (!used) return;
        const u64 k = key_of(d2);
        ci[1] += 1;
        mn = k < mn ? k : mn;
        if (k >= mx) {  // (rare once the walk has seen a large value: the index is loaded only then)
            const long long o = MODE == 0 ? sp[i].idx : i;
            if (k > mx || arg < 0 || o < arg) arg = o;
            mx = k;
        }
        sd[0] += sqrt(d2);
        sd[1] += d2;
#pragma unroll
        for (int q = 0; q < ME_ERRDIST_MAX_THRESHOLDS; ++q)
            if (q < thr.n && d2 <= thr.t2[q]) ci[2 + q] += 1;
    };
    const long long S = (long long) gridDim.x * 256;
    long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * S < n; i += 4 * S) {
        const double a0 = v[i], a1 = v[i + S], a2 = v[i + 2 * S], a3 = v[i + 3 * S];
        unsigned char u0 = 1, u1 = 1, u2 = 1, u3 = 1;
        if (MODE == 1 && use_in) u0 = use_in[i], u1 = use_in[i + S], u2 = use_in[i + 2 * S], u3 = use_in[i + 3 * S];
        take(i, a0, u0);
        take(i + S, a1, u1);
        take(i + 2 * S, a2, u2);
        take(i + 3 * S, a3, u3);
    }
    for (; i < n; i += S) take(i, v[i], (MODE == 1 && use_in) ? use_in[i] : (unsigned char) 1);
    if (bad) atomicOr(err, 1u);
    red_store_partial<2, kEdNI, true>(sd, ci, mx, arg, mn, pd + (size_t) blockIdx.x * 2, pi + (size_t) blockIdx.x * EdRed::Totals::NR);
}

// hist[j], j in [0, n_bins]: the used entries with E[j - 1] < d2 <= E[j] (E[-1] = -inf), hist[n_bins] those beyond the last edge.
// 32 KB of LDS for the edges, 16 KB for the counters; the bin index is the result of a search over [0, n_bins] and bounds both.
__global__ void __launch_bounds__(256)
k_ed_hist(const double *__restrict__ v, const unsigned char *__restrict__ use, long long n, const double *__restrict__ edges, int n_bins,
          u64 *__restrict__ hist) {
    __shared__ double s_e[kEdMaxBins];
    __shared__ unsigned int s_h[kEdMaxBins + 1];
    for (int t = threadIdx.x; t < kEdMaxBins; t += 256) s_e[t] = t < n_bins ? edges[t] : INFINITY;
    for (int t = threadIdx.x; t <= kEdMaxBins; t += 256) s_h[t] = 0u;
    __syncthreads();
    const long long S = (long long) gridDim.x * 256;
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += S) {
        if (!use[i]) continue;
        const double d2 = v[i];
        int lo = 0, hi = n_bins;  // the number of edges below d2: the first j with E[j] >= d2
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_e[mid] < d2) lo = mid + 1;
            else hi = mid;
        }
        atomicAdd(&s_h[lo], 1u);
    }
    __syncthreads();
    for (int t = threadIdx.x; t <= n_bins; t += 256) {
        const unsigned int c = s_h[t];
        if (c) atomicAdd(&hist[t], (u64) c);
    }
}

__global__ void __launch_bounds__(256)
k_rs_start(RsBlock *__restrict__ b, const double *values, const unsigned char *use, long long n, int n_ranks, double *buf0, long long cap0,
           double *buf1, long long cap1) {
    for (int t = threadIdx.x; t < kRsMax * kRsBins; t += 256) b->hist[t] = 0ull;
    const long long count = b->tot.i[1];
    if ((int) threadIdx.x < kRsMax) {
        const int j = threadIdx.x;
        long long r = 0;
        if (j < n_ranks) {
            r = b->rank_in[j];
            if (r < 0 || r >= count) {
                atomicOr(&b->err, 2u);
                r = 0;
            }
        }
        b->slot_of[j] = 0;
        b->rank[j] = r;
        b->prefix[j] = 0ull;
    }
    if (threadIdx.x == 0) {
        const int live = (count > 0 && n_ranks > 0) ? 1 : 0;
        b->n_slots = live;
        b->n_ranks = live ? n_ranks : 0;
        b->compact = 0;
        b->n_compact = 0;
        b->live_n = count;
        b->cur.v = values;
        b->cur.use = use;
        b->cur.n = n;
        b->src = b->cur;
        b->buf[0] = buf0;
        b->buf[1] = buf1;
        b->cap[0] = cap0;
        b->cap[1] = cap1;
    }
}

// the piece of block `blk` of a list of n entries cut into `nblk` pieces (a multiple of 256 entries each)
__device__ __forceinline__ void rs_piece(long long n, unsigned int nblk, unsigned int blk, long long &i0, long long &i1) {
    const long long per = (((n + nblk - 1) / nblk) + 255) & ~255ll;
    i0 = (long long) blk * per;
    i1 = i0 + per < n ? i0 + per : n;
}
// the slot whose prefix the key carries, -1: none (the prefixes of the live slots are distinct)
__device__ __forceinline__ int rs_slot(const u64 *s_pre, int n_slots, u64 top) {
    int s = -1;
    for (int q = 0; q < n_slots; ++q)
        if (top == s_pre[q]) s = q;
    return s;
}

// mask = the key bits above this pass' digit (0 in the first pass), shift = the bits below it.  16 KB of LDS for the histograms; every
// LDS index is bounded by the slot search (s < n_slots <= 16) and the 8-bit digit, every read by the piece's end (<= n).
__global__ void __launch_bounds__(256) k_rs_hist(RsBlock *__restrict__ b, u64 mask, int shift) {
    __shared__ unsigned int s_h[kRsMax * kRsBins];
    __shared__ u64 s_pre[kRsMax];
    __shared__ long long smi[4];
    const int ns = min(b->n_slots, kRsMax);
    for (int t = threadIdx.x; t < kRsMax * kRsBins; t += 256) s_h[t] = 0u;
    if ((int) threadIdx.x < kRsMax) s_pre[threadIdx.x] = b->prefix[threadIdx.x];
    __syncthreads();
    const RsList L = b->cur;
    long long i0, i1;
    rs_piece(L.n, gridDim.x, blockIdx.x, i0, i1);
    const int lane = threadIdx.x & 63;
    long long cnt = 0;
    auto take = [&](bool used, double v) {
        int bin = -1;
        if (used) {
            const u64 k = key_of(v);
            const int s = rs_slot(s_pre, ns, k & mask);
            if (s >= 0) bin = s * kRsBins + (int) ((k >> shift) & (u64) (kRsBins - 1));
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
        cnt += bin >= 0 ? 1 : 0;
    };
    if (ns > 0) {
        for (long long base = i0 + threadIdx.x; base < i1 + threadIdx.x; base += 1024) {  // (block-uniform trip count; four loads in flight)
            bool u[4];
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long i = base + q * 256;
                u[q] = i < i1 && (!L.use || L.use[i]);
                v[q] = u[q] ? L.v[i] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) take(u[q], v[q]);
        }
    }
    const long long c = block_sum_256_ll(cnt, smi);
    if (threadIdx.x == 0) b->blkcnt[blockIdx.x] = c;
    __syncthreads();
    for (int t = threadIdx.x; t < ns * kRsBins; t += 256) {
        const unsigned int h = s_h[t];
        if (h) atomicAdd(&b->hist[t], (u64) h);
    }
}

// inclusive scan over the 256 threads of the block; `sw` holds 4 values
__device__ __forceinline__ long long block_scan_256(long long x, long long *sw) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();
    if (lane == 63) sw[w] = x;
    __syncthreads();
    for (int q = 0; q < w; ++q) x += sw[q];
    return x;
}

// one block.  nblk = the grid of k_rs_hist / k_rs_scatter (<= kRsHistBlocks); last = no compaction after this pass
__global__ void __launch_bounds__(256) k_rs_narrow(RsBlock *__restrict__ b, int shift, unsigned int nblk, int last) {
    __shared__ long long s_incl[kRsMax][kRsBins];
    __shared__ long long sw[4];
    __shared__ int s_dig[kRsMax], s_old[kRsMax], s_new[kRsMax];
    __shared__ long long s_rank[kRsMax], s_pop[kRsMax];
    __shared__ u64 s_pre[kRsMax];
    __shared__ int s_compact;
    const int ns = min(b->n_slots, kRsMax), nr = min(b->n_ranks, kRsMax);
    for (int s = 0; s < ns; ++s) s_incl[s][threadIdx.x] = block_scan_256((long long) b->hist[s * kRsBins + threadIdx.x], sw);
    __syncthreads();
    if ((int) threadIdx.x < nr) {
        const int j = threadIdx.x, s = min(max(b->slot_of[j], 0), kRsMax - 1);
        const long long r = b->rank[j];
        int lo = 0, hi = kRsBins - 1;  // the first digit whose inclusive count exceeds the rank (the rank is below the slot's population)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_incl[s][mid] <= r) lo = mid + 1;
            else hi = mid;
        }
        s_old[j] = s;
        s_dig[j] = lo;
        s_rank[j] = r - (lo ? s_incl[s][lo - 1] : 0);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n_new = 0;
        long long live = 0;
        for (int j = 0; j < nr; ++j) {
            const int s = s_old[j], d = s_dig[j];
            int f = -1;
            for (int q = 0; q < j; ++q)
                if (s_old[q] == s && s_dig[q] == d) f = s_new[q];
            if (f < 0) {
                f = n_new++;
                s_pre[f] = b->prefix[s] | ((u64) d << shift);
                s_pop[f] = s_incl[s][d] - (d ? s_incl[s][d - 1] : 0);
                live += s_pop[f];
            }
            s_new[j] = f;
        }
        for (int j = 0; j < nr; ++j) {
            b->slot_of[j] = s_new[j];
            b->rank[j] = s_rank[j];
        }
        for (int f = 0; f < n_new; ++f) b->prefix[f] = s_pre[f];
        b->n_slots = n_new;
        // the compaction rule: `matched` entries of the list carried a prefix in this pass (the sum of the block counts)
        const long long matched = b->live_n, n_cur = b->cur.n;
        const int which = b->n_compact & 1;
        int go = 0;
        if (!last && nr > 0 && n_cur >= kRsCompactMin && matched * kRsCompactDiv <= n_cur && matched <= b->cap[which]) go = 1;
        b->live_n = live;
        b->compact = go;
        if (go) {
            b->src = b->cur;
            b->cur.v = b->buf[which];
            b->cur.use = nullptr;
            b->cur.n = matched;
            b->n_compact += 1;
        }
        s_compact = go;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < ns * kRsBins; t += 256) b->hist[t] = 0ull;
    if (s_compact) {  // (block-uniform) exclusive scan of the block counts: thread t its eight pieces in order
        long long c[8], tot = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const unsigned int p = threadIdx.x * 8 + q;
            c[q] = p < nblk ? b->blkcnt[p] : 0;
            tot += c[q];
        }
        long long off = block_scan_256(tot, sw) - tot;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const unsigned int p = threadIdx.x * 8 + q;
            if (p < nblk) b->blkoff[p] = off;
            off += c[q];
        }
    }
}

// the same grid, pieces and mask as the k_rs_hist before it: block b writes the entries it counted, in order, from blkoff[b] on.  The
// slots may have parted since; their prefixes cut back to `mask` are the prefixes that pass counted.  Every write is below the new
// list's length (the sum of the counts), tested again.
__global__ void __launch_bounds__(256) k_rs_scatter(RsBlock *__restrict__ b, u64 mask) {
    __shared__ u64 s_pre[kRsMax];
    __shared__ long long s_w[4];
    if (!b->compact) return;
    const int ns = min(b->n_slots, kRsMax);
    if ((int) threadIdx.x < kRsMax) s_pre[threadIdx.x] = b->prefix[threadIdx.x] & mask;
    __syncthreads();
    const RsList L = b->src;
    double *dst = const_cast<double *>(b->cur.v);
    const long long n_dst = b->cur.n;
    long long i0, i1;
    rs_piece(L.n, gridDim.x, blockIdx.x, i0, i1);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long base = b->blkoff[blockIdx.x];
    for (long long i = i0 + threadIdx.x; i < i1 + threadIdx.x; i += 256) {  // (block-uniform trip count)
        bool m = false;
        double v = 0.0;
        if (i < i1 && (!L.use || L.use[i])) {
            v = L.v[i];
            m = rs_slot(s_pre, ns, key_of(v) & mask) >= 0;
        }
        const u64 bal = __ballot(m);
        if (lane == 0) s_w[w] = __popcll(bal);
        __syncthreads();
        long long pos = base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int q = 0; q < w; ++q) pos += s_w[q];
        if (m && pos < n_dst) dst[pos] = v + 0.0;
        base += (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) k_rs_out(RsBlock *__restrict__ b) {
    const int j = threadIdx.x;
    const long long count = b->tot.i[1];
    if (j < kRsMax) {
        double v = 0.0;
        if (j < b->n_ranks && count > 0) v = __longlong_as_double((long long) b->prefix[min(max(b->slot_of[j], 0), kRsMax - 1)]);
        b->out.value[j] = v;
    }
    if (j == 0) {
        b->out.count = count;
        b->out.sum = count > 0 ? b->tot.d[1] : 0.0;
        b->out.min = count > 0 ? __longlong_as_double(b->tot.i[kEdMn]) : 0.0;
        b->out.max = count > 0 ? __longlong_as_double(b->tot.i[kEdMx]) : 0.0;
        b->out_compact[0] = b->n_compact;
        b->out_compact[1] = b->cur.n;
    }
}

int ensure_rs(me_ctx *ctx, long long n) {
    ME_CHECK(ctx, ctx->rs_tmp[0].ensure(sizeof(RsBlock)));
    ME_CHECK(ctx, ctx->rs_tmp[1].ensure((size_t) (n / kRsCompactDiv + 1) * 8));
    ME_CHECK(ctx, ctx->rs_tmp[2].ensure((size_t) (n / (kRsCompactDiv * kRsCompactDiv) + 1) * 8));
    ME_CHECK(ctx, ctx->rs_tmp[3].ensure((size_t) std::max<long long>(n, 1)));
    ME_CHECK(ctx, ctx->red.ensure(EdRed::bytes(kEdStatBlocks)));
    return ME_OK;
}

// the fused pass: values -> use bytes (rs_tmp[3]) and the state block's counts, extremes and sums; queued on the context's stream
template <int MODE>
void stat_device(me_ctx *ctx, const double *v, const unsigned char *use_in, const SPoint *sp, long long n, const StatParams &gp, const EdThr &thr) {
    RsBlock *blk = ctx->rs_tmp[0].as<RsBlock>();
    const int nb = (int) std::min<long long>(kEdStatBlocks, blocks_of(n));
    const EdRed red(ctx, kEdStatBlocks);
    hipLaunchKernelGGL(k_ed_stat<MODE>, dim3(nb), dim3(256), 0, ctx->stream, v, use_in, sp, n, gp, thr, ctx->rs_tmp[3].as<unsigned char>(), red.pi,
                       red.pd, &blk->err);
    red.total(ctx, nb, &blk->tot);
}

// The select on n (value, use byte) pairs on the device; the state block holds the counts of stat_device and the ranks asked for
// (rank_in).  The result is left in the state block's `out`, queued on the context's stream.  The values are read in place.
int rank_select_device(me_ctx *ctx, const double *v, const unsigned char *use, long long n, int n_ranks) {
    RsBlock *blk = ctx->rs_tmp[0].as<RsBlock>();
    TimerScope ts(ctx, "rank_select");
    hipLaunchKernelGGL(k_rs_start, dim3(1), dim3(256), 0, ctx->stream, blk, v, use, n, n_ranks, ctx->rs_tmp[1].as<double>(),
                       (long long) (ctx->rs_tmp[1].bytes / 8), ctx->rs_tmp[2].as<double>(), (long long) (ctx->rs_tmp[2].bytes / 8));
    const unsigned int gx = std::min(blocks_of(n, 1024), kRsHistBlocks);
    if (n_ranks > 0)
        for (int pass = 0; pass < kRsPasses; ++pass) {
            const int shift = 64 - kRsBits * (pass + 1);
            const u64 mask = pass == 0 ? 0ull : ~0ull << (shift + kRsBits);
            const int last = pass == kRsPasses - 1;
            hipLaunchKernelGGL(k_rs_hist, dim3(gx), dim3(256), 0, ctx->stream, blk, mask, shift);
            hipLaunchKernelGGL(k_rs_narrow, dim3(1), dim3(256), 0, ctx->stream, blk, shift, gx, last);
            if (!last) hipLaunchKernelGGL(k_rs_scatter, dim3(gx), dim3(256), 0, ctx->stream, blk, mask);
        }
    hipLaunchKernelGGL(k_rs_out, dim3(1), dim3(64), 0, ctx->stream, blk);
    ts.end();
    ME_CHECK(ctx, hipGetLastError());
    return ME_OK;
}

}  // namespace

int rank_select(me_ctx *ctx, const double *values_host, const uint8_t *use_host, long long n, const int64_t *ranks, int n_ranks,
                me_rank_stats *out) {
    if (n < 0) return ctx->fail(ME_ERR_ARG, "me_rank_select: n must be >= 0");
    if (n_ranks < 0 || n_ranks > kRsMax) return ctx->fail(ME_ERR_ARG, "me_rank_select: n_ranks must be in [0, 16]");
    if (!out || (n > 0 && !values_host) || (n_ranks > 0 && !ranks)) return ctx->fail(ME_ERR_ARG, "me_rank_select: NULL argument");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    ME_TRY(ensure_rs(ctx, n));
    DevBuf &dv = ctx->tmp[2], &du = ctx->tmp[3];
    ME_CHECK(ctx, dv.ensure((size_t) n * 8));
    ME_TRY(copy_h2d(ctx, dv.p, values_host, (size_t) n * 8));
    if (use_host) {
        ME_CHECK(ctx, du.ensure((size_t) n));
        ME_TRY(copy_h2d(ctx, du.p, use_host, (size_t) n));
    }
    RsBlock *blk = ctx->rs_tmp[0].as<RsBlock>();
    ME_CHECK(ctx, hipMemsetAsync(&blk->err, 0, 8, ctx->stream));
    long long h_rank[kRsMax] = {0};
    for (int j = 0; j < n_ranks; ++j) h_rank[j] = ranks[j];
    ME_TRY(copy_h2d(ctx, blk->rank_in, h_rank, sizeof(h_rank)));
    {
        TimerScope ts(ctx, "rank_select");
        EdThr thr{};
        stat_device<1>(ctx, dv.as<double>(), use_host ? du.as<unsigned char>() : nullptr, nullptr, n, make_params(-1.0, 0, nullptr), thr);
    }
    ME_TRY(rank_select_device(ctx, dv.as<double>(), ctx->rs_tmp[3].as<unsigned char>(), n, n_ranks));
    unsigned int h_err[2] = {0, 0};
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, out, &blk->out, sizeof(me_rank_stats)));
        ME_TRY(mail_post(ctx, h_err, &blk->err, 8));
        ME_TRY(mail_post(ctx, ctx->rs_compact, blk->out_compact, 16));
        ME_TRY(mg.sync());
    }
    if (h_err[0] & 1u) return ctx->fail(ME_ERR_ARG, "me_rank_select: a used value that is negative or not finite");
    if (h_err[0] & 2u) return ctx->fail(ME_ERR_ARG, "me_rank_select: a rank outside [0, count)");
    return ME_OK;
}

int nn_error_distribution(me_ctx *ctx, int qslot, const me_errdist_params *p, me_errdist_out *out, int64_t *hist_host) {
    ME_TRY(need_single_gpu_cloud(ctx, qslot, "me_nn_error_distribution"));
    if (!p || !out) return ctx->fail(ME_ERR_ARG, "me_nn_error_distribution: NULL argument");
    if (p->gate != p->gate || (p->gate_mode != ME_GATE_LE_UNSQUARED && p->gate_mode != ME_GATE_LT_SQUARED))
        return ctx->fail(ME_ERR_ARG, "me_nn_error_distribution: bad gate or gate_mode");
    if (p->n_quantiles < 0 || p->n_quantiles > ME_RANK_MAX) return ctx->fail(ME_ERR_ARG, "me_nn_error_distribution: n_quantiles must be in [0, 16]");
    for (int j = 0; j < p->n_quantiles; ++j)
        if (!(p->prob[j] >= 0.0 && p->prob[j] <= 1.0)) return ctx->fail(ME_ERR_ARG, "me_nn_error_distribution: every prob must be in [0, 1]");
    if (p->n_thresholds < 0 || p->n_thresholds > ME_ERRDIST_MAX_THRESHOLDS)
        return ctx->fail(ME_ERR_ARG, "me_nn_error_distribution: n_thresholds must be in [0, 8]");
    for (int k = 0; k < p->n_thresholds; ++k)
        if (!(p->tau[k] >= 0.0) || p->tau[k] == INFINITY) return ctx->fail(ME_ERR_ARG, "me_nn_error_distribution: every tau must be finite and >= 0");
    if (p->n_bins < 0 || p->n_bins > kEdMaxBins) return ctx->fail(ME_ERR_ARG, "me_nn_error_distribution: n_bins must be in [0, 4096]");
    if (p->n_bins > 0 && (!(p->bin_width > 0.0) || p->bin_width == INFINITY || !hist_host))
        return ctx->fail(ME_ERR_ARG, "me_nn_error_distribution: a histogram needs bin_width > 0 and the hist array");
    Cloud &q = ctx->cloud[qslot];
    if (q.nn_ref_slot < 0) return ctx->fail(ME_ERR_STATE, "no NN result for this slot (call me_nn1 first)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = q.n;
    const int n_bins = p->n_bins;
    ME_TRY(ensure_rs(ctx, n));
    RsBlock *blk = ctx->rs_tmp[0].as<RsBlock>();
    EdThr thr{};
    thr.n = p->n_thresholds;
    for (int k = 0; k < thr.n; ++k) thr.t2[k] = sqrt_threshold(p->tau[k]);
    const double *d2 = q.nn_d2.as<double>();
    unsigned char *use = ctx->rs_tmp[3].as<unsigned char>();
    DevBuf &de = ctx->tmp[2], &dh = ctx->tmp[3];
    if (n_bins > 0) {
        std::vector<double> E((size_t) n_bins);
        for (int j = 0; j < n_bins; ++j) E[(size_t) j] = sqrt_threshold((double) (j + 1) * p->bin_width);
        ME_CHECK(ctx, de.ensure((size_t) n_bins * 8));
        ME_CHECK(ctx, dh.ensure((size_t) (n_bins + 1) * 8));
        ME_TRY(copy_h2d(ctx, de.p, E.data(), (size_t) n_bins * 8));
        ME_CHECK(ctx, hipMemsetAsync(dh.p, 0, (size_t) (n_bins + 1) * 8, ctx->stream));
    }
    {
        TimerScope ts(ctx, "errdist");
        stat_device<0>(ctx, d2, nullptr, q.sp.as<SPoint>(), n, make_params(p->gate, p->gate_mode, nullptr), thr);
        if (n_bins > 0)
            hipLaunchKernelGGL(k_ed_hist, dim3(std::min(blocks_of(n, 1024), 2048u)), dim3(256), 0, ctx->stream, d2, (const unsigned char *) use, n,
                               de.as<double>(), n_bins, dh.as<u64>());
    }
    ME_CHECK(ctx, hipGetLastError());
    EdRed::Totals h;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h, &blk->tot, sizeof(h)));
        ME_TRY(mg.sync());
    }
    const long long n_used = h.i[1];
    std::memset(out, 0, sizeof(*out));
    out->n_query = h.i[0];
    out->n_used = n_used;
    out->argmax = -1;
    auto as_double = [](long long k) {
        double v;
        std::memcpy(&v, &k, 8);
        return v;
    };
    if (n_used > 0) {
        out->sum_d = h.d[0];
        out->sum_d2 = h.d[1];
        out->min_d = std::sqrt(as_double(h.i[kEdMn]));
        out->max_d = std::sqrt(as_double(h.i[kEdMx]));
        out->argmax = h.i[kEdArg];
    }
    for (int k = 0; k < p->n_thresholds; ++k) out->n_within[k] = h.i[2 + k];
    long long h_rank[kRsMax] = {0};
    for (int j = 0; j < p->n_quantiles; ++j) {
        // nearest rank: ceil(p n) - 1, one fp64 multiplication, clamped to [0, n_used - 1]
        long long r = -1;
        if (n_used > 0) r = std::min<long long>(n_used - 1, std::max<long long>(0, (long long) std::ceil(p->prob[j] * (double) n_used) - 1));
        out->rank[j] = r;
        h_rank[j] = std::max<long long>(r, 0);
    }
    if (p->n_quantiles > 0 && n_used > 0) {
        ME_TRY(copy_h2d(ctx, blk->rank_in, h_rank, sizeof(h_rank)));
        ME_TRY(rank_select_device(ctx, d2, use, n, p->n_quantiles));
        me_rank_stats rs;
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &rs, &blk->out, sizeof(rs)));
        ME_TRY(mail_post(ctx, ctx->rs_compact, blk->out_compact, 16));
        ME_TRY(mg.sync());
        for (int j = 0; j < p->n_quantiles; ++j) {
            out->quantile_d2[j] = rs.value[j];
            out->quantile_d[j] = std::sqrt(rs.value[j]);
        }
    }
    if (n_bins > 0) {
        std::vector<long long> hh((size_t) n_bins + 1);
        ME_TRY(copy_d2h(ctx, hh.data(), dh.p, (size_t) (n_bins + 1) * 8));
        for (int j = 0; j < n_bins; ++j) hist_host[j] = hh[(size_t) j];
        out->n_overflow = hh[(size_t) n_bins];
    }
    return ME_OK;
}

void fscore_finalize(long long n_within_est, long long n_est, long long n_within_gt, long long n_gt, double prf[3]) {
    const double P = n_est > 0 ? (double) n_within_est / (double) n_est : 0.0;
    const double R = n_gt > 0 ? (double) n_within_gt / (double) n_gt : 0.0;
    prf[0] = P;
    prf[1] = R;
    prf[2] = (P + R > 0) ? 2 * P * R / (P + R) : 0.0;
}

}  // namespace me
