// me_reduce.hpp — the per-cloud result totals, once: fp64 sums, int64 counts and a (largest key, smallest original index) pair, folded
// in one fixed order.  No floating-point atomics: a total is bit-identical from run to run.
// THE ORDER.  A thread adds its own elements in increasing index (or block) order.  A block of 256 threads folds a component by
// block_sum_256: wave_sum (64-lane __shfl_down from 32 down to 1), then (sm[0] + sm[1]) + (sm[2] + sm[3]).  Partial records are added by
// one block in which thread t takes the records t, t + 256, ... and the same tree follows.
// THE PAIR.  arg < 0 means no entry; the larger key wins, on equal keys the smaller index.  That is a total order with "no entry" as
// its identity, so the result does not depend on the order of the fold; the fold is still fixed (the shuffles, then the four wave
// leaders in wave order).  The smallest key (errdist) goes the same way.
// Two layouts cover every caller:
//   one level   [blocks] records of ND doubles and NR = NI + 2 (+ 1) integers — the NI sums, the pair's key and index, then the
//               smallest key when MIN — written by red_store_partial and added by k_red_total into a RedTotals of the same layout
//   two levels  [rows][nb] words -> [rows][256] -> [rows] by k_row_sum, a row being fp64 or int64              (row_sum_device)
#pragma once

#include "me_internal.hpp"

#ifdef __HIPCC__
namespace me {

__device__ __forceinline__ void take_max(unsigned long long &mx, long long &arg, unsigned long long omx, long long oa) {
    if (oa >= 0 && (arg < 0 || omx > mx || (omx == mx && oa < arg))) mx = omx, arg = oa;
}

// the block's pair and, when MIN, its smallest key: valid in thread 0.  blockDim.x == 256.
template <bool MIN>
__device__ __forceinline__ void block_extremes_256(unsigned long long &mx, long long &arg, unsigned long long &mn) {
    __shared__ unsigned long long s_mx[4], s_mn[4];
    __shared__ long long s_arg[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long omx = (unsigned long long) __shfl_down((long long) mx, o, 64);
        const long long oa = __shfl_down(arg, o, 64);
        take_max(mx, arg, omx, oa);
        if (MIN) {
            const unsigned long long omn = (unsigned long long) __shfl_down((long long) mn, o, 64);
            mn = omn < mn ? omn : mn;
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        s_mx[w] = mx, s_arg[w] = arg;
        if (MIN) s_mn[w] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            take_max(mx, arg, s_mx[q], s_arg[q]);
            if (MIN) mn = s_mn[q] < mn ? s_mn[q] : mn;
        }
    }
}

template <int ND, int NI, bool MIN>
struct RedTotals {
    static constexpr int NR = NI + 2 + (MIN ? 1 : 0);
    double d[ND];
    long long i[NR];  // [0, NI) the sums, [NI] the pair's key, [NI + 1] its index (-1: none, key 0), [NI + 2] the smallest key
};

// every thread's sums and extremes -> the block's record (bd: ND doubles, bi: NR integers), one block_sum_256 per component in
// index order.  Called once per kernel, by all 256 threads.
template <int ND, int NI, bool MIN>
__device__ __forceinline__ void red_store_partial(const double (&sd)[ND], const long long (&ci)[NI], unsigned long long mx, long long arg,
                                                  unsigned long long mn, double *__restrict__ bd, long long *__restrict__ bi) {
    __shared__ double smd[4];
    __shared__ long long smi[4];
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        const double r = block_sum_256(sd[k], smd);
        if (threadIdx.x == 0) bd[k] = r;
    }
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const long long v = block_sum_256_ll(ci[k], smi);
        if (threadIdx.x == 0) bi[k] = v;
    }
    block_extremes_256<MIN>(mx, arg, mn);
    if (threadIdx.x == 0) {
        bi[NI] = (long long) mx;
        bi[NI + 1] = arg;
        if (MIN) bi[NI + 2] = (long long) mn;
    }
}

// one block: the nb partial records in block order
template <int ND, int NI, bool MIN>
__global__ void __launch_bounds__(256)
k_red_total(const double *__restrict__ pd, const long long *__restrict__ pi, int nb, RedTotals<ND, NI, MIN> *__restrict__ t) {
    constexpr int NR = RedTotals<ND, NI, MIN>::NR;
    double sd[ND];
    long long ci[NI];
#pragma unroll
    for (int k = 0; k < ND; ++k) sd[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NI; ++k) ci[k] = 0;
    unsigned long long mx = 0ull, mn = ~0ull;
    long long arg = -1;
    for (int q = threadIdx.x; q < nb; q += 256) {
        const double *bd = pd + (size_t) q * ND;
        const long long *bi = pi + (size_t) q * NR;
#pragma unroll
        for (int k = 0; k < ND; ++k) sd[k] += bd[k];
#pragma unroll
        for (int k = 0; k < NI; ++k) ci[k] += bi[k];
        take_max(mx, arg, (unsigned long long) bi[NI], bi[NI + 1]);
        if (MIN) mn = (unsigned long long) bi[NR - 1] < mn ? (unsigned long long) bi[NR - 1] : mn;
    }
    red_store_partial<ND, NI, MIN>(sd, ci, mx, arg, mn, t->d, t->i);
}

// HOST: ctx->red (ensured to bytes(blocks) by the caller) as [blocks][ND] doubles | [blocks][NR] integers | the totals
template <int ND, int NI, bool MIN = false>
struct RedBufs {
    typedef RedTotals<ND, NI, MIN> Totals;
    static size_t bytes(unsigned int blocks) { return (size_t) blocks * (ND + Totals::NR) * 8 + sizeof(Totals); }
    double *pd;
    long long *pi;
    Totals *tot;
    RedBufs(me_ctx *ctx, unsigned int blocks)
        : pd(ctx->red.as<double>()), pi(reinterpret_cast<long long *>(pd + (size_t) blocks * ND)),
          tot(reinterpret_cast<Totals *>(pi + (size_t) blocks * Totals::NR)) {}
    // the nb records written by the kernel before -> `to` (device), queued on the context's stream
    void total(me_ctx *ctx, int nb, Totals *to) const {
        hipLaunchKernelGGL((k_red_total<ND, NI, MIN>), dim3(1), dim3(256), 0, ctx->stream, (const double *) pd, (const long long *) pi, nb, to);
    }
};

// ---- two levels: rows of block partials ----
constexpr int kRowStage = 256;  // chunks of the first level; part of the order

union RedWord {
    double d;
    long long i;
};

// row v of `in` ([rows][nb]) -> out[v * gridDim.x + block]: block b sums the chunk [b chunk, (b + 1) chunk) of the row, thread t taking
// t, t + 256, ... in order.  Bit v of INT_ROWS: the row holds int64.  (A template argument, so that each file has a kernel of its own.)
template <unsigned long long INT_ROWS>
__global__ void __launch_bounds__(256)
k_row_sum(const RedWord *__restrict__ in, long long nb, long long chunk, int rows, RedWord *__restrict__ out) {
    __shared__ double smd[4];
    __shared__ long long smi[4];
    const long long b0 = (long long) blockIdx.x * chunk, b1 = b0 + chunk < nb ? b0 + chunk : nb;
    for (int v = 0; v < rows; ++v) {
        const RedWord *row = in + (size_t) v * nb;
        RedWord r;
        if (!((INT_ROWS >> v) & 1ull)) {
            double s = 0.0;
            for (long long b = b0 + threadIdx.x; b < b1; b += 256) s += row[b].d;
            r.d = block_sum_256(s, smd);
        } else {
            long long s = 0;
            for (long long b = b0 + threadIdx.x; b < b1; b += 256) s += row[b].i;
            r.i = block_sum_256_ll(s, smi);
        }
        if (threadIdx.x == 0) out[(size_t) v * gridDim.x + blockIdx.x] = r;
    }
}

// HOST: ctx->red (ensured to row_sum_bytes by the caller) as [rows][nb] block partials | [rows][kRowStage] | [rows] totals
inline size_t row_sum_bytes(int rows, unsigned int nb) { return ((size_t) nb + kRowStage + 1) * (size_t) rows * 8; }
inline RedWord *row_sum_part(me_ctx *ctx) { return ctx->red.as<RedWord>(); }
// the two launches over the partials, queued on the context's stream; the totals go to `out` (device) or, when nullptr, to the tail of
// ctx->red.  Returns where they are.  rows <= 64.
template <unsigned long long INT_ROWS>
inline RedWord *row_sum_device(me_ctx *ctx, int rows, unsigned int nb, RedWord *out = nullptr) {
    const RedWord *part = row_sum_part(ctx);
    RedWord *stage = row_sum_part(ctx) + (size_t) nb * rows;
    if (!out) out = stage + (size_t) kRowStage * rows;
    const long long chunk = ((long long) nb + kRowStage - 1) / kRowStage;
    hipLaunchKernelGGL(k_row_sum<INT_ROWS>, dim3(kRowStage), dim3(256), 0, ctx->stream, part, (long long) nb, chunk, rows, stage);
    hipLaunchKernelGGL(k_row_sum<INT_ROWS>, dim3(1), dim3(256), 0, ctx->stream, (const RedWord *) stage, (long long) kRowStage,
                       (long long) kRowStage, rows, out);
    return out;
}

}  // namespace me
#endif
