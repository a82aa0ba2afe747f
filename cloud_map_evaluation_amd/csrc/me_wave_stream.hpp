// me_wave_stream.hpp — the neighbourhood stream of the per-point kernels over a cloud's own cell table (me_outlier.hip, me_cluster.hip).
#pragma once

#include "me_internal.hpp"

#ifdef __HIPCC__
namespace me {

// One wave's sorted queries against the cell table g: groups of lanes (wave_group_table, Chebyshev 2 around a leader) stream every
// run of their box through a wave-private LDS tile ONCE; every lane of the round's group calls f(px, py, pz, pos, j) on each
// candidate: pos = its sorted position, j = its place in the tile (0 .. 63).  The box of a group holds every lane's own 3x3x3 block.
// stage(j, pos) is called by lane j when it puts the candidate at pos into the tile: a kernel that needs a per-candidate word next to
// the coordinates writes it to an LDS array of its own there and reads it in f at [j].
struct WaveTile {
    double x[64], y[64], z[64];
};
template <class S, class F>
__device__ __forceinline__ void wave_stream_staged(bool pending, int cx, int cy, int cz, const SPoint *__restrict__ sp, const GridView &g,
                                                   int lane, int2 *tab, WaveTile *tile, S &&stage, F &&f) {
    const int cell_lim = 1 << (kMortonBits - g.shift);
    bool done = !pending;
    while (__ballot(!done)) {
        GroupBox bx;
        int nk = 0;
        const bool in = wave_group_table<1>(!done, cx, cy, cz, g, cell_lim, lane, tab, bx, &nk);
        wave_for_each_run<true>(tab, nk, lane, [&](int b, int e, int) {
            for (int base = b; base < e; base += 64) {
                const int m = min(64, e - base);  // wave-uniform
                if (lane < m) {
                    const SPoint p = sp[base + lane];
                    tile->x[lane] = p.x;
                    tile->y[lane] = p.y;
                    tile->z[lane] = p.z;
                    stage(lane, base + lane);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (in)
                    for (int j = 0; j < m; ++j) f(tile->x[j], tile->y[j], tile->z[j], base + j, j);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();  // the tile is overwritten by the next chunk
            }
        });
        if (in) done = true;
    }
}
template <class F>
__device__ __forceinline__ void wave_stream(bool pending, int cx, int cy, int cz, const SPoint *__restrict__ sp, const GridView &g,
                                            int lane, int2 *tab, WaveTile *tile, F &&f) {
    wave_stream_staged(pending, cx, cy, cz, sp, g, lane, tab, tile, [](int, int) {}, f);
}

__device__ __forceinline__ void cell_of(unsigned long long code, int shift, int &cx, int &cy, int &cz) {
    const unsigned long long c = code >> (3 * shift);
    cx = (int) compact21(c);
    cy = (int) compact21(c >> 1);
    cz = (int) compact21(c >> 2);
}

// The query of one lane of a wave_stream kernel: the sorted point i (inactive past the end: zeros, and the stream skips the lane), its
// original index and its cell at the grid's shift.
struct StreamQuery {
    bool active;
    double qx, qy, qz;
    long long idx;
    int cx, cy, cz;
};
__device__ __forceinline__ StreamQuery stream_query(const SPoint *__restrict__ sp, const unsigned long long *__restrict__ codes, long long i,
                                                    long long n, int shift) {
    StreamQuery q{i < n, 0, 0, 0, 0, 0, 0, 0};
    if (q.active) {
        const SPoint p = sp[i];
        q.qx = p.x;
        q.qy = p.y;
        q.qz = p.z;
        q.idx = p.idx;
        cell_of(codes[i], shift, q.cx, q.cy, q.cz);
    }
    return q;
}

}  // namespace me
#endif
