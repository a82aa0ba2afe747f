// me_oct_walk.hpp — the stackless nearest-first walk of the sparse octree (OctView), one lane per query: box bound, the "children
// already entered" masks (me_reg.hip, me_outlier.hip) and the walk itself as a function (me_outlier.hip).
#pragma once

#include "me_internal.hpp"

#ifdef __HIPCC__
namespace me {

// squared distance from q to a node's box: never exceeds the computed d2 of a point inside (boxes rounded outward)
__device__ __forceinline__ double box_lb(const ONode *__restrict__ nd, double qx, double qy, double qz) {
    const double dx = fmax(fmax((double) nd->lo[0] - qx, qx - (double) nd->hi[0]), 0.0);
    const double dy = fmax(fmax((double) nd->lo[1] - qy, qy - (double) nd->hi[1]), 0.0);
    const double dz = fmax(fmax((double) nd->lo[2] - qz, qz - (double) nd->hi[2]), 0.0);
    return (dx * dx + dy * dy) + dz * dz;
}

// One byte of "children already entered" per level of the path from the root: levels 1..8 in lo, 9..16 in hi (level 0 = the leaves).
static_assert(kMaxLevels == 17, "the taken masks hold one byte for each of the levels 1..16");
struct OctTaken {
    unsigned long long lo = 0, hi = 0;
};
__device__ __forceinline__ unsigned int taken_get(const OctTaken &t, int l) {
    return (l <= 8) ? (unsigned int) (t.lo >> (8 * (l - 1))) & 0xffu : (unsigned int) (t.hi >> (8 * (l - 9))) & 0xffu;
}
__device__ __forceinline__ void taken_set(OctTaken &t, int l, int kc) {
    if (l <= 8) t.lo |= 1ULL << (8 * (l - 1) + kc);
    else t.hi |= 1ULL << (8 * (l - 9) + kc);
}
__device__ __forceinline__ void taken_clear(OctTaken &t, int l) {
    if (l <= 8) t.lo &= ~(0xffULL << (8 * (l - 1)));
    else t.hi &= ~(0xffULL << (8 * (l - 9)));
}

// From the root (level L) always into the nearest child not yet entered whose box bound lb passes admit(lb); back to the parent when
// a node has none left; scan_leaf(index into nodes) for every leaf reached.  admit reads the caller's current bound each time it is
// called: a scan tightens it.  s_off = OctView::off in LDS (the caller loads it, and owns the barrier after the load).
template <class Admit, class Scan>
__device__ __forceinline__ void oct_walk_nearest(const ONode *__restrict__ nodes, const long long *s_off, int L, double qx, double qy,
                                                 double qz, Admit &&admit, Scan &&scan_leaf) {
    int l = L;
    long long nd = 0;
    OctTaken taken;
    for (;;) {
        long long leaf = 0;  // (a tree of one level: leaf 0 is all there is)
        if (L != 0) {
            const ONode *__restrict__ me = nodes + s_off[l] + nd;
            const long long cb = me[0].begin;
            const int cc = (int) (me[1].begin - cb);
            const unsigned int tk = taken_get(taken, l);
            double kd = INFINITY;
            int kc = 8;
            const ONode *__restrict__ ch = nodes + s_off[l - 1] + cb;
            for (int c = 0; c < cc; ++c) {
                if ((tk >> c) & 1u) continue;
                const double lb = box_lb(ch + c, qx, qy, qz);
                if (admit(lb) && lb < kd) {
                    kd = lb;
                    kc = c;
                }
            }
            if (kc >= 8) {
                if (l == L) break;
                nd = me[0].parent;
                ++l;
                continue;
            }
            taken_set(taken, l, kc);
            if (l != 1) {
                --l;
                nd = cb + kc;
                taken_clear(taken, l);
                continue;
            }
            leaf = s_off[0] + cb + kc;
        }
        scan_leaf(leaf);
        if (L == 0) break;
    }
}

}  // namespace me
#endif
