// me_mesh.hip — a resident triangle mesh beside the two clouds: the exact distance from every point of a cloud to the mesh
// (CloudCompare's cloud-to-mesh distance) and an area-uniform sample of the mesh into a cloud slot.  Definitions: include/mapeval_hip.h,
// DESIGN.md section 4.18.
//   mesh_upload    HOST: the optional transform (k_transform's arithmetic), validation of the referenced vertices, the per-triangle area
//                  and the cumulative area table in the caller's order, the degenerate flags — this file is compiled with
//                  -ffp-contract=off, so the host arithmetic is the one numpy restates.  DEVICE: k_mesh_codes (Morton code of the
//                  centroid), the library's radix sort, k_mesh_gather (sorted triangles + caller index), k_mesh_leaves (one box per 8
//                  consecutive sorted triangles), k_mesh_up once per level (union of 8 children), all queued without a host round trip
//   k_mesh_dist    one query per lane, in the cloud's sorted order.  The implicit 8-ary tree is walked nearest child first without a
//                  stack: the path is the node index itself (parent = j >> 3) and one byte per level marks the children already taken.
//                  A child is opened iff its box distance <= bound(best), see mesh_bound; a leaf runs tri_closest on its <= 8 triangles.
//                  The winner is the lexicographic minimum of (d2, caller index): independent of the order of the walk.
//   k_mesh_final   the gate, the sums and counts; the block's partial record and the one-block total over the records are
//                  me_reduce.hpp's
//   k_mesh_unpermute  the per-point results back in cloud order                                              (me_mesh_distance_fetch)
//   k_mesh_sample  Philox4x64-10 at counter (i, 0, 0, 0): triangle by binary search in the cumulative areas, point by the square-root
//                  parametrisation; written into the slot's own buffer, then the normal cloud_finish
// tests/_mesh_ref.py restates tri_closest, the sampler and the area order operation by operation.
#include <cmath>
#include <cstring>
#include <vector>

#include "me_internal.hpp"
#include "me_philox.hpp"
#include "me_reduce.hpp"

namespace me {

namespace {

constexpr unsigned int kMdBlocks = 1024;
constexpr int kMdD = 4;    // double sums per block: sum_d, sum_d2, sum_signed, sum_abs_signed
constexpr int kMdNI = 2 + ME_MESH_MAX_THRESHOLDS;  // integer sums: n_matched, n_face, n_within[8]; then max key, argmax
typedef RedBufs<kMdD, kMdNI> MdRed;
constexpr unsigned int kDegBit = 0x80000000u;  // in the stored caller index: the triangle is degenerate

struct MdGate {
    double max2;  // max_distance * max_distance
    double t2[ME_MESH_MAX_THRESHOLDS];
    int nt;
};

// ---- the point-triangle routine: ONE sequence of fp64 operations (tests/_mesh_ref.py restates it) ----
#define ME_HD __device__ __forceinline__
ME_HD double md_dot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }
ME_HD double md_clamp01(double v) { return fmin(fmax(v, 0.0), 1.0); }  // (fmax(NaN, 0) = 0: a 0/0 lands on the first end point)

// closest point of the segment P0 P1: the end points where the projection leaves the segment, else P0 + (t / l) e
ME_HD void seg_closest(double px, double py, double pz, double x0, double y0, double z0, double x1, double y1, double z1, int code_edge,
                       int code0, int code1, double &cx, double &cy, double &cz, int &region) {
    const double ex = x1 - x0, ey = y1 - y0, ez = z1 - z0;
    const double l = md_dot(ex, ey, ez, ex, ey, ez);
    const double t = md_dot(ex, ey, ez, px - x0, py - y0, pz - z0);
    if (t <= 0.0) {
        cx = x0, cy = y0, cz = z0, region = code0;
    } else if (t >= l) {
        cx = x1, cy = y1, cz = z1, region = code1;
    } else {
        const double s = t / l;
        cx = x0 + s * ex, cy = y0 + s * ey, cz = z0 + s * ez, region = code_edge;
    }
}

// region codes: 0 face, 1 edge AB, 2 edge BC, 3 edge CA, 4 vertex A, 5 vertex B, 6 vertex C
ME_HD double tri_closest(double px, double py, double pz, const double *__restrict__ v, bool degenerate, double &cx, double &cy, double &cz,
                         int &region) {
    const double ax = v[0], ay = v[1], az = v[2], bx = v[3], by = v[4], bz = v[5], gx = v[6], gy = v[7], gz = v[8];
    if (degenerate) {  // the three segments AB, BC, CA in this order; a later one wins only when strictly nearer
        seg_closest(px, py, pz, ax, ay, az, bx, by, bz, 1, 4, 5, cx, cy, cz, region);
        double dx = px - cx, dy = py - cy, dz = pz - cz;
        double best = (dx * dx + dy * dy) + dz * dz;
        double qx, qy, qz;
        int r;
        seg_closest(px, py, pz, bx, by, bz, gx, gy, gz, 2, 5, 6, qx, qy, qz, r);
        dx = px - qx, dy = py - qy, dz = pz - qz;
        double d = (dx * dx + dy * dy) + dz * dz;
        if (d < best) best = d, cx = qx, cy = qy, cz = qz, region = r;
        seg_closest(px, py, pz, gx, gy, gz, ax, ay, az, 3, 6, 4, qx, qy, qz, r);
        dx = px - qx, dy = py - qy, dz = pz - qz;
        d = (dx * dx + dy * dy) + dz * dz;
        if (d < best) best = d, cx = qx, cy = qy, cz = qz, region = r;
        return best;
    }
    const double abx = bx - ax, aby = by - ay, abz = bz - az;
    const double acx = gx - ax, acy = gy - ay, acz = gz - az;
    const double d1 = md_dot(abx, aby, abz, px - ax, py - ay, pz - az), d2 = md_dot(acx, acy, acz, px - ax, py - ay, pz - az);
    const double d3 = md_dot(abx, aby, abz, px - bx, py - by, pz - bz), d4 = md_dot(acx, acy, acz, px - bx, py - by, pz - bz);
    const double d5 = md_dot(abx, aby, abz, px - gx, py - gy, pz - gz), d6 = md_dot(acx, acy, acz, px - gx, py - gy, pz - gz);
    if (d1 <= 0.0 && d2 <= 0.0) {
        cx = ax, cy = ay, cz = az, region = 4;
    } else if (d3 >= 0.0 && d4 <= d3) {
        cx = bx, cy = by, cz = bz, region = 5;
    } else if (d1 * d4 - d3 * d2 <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double t = md_clamp01(d1 / (d1 - d3));
        cx = ax + t * abx, cy = ay + t * aby, cz = az + t * abz, region = 1;
    } else if (d6 >= 0.0 && d5 <= d6) {
        cx = gx, cy = gy, cz = gz, region = 6;
    } else if (d5 * d2 - d1 * d6 <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double t = md_clamp01(d2 / (d2 - d6));
        cx = ax + t * acx, cy = ay + t * acy, cz = az + t * acz, region = 3;
    } else if (d3 * d6 - d5 * d4 <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double t = md_clamp01((d4 - d3) / ((d4 - d3) + (d5 - d6)));
        cx = bx + t * (gx - bx), cy = by + t * (gy - by), cz = bz + t * (gz - bz), region = 2;
    } else {
        const double va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
        const double den = (va + vb) + vc;
        const double s = md_clamp01(vb / den);
        const double t = fmin(fmax(vc / den, 0.0), 1.0 - s);
        cx = (ax + s * abx) + t * acx, cy = (ay + s * aby) + t * acy, cz = (az + s * abz) + t * acz, region = 0;
    }
    const double dx = px - cx, dy = py - cy, dz = pz - cz;
    return (dx * dx + dy * dy) + dz * dz;
}

// the prune bound of a best distance: a box is skipped iff its computed distance is ABOVE this (DESIGN.md 4.18 "Pruning")
__device__ __forceinline__ double mesh_bound(double best, double delta) {
    const double s = sqrt(best) + delta;
    return (s * s) * (1.0 + 0x1p-46);
}

__device__ __forceinline__ double box_d2(const double *__restrict__ b, double px, double py, double pz) {
    const double ex = fmax(fmax(b[0] - px, px - b[3]), 0.0), ey = fmax(fmax(b[1] - py, py - b[4]), 0.0),
                 ez = fmax(fmax(b[2] - pz, pz - b[5]), 0.0);
    return (ex * ex + ey * ey) + ez * ez;
}

struct MeshView {
    const double *tri;         // [nt][9] sorted triangles
    const unsigned int *orig;  // [nt] caller index | kDegBit
    const double *boxes;       // [nodes][6] lo xyz, hi xyz; level l at lv[l].x
    const int2 *lv;            // per level: offset into boxes, node count
    long long nt;
    int n_levels;
    double delta;
};

__global__ void __launch_bounds__(256) k_mesh_codes(const double *__restrict__ tri, long long nt, double ox, double oy, double oz, double h,
                                                    unsigned long long *__restrict__ codes, unsigned int *__restrict__ iota) {
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const double *v = tri + 9 * t;
    const double c[3] = {((v[0] + v[3]) + v[6]) / 3.0, ((v[1] + v[4]) + v[7]) / 3.0, ((v[2] + v[5]) + v[8]) / 3.0};
    const double o[3] = {ox, oy, oz};
    unsigned long long g[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) g[d] = (unsigned long long) fmin(fmax(floor((c[d] - o[d]) / h), 0.0), 2097151.0);
    codes[t] = spread21(g[0]) | (spread21(g[1]) << 1) | (spread21(g[2]) << 2);
    iota[t] = (unsigned int) t;
}

__global__ void __launch_bounds__(256) k_mesh_gather(const double *__restrict__ tri_in, const unsigned char *__restrict__ deg,
                                                     const unsigned int *__restrict__ perm, long long nt, double *__restrict__ tri_s,
                                                     unsigned int *__restrict__ orig) {
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const unsigned int o = perm[t];  // a permutation of [0, nt)
#pragma unroll
    for (int k = 0; k < 9; ++k) tri_s[9 * t + k] = tri_in[9 * (long long) o + k];
    orig[t] = o | (deg[o] ? kDegBit : 0u);
}

__global__ void __launch_bounds__(256) k_mesh_leaves(const double *__restrict__ tri_s, long long nt, int n_leaves, double *__restrict__ boxes) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_leaves) return;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const long long t1 = min((long long) j * 8 + 8, nt);
    for (long long t = (long long) j * 8; t < t1; ++t)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double x = tri_s[9 * t + k];
            lo[k % 3] = fmin(lo[k % 3], x);
            hi[k % 3] = fmax(hi[k % 3], x);
        }
#pragma unroll
    for (int d = 0; d < 3; ++d) boxes[6 * (long long) j + d] = lo[d], boxes[6 * (long long) j + 3 + d] = hi[d];
}

__global__ void __launch_bounds__(256) k_mesh_up(const double *__restrict__ child, int n_child, int n_parent, double *__restrict__ parent) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_parent) return;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int c1 = min(j * 8 + 8, n_child);
    for (int c = j * 8; c < c1; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fmin(lo[d], child[6 * (long long) c + d]);
            hi[d] = fmax(hi[d], child[6 * (long long) c + 3 + d]);
        }
#pragma unroll
    for (int d = 0; d < 3; ++d) parent[6 * (long long) j + d] = lo[d], parent[6 * (long long) j + 3 + d] = hi[d];
}

// the taken-children byte of level l (1 ..): levels 1-8 in `a`, 9-16 in `b`
__device__ __forceinline__ unsigned int taken_get(unsigned long long a, unsigned long long b, int l) {
    const int s = 8 * (l - 1);
    return (unsigned int) ((s < 64 ? a >> s : b >> (s - 64)) & 0xffull);
}
__device__ __forceinline__ void taken_set(unsigned long long &a, unsigned long long &b, int l, unsigned int v) {
    const int s = 8 * (l - 1);
    if (s < 64) a = (a & ~(0xffull << s)) | ((unsigned long long) v << s);
    else b = (b & ~(0xffull << (s - 64))) | ((unsigned long long) v << (s - 64));
}

// sp / n: the query cloud's sorted points.  Results in SORTED order: d2[n], tri[n] (caller index), reg[n], cp[3][n], sd[n] (NaN off the face).
__global__ void __launch_bounds__(256)
k_mesh_dist(const SPoint *__restrict__ sp, long long n, MeshView m, double *__restrict__ d2_s, int *__restrict__ tri_out,
            unsigned char *__restrict__ reg_s, double *__restrict__ cp_s, double *__restrict__ sd_s) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double px = sp[i].x, py = sp[i].y, pz = sp[i].z;
    double best = INFINITY, bound = INFINITY;
    unsigned int best_o = 0xffffffffu;
    long long best_t = 0;
    int level = m.n_levels - 1;
    long long j = 0;
    unsigned long long ta = 0, tb = 0;
    for (;;) {
        if (level == 0) {
            const long long t1 = min(j * 8 + 8, m.nt);
            for (long long t = j * 8; t < t1; ++t) {
                const unsigned int og = m.orig[t], o = og & ~kDegBit;
                double cx, cy, cz;
                int r;
                const double d = tri_closest(px, py, pz, m.tri + 9 * t, (og & kDegBit) != 0, cx, cy, cz, r);
                if (d < best || (d == best && o < best_o)) {
                    if (d < best) bound = mesh_bound(d, m.delta);
                    best = d, best_o = o, best_t = t;
                }
            }
            if (m.n_levels == 1) break;
            level = 1;
            j >>= 3;
            continue;
        }
        const int2 cl = m.lv[level - 1];
        const int nch = (int) min(8ll, (long long) cl.y - j * 8);
        const unsigned int taken = taken_get(ta, tb, level);
        const double *cb = m.boxes + 6 * ((long long) cl.x + j * 8);
        double bb = INFINITY;
        int bc = -1;
        for (int c = 0; c < nch; ++c) {
            if ((taken >> c) & 1u) continue;
            const double b = box_d2(cb + 6 * c, px, py, pz);
            if (bc < 0 || b < bb) bb = b, bc = c;
        }
        if (bc < 0 || bb > bound) {  // (the nearest remaining child is out: so is every other)
            if (level == m.n_levels - 1) break;
            taken_set(ta, tb, level, 0u);
            ++level;
            j >>= 3;
            continue;
        }
        taken_set(ta, tb, level, taken | (1u << bc));
        j = j * 8 + bc;
        --level;
    }
    // the winner once more, for the closest point, the region and the sign
    const double *v = m.tri + 9 * best_t;
    double cx, cy, cz;
    int r;
    const double d = tri_closest(px, py, pz, v, (m.orig[best_t] & kDegBit) != 0, cx, cy, cz, r);
    double sd = NAN;
    if (r == 0) {
        const double ab[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, ac[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
        double nn[3];
        cross3(ab, ac, nn);
        const double e[3] = {px - cx, py - cy, pz - cz};
        sd = dot3(e, nn) / sqrt(dot3(nn, nn));
    }
    d2_s[i] = d;
    tri_out[i] = (int) best_o;
    reg_s[i] = (unsigned char) r;
    cp_s[i] = cx, cp_s[n + i] = cy, cp_s[2 * n + i] = cz;
    sd_s[i] = sd;
}

__global__ void __launch_bounds__(256)
k_mesh_final(const SPoint *__restrict__ sp, long long n, const double *__restrict__ d2_s, const unsigned char *__restrict__ reg_s,
             const double *__restrict__ sd_s, MdGate g, double *__restrict__ pd, long long *__restrict__ pi) {
    long long arg = -1, ci[kMdNI];  // n_matched, n_face, n_within[8]
#pragma unroll
    for (int k = 0; k < kMdNI; ++k) ci[k] = 0;
    unsigned long long mx = 0ull;
    double sd[kMdD] = {0.0, 0.0, 0.0, 0.0};  // sum_d, sum_d2, sum_signed, sum_abs_signed
    const long long stride = (long long) gridDim.x * 256;
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const double d2 = d2_s[i];
        if (!(d2 <= g.max2)) continue;
        const double d = sqrt(d2);
        ci[0] += 1;
        sd[0] += d;
        sd[1] += d2;
#pragma unroll
        for (int k = 0; k < ME_MESH_MAX_THRESHOLDS; ++k)
            if (k < g.nt && d2 <= g.t2[k]) ci[2 + k] += 1;
        if (reg_s[i] == 0) {
            const double s = sd_s[i];
            ci[1] += 1;
            sd[2] += s;
            sd[3] += fabs(s);
        }
        take_max(mx, arg, (unsigned long long) __double_as_longlong(d), sp[i].idx);  // (d >= +0.0: bit order = numeric order)
    }
    red_store_partial<kMdD, kMdNI, false>(sd, ci, mx, arg, 0ull, pd + (size_t) blockIdx.x * kMdD, pi + (size_t) blockIdx.x * MdRed::Totals::NR);
}

// every output is nullable
__global__ void __launch_bounds__(256)
k_mesh_unpermute(const SPoint *__restrict__ sp, long long n, const double *__restrict__ d2_s, const int *__restrict__ tri_s,
                 const unsigned char *__restrict__ reg_s, const double *__restrict__ cp_s, const double *__restrict__ sd_s,
                 double *__restrict__ d2, int *__restrict__ tri, unsigned char *__restrict__ reg, double *__restrict__ cp,
                 double *__restrict__ sd) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long o = sp[i].idx;  // a permutation of [0, n)
    if (d2) d2[o] = d2_s[i];
    if (tri) tri[o] = tri_s[i];
    if (reg) reg[o] = reg_s[i];
    if (cp) cp[3 * o] = cp_s[i], cp[3 * o + 1] = cp_s[n + i], cp[3 * o + 2] = cp_s[2 * n + i];
    if (sd) sd[o] = sd_s[i];
}

// tri_in / cum in the CALLER's order; cum[nt - 1] = total
__global__ void __launch_bounds__(256) k_mesh_sample(const double *__restrict__ tri_in, const double *__restrict__ cum, long long nt,
                                                     double total, unsigned long long seed, long long n, double *__restrict__ xyz) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u64 w[4];
    philox_block(seed, (u64) i, 0, 0, w);
    const double u = u01(w[0]) * total;
    long long lo = 0, hi = nt - 1;  // the first index whose cumulative area exceeds u (the last one if rounding left none)
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (cum[mid] > u) hi = mid;
        else lo = mid + 1;
    }
    const double *v = tri_in + 9 * lo;
    const double r1 = sqrt(u01(w[1])), r2 = u01(w[2]);
    const double wa = 1.0 - r1, wb = r1 * (1.0 - r2), wc = r1 * r2;
#pragma unroll
    for (int d = 0; d < 3; ++d) xyz[3 * i + d] = (wa * v[d] + wb * v[3 + d]) + wc * v[6 + d];
}

void mesh_drop_results(me_ctx *ctx) {
    ctx->cloud[0].mesh_have = false;
    ctx->cloud[1].mesh_have = false;
    ctx->cloud[0].mesh_sign_have = false;
    ctx->cloud[1].mesh_sign_have = false;
    ctx->cloud[0].vis_have = false;  // (the visibility of a slot's points was cast against this mesh: me_ray.hip)
    ctx->cloud[1].vis_have = false;
    ctx->mesh->topo_have = false;  // (the topology and the pseudo-normals go with the mesh they were built from: me_meshsign.hip)
}

}  // namespace

int mesh_upload(me_ctx *ctx, const double *vertices, long long nv, const int32_t *triangles, long long nt, const double *T) {
    if (!vertices || !triangles) return ctx->fail(ME_ERR_ARG, "me_mesh_upload: NULL argument");
    if (nt < 1) return ctx->fail(ME_ERR_ARG, "me_mesh_upload: n_triangles must be >= 1");
    if (nv < 1 || nt >= (1LL << 31) || nv >= (1LL << 31))
        return ctx->fail(ME_ERR_ARG, "me_mesh_upload: needs 1 <= n_vertices < 2^31 and n_triangles < 2^31");
    for (long long k = 0; k < 3 * nt; ++k)
        if (triangles[k] < 0 || triangles[k] >= nv) return ctx->fail(ME_ERR_ARG, "me_mesh_upload: a vertex index is outside [0, n_vertices)");
    if (T) {
        bool identity = true;
        for (int i = 0; i < 16; ++i) identity = identity && T[i] == ((i % 5 == 0) ? 1.0 : 0.0);
        if (identity) T = nullptr;
    }
    // the triangles' corner coordinates in the caller's order; the transform is Open3D's PointCloud::Transform as k_transform applies it
    std::vector<double> tri((size_t) nt * 9), cum((size_t) nt);
    std::vector<unsigned char> deg((size_t) nt);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, max_abs = 0.0, total = 0.0;
    long long n_deg = 0;
    for (long long t = 0; t < nt; ++t) {
        double *v = &tri[(size_t) t * 9];
        for (int c = 0; c < 3; ++c) {
            const double *s = vertices + 3 * (long long) triangles[3 * t + c];
            double p[3] = {s[0], s[1], s[2]};
            if (T) {
                double h[4];
                for (int r = 0; r < 4; ++r) h[r] = ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3];
                p[0] = h[0] / h[3], p[1] = h[1] / h[3], p[2] = h[2] / h[3];
            }
            for (int d = 0; d < 3; ++d) {
                if (!std::isfinite(p[d])) return ctx->fail(ME_ERR_ARG, "me_mesh_upload: a referenced vertex has a non-finite coordinate");
                v[3 * c + d] = p[d];
                lo[d] = std::fmin(lo[d], p[d]);
                hi[d] = std::fmax(hi[d], p[d]);
                max_abs = std::fmax(max_abs, std::fabs(p[d]));
            }
        }
        // area = 0.5 * sqrt((nx*nx + ny*ny) + nz*nz), n = (B - A) x (C - A); degenerate iff n is exactly the zero vector
        const double ab[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, ac[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
        const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
        deg[(size_t) t] = nx == 0.0 && ny == 0.0 && nz == 0.0;
        n_deg += deg[(size_t) t];
        total += 0.5 * std::sqrt((nx * nx + ny * ny) + nz * nz);
        cum[(size_t) t] = total;
    }
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    Mesh &m = *ctx->mesh;
    m.have = false;
    mesh_drop_results(ctx);
    // levels: leaves of 8 consecutive sorted triangles, then unions of 8, up to one root
    int L = 0;
    long long off = 0;
    for (long long c = (nt + 7) / 8;; c = (c + 7) / 8) {
        m.lv_off[L] = (int) off, m.lv_cnt[L] = (int) c;
        off += c;
        ++L;
        if (c == 1) break;
    }
    ME_CHECK(ctx, m.tri_in.ensure((size_t) nt * 72));
    ME_CHECK(ctx, m.tri_s.ensure((size_t) nt * 72));
    ME_CHECK(ctx, m.orig.ensure((size_t) nt * 4));
    ME_CHECK(ctx, m.cum.ensure((size_t) nt * 8));
    ME_CHECK(ctx, m.idx.ensure((size_t) nt * 12));
    ME_CHECK(ctx, m.boxes.ensure((size_t) off * 48));
    ME_CHECK(ctx, m.lv.ensure(sizeof(int2) * kMeshMaxLevels));
    int2 lv[kMeshMaxLevels] = {};
    for (int l = 0; l < L; ++l) lv[l] = make_int2(m.lv_off[l], m.lv_cnt[l]);
    DevBuf &codes_in = ctx->tmp[0], &iota = ctx->tmp[1], &perm = ctx->tmp[2], &codes_out = ctx->tmp[3], &degd = ctx->tmp[4];
    ME_CHECK(ctx, codes_in.ensure((size_t) nt * 8));
    ME_CHECK(ctx, codes_out.ensure((size_t) nt * 8));
    ME_CHECK(ctx, iota.ensure((size_t) nt * 4));
    ME_CHECK(ctx, perm.ensure((size_t) nt * 4));
    ME_CHECK(ctx, degd.ensure((size_t) nt));
    ME_TRY(copy_h2d(ctx, m.tri_in.p, tri.data(), (size_t) nt * 72));
    ME_TRY(copy_h2d(ctx, m.cum.p, cum.data(), (size_t) nt * 8));
    ME_TRY(copy_h2d(ctx, m.idx.p, triangles, (size_t) nt * 12));
    ME_TRY(copy_h2d(ctx, degd.p, deg.data(), (size_t) nt));
    ME_TRY(copy_h2d(ctx, m.lv.p, lv, sizeof(lv)));
    double extent = 0.0;
    for (int d = 0; d < 3; ++d) extent = std::fmax(extent, hi[d] - lo[d]);
    const double h = extent > 0 ? std::ldexp(extent, -kMortonBits) * (1.0 + 0x1p-20) : 1.0;
    {
        TimerScope ts(ctx, "mesh_index");
        hipLaunchKernelGGL(k_mesh_codes, dim3(blocks_of(nt)), dim3(256), 0, ctx->stream, m.tri_in.as<double>(), nt, lo[0], lo[1], lo[2], h,
                           codes_in.as<unsigned long long>(), iota.as<unsigned int>());
    }
    ME_TRY(sort_pairs_u64_u32(ctx, codes_in.as<unsigned long long>(), codes_out.as<unsigned long long>(), iota.as<unsigned int>(),
                              perm.as<unsigned int>(), nt, 0, 3 * kMortonBits));
    {
        TimerScope ts(ctx, "mesh_index");
        hipLaunchKernelGGL(k_mesh_gather, dim3(blocks_of(nt)), dim3(256), 0, ctx->stream, m.tri_in.as<double>(), degd.as<unsigned char>(),
                           perm.as<unsigned int>(), nt, m.tri_s.as<double>(), m.orig.as<unsigned int>());
        hipLaunchKernelGGL(k_mesh_leaves, dim3(blocks_of(m.lv_cnt[0])), dim3(256), 0, ctx->stream, m.tri_s.as<double>(), nt, m.lv_cnt[0],
                           m.boxes.as<double>());
        for (int l = 1; l < L; ++l)
            hipLaunchKernelGGL(k_mesh_up, dim3(blocks_of(m.lv_cnt[l])), dim3(256), 0, ctx->stream,
                               m.boxes.as<double>() + 6 * (size_t) m.lv_off[l - 1], m.lv_cnt[l - 1], m.lv_cnt[l],
                               m.boxes.as<double>() + 6 * (size_t) m.lv_off[l]);
    }
    ME_CHECK(ctx, hipGetLastError());
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the host vectors and `lv` are released on return)
    m.nv = nv, m.nt = nt, m.n_deg = n_deg, m.n_levels = L;
    for (int d = 0; d < 3; ++d) m.lo[d] = lo[d], m.hi[d] = hi[d];
    m.area = total;
    m.max_abs = max_abs;
    m.have = true;
    return ME_OK;
}

int mesh_clear(me_ctx *ctx) {
    Mesh &m = *ctx->mesh;
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    m.have = false;
    mesh_drop_results(ctx);
    m.tri_in.release(), m.tri_s.release(), m.orig.release(), m.cum.release(), m.boxes.release(), m.lv.release();
    m.idx.release(), m.eid.release(), m.e_n.release(), m.e_fl.release(), m.v_n.release(), m.v_fl.release(), m.topo_cnt.release();
    reconstruct_drop(ctx);  // (the last reconstruction goes with the mesh it may have become: me_recon.hip)
    return ME_OK;
}

int mesh_info(me_ctx *ctx, me_mesh_info_out *out) {
    if (!out) return ctx->fail(ME_ERR_ARG, "me_mesh_info: NULL argument");
    const Mesh &m = *ctx->mesh;
    if (!m.have) return ctx->fail(ME_ERR_STATE, "me_mesh_info: no mesh (me_mesh_upload)");
    std::memset(out, 0, sizeof(*out));
    out->n_vertices = m.nv, out->n_triangles = m.nt, out->n_degenerate = m.n_deg, out->depth = m.n_levels;
    for (int d = 0; d < 3; ++d) out->bbox_lo[d] = m.lo[d], out->bbox_hi[d] = m.hi[d];
    out->area = m.area;
    return ME_OK;
}

int mesh_distance(me_ctx *ctx, int qslot, const me_mesh_params *p, me_mesh_out *out) {
    if (qslot < 0 || qslot > 1) return ctx->fail(ME_ERR_ARG, "me_mesh_distance: bad slot");
    if (!p || !out) return ctx->fail(ME_ERR_ARG, "me_mesh_distance: NULL argument");
    if (!(p->max_distance >= 0)) return ctx->fail(ME_ERR_ARG, "me_mesh_distance: max_distance must be >= 0 (+inf: every point)");
    if (p->n_thresholds < 0 || p->n_thresholds > ME_MESH_MAX_THRESHOLDS)
        return ctx->fail(ME_ERR_ARG, "me_mesh_distance: at most 8 thresholds");
    MdGate g{};
    g.max2 = p->max_distance * p->max_distance;
    g.nt = (int) p->n_thresholds;
    for (int k = 0; k < g.nt; ++k) {
        if (!(p->thresholds[k] >= 0) || !std::isfinite(p->thresholds[k]))
            return ctx->fail(ME_ERR_ARG, "me_mesh_distance: thresholds must be finite and >= 0");
        g.t2[k] = p->thresholds[k] * p->thresholds[k];
    }
    ME_TRY(need_single_gpu_cloud(ctx, qslot, "me_mesh_distance"));
    Mesh &m = *ctx->mesh;
    if (!m.have) return ctx->fail(ME_ERR_STATE, "me_mesh_distance: no mesh (me_mesh_upload)");
    Cloud &q = ctx->cloud[qslot];
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    q.mesh_have = false;
    q.mesh_sign_have = false;  // (the sign pass reads this result: me_meshsign.hip)
    if (!q.index_valid) ME_TRY(cloud_build_index(ctx, qslot, q.cell_size_req));  // (a slot whose points a device pass has just replaced)
    const long long n = q.n;
    ME_CHECK(ctx, q.mesh_d2.ensure((size_t) n * 8));
    ME_CHECK(ctx, q.mesh_tri.ensure((size_t) n * 4));
    ME_CHECK(ctx, q.mesh_reg.ensure((size_t) n));
    ME_CHECK(ctx, q.mesh_cp.ensure((size_t) n * 24));
    ME_CHECK(ctx, q.mesh_sd.ensure((size_t) n * 8));
    const int nb = (int) std::min<long long>(kMdBlocks, blocks_of(n));
    ME_CHECK(ctx, ctx->red.ensure(MdRed::bytes(kMdBlocks)));
    const MdRed red(ctx, kMdBlocks);
    MeshView mv{m.tri_s.as<double>(), m.orig.as<unsigned int>(), m.boxes.as<double>(), m.lv.as<int2>(), m.nt, m.n_levels,
                kMeshDeltaUlps * 0x1p-53 * m.max_abs};
    {
        TimerScope ts(ctx, "mesh_dist");
        hipLaunchKernelGGL(k_mesh_dist, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, mv, q.mesh_d2.as<double>(),
                           q.mesh_tri.as<int>(), q.mesh_reg.as<unsigned char>(), q.mesh_cp.as<double>(), q.mesh_sd.as<double>());
    }
    hipLaunchKernelGGL(k_mesh_final, dim3(nb), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, q.mesh_d2.as<double>(),
                       q.mesh_reg.as<unsigned char>(), q.mesh_sd.as<double>(), g, red.pd, red.pi);
    red.total(ctx, nb, red.tot);
    ME_CHECK(ctx, hipGetLastError());
    MdRed::Totals h;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h, red.tot, sizeof(h)));
        ME_TRY(mg.sync());
    }
    q.mesh_have = true;
    std::memset(out, 0, sizeof(*out));
    out->n_query = n;
    out->n_matched = h.i[0];
    out->n_face = h.i[1];
    out->sum_d = h.d[0], out->sum_d2 = h.d[1], out->sum_signed = h.d[2], out->sum_abs_signed = h.d[3];
    for (int k = 0; k < g.nt; ++k) out->n_within[k] = h.i[2 + k];
    out->argmax = -1;
    if (h.i[0] > 0) {
        std::memcpy(&out->max_d, &h.i[kMdNI], 8);
        out->argmax = h.i[kMdNI + 1];
    }
    return ME_OK;
}

int mesh_distance_fetch(me_ctx *ctx, int qslot, double *d2, int32_t *tri, uint8_t *region, double *closest, double *signed_d) {
    ME_TRY(need_single_gpu_cloud(ctx, qslot, "me_mesh_distance_fetch"));
    Cloud &q = ctx->cloud[qslot];
    if (!q.mesh_have || !q.index_valid || !ctx->mesh->have)
        return ctx->fail(ME_ERR_STATE,
                         "me_mesh_distance_fetch: no result for this slot (run me_mesh_distance; a changed cloud, a new index or a new mesh discards it)");
    if (!d2 && !tri && !region && !closest && !signed_d) return ME_OK;
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = q.n;
    DevBuf &buf = ctx->tmp[2];  // d2 | signed | closest | tri | region
    ME_CHECK(ctx, buf.ensure((size_t) n * (8 + 8 + 24 + 4 + 1)));
    double *dd = buf.as<double>(), *ds = dd + n, *dc = ds + n;
    int *dt = reinterpret_cast<int *>(dc + 3 * n);
    unsigned char *dr = reinterpret_cast<unsigned char *>(dt + n);
    hipLaunchKernelGGL(k_mesh_unpermute, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, q.mesh_d2.as<double>(),
                       q.mesh_tri.as<int>(), q.mesh_reg.as<unsigned char>(), q.mesh_cp.as<double>(), q.mesh_sd.as<double>(), d2 ? dd : nullptr,
                       tri ? dt : nullptr, region ? dr : nullptr, closest ? dc : nullptr, signed_d ? ds : nullptr);
    ME_CHECK(ctx, hipGetLastError());
    if (d2) ME_TRY(copy_d2h(ctx, d2, dd, (size_t) n * 8));
    if (signed_d) ME_TRY(copy_d2h(ctx, signed_d, ds, (size_t) n * 8));
    if (closest) ME_TRY(copy_d2h(ctx, closest, dc, (size_t) n * 24));
    if (tri) ME_TRY(copy_d2h(ctx, tri, dt, (size_t) n * 4));
    if (region) ME_TRY(copy_d2h(ctx, region, dr, (size_t) n));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

int mesh_sample(me_ctx *ctx, int dst_slot, long long n, unsigned long long seed) {
    if (dst_slot < 0 || dst_slot > 1) return ctx->fail(ME_ERR_ARG, "me_mesh_sample: bad slot");
    if (n < 1 || n >= (1LL << 31)) return ctx->fail(ME_ERR_ARG, "me_mesh_sample: needs 1 <= n_points < 2^31");
    if (ctx->shard_world != 1 || ctx->slab.axis >= 0) return ctx->fail(ME_ERR_ARG, "me_mesh_sample: single GPU only (no slab or shard mode)");
    Mesh &m = *ctx->mesh;
    if (!m.have) return ctx->fail(ME_ERR_STATE, "me_mesh_sample: no mesh (me_mesh_upload)");
    if (!(m.area > 0) || !std::isfinite(m.area)) return ctx->fail(ME_ERR_ARG, "me_mesh_sample: the mesh's total area is not positive and finite");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    Cloud &D = ctx->cloud[dst_slot];
    const Cloud &O = ctx->cloud[1 - dst_slot];
    ME_CHECK(ctx, D.xyz.ensure((size_t) n * 24));  // (a borrowed buffer is the caller's: ensure() replaces it by an own one)
    hipLaunchKernelGGL(k_mesh_sample, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, m.tri_in.as<double>(), m.cum.as<double>(), m.nt, m.area,
                       seed, n, D.xyz.as_mut<double>());
    ME_CHECK(ctx, hipGetLastError());
    cloud_reset_replaced(ctx, dst_slot, n, O.uploaded ? O.cell_size_req : 0.0);  // (the other cloud's cell: aligned grids for the 1-NN)
    return cloud_finish(ctx, dst_slot);
}

}  // namespace me
