// me_ray.hip — rays against the resident triangle mesh (me_mesh.hip): closest hit, any hit, a simulated range sensor moved along a
// trajectory, and the observability of a resident cloud's points from a set of origins.  Definitions: include/mapeval_hip.h,
// DESIGN.md section 4.25.
//   ray_tri        the watertight ray-triangle test of Woop, Benthin and Wald (2013) in fp64 as ONE sequence of operations (this file
//                  is compiled with -ffp-contract=off: the edge functions Qx*Py - Qy*Px are exactly antisymmetric); a degenerate
//                  triangle and a grazing one (cos^2 of the incidence below 2^-40) never hit
//   k_mesh_ray     one ray per lane, closest hit: the implicit 8-ary tree of MeshView is walked without a stack (the node index is the
//                  path, one byte per level marks the children taken OR culled), the open child with the smallest entry parameter first.
//                  A box is culled iff box_cull says so: no triangle inside it can be a computed hit with t_min <= t <= bound.
//                  The winner is the lexicographic minimum of (t, caller index): independent of the order of the walk.
//   k_mesh_occl    the same walk, left at the first hit (any hit): the answer is a boolean and does not depend on the walk
//   k_scan_trace / k_scan_emit   ray r = pose * n_dirs + beam built on the device, closest hit in [min_range, max_range] / |d|; the
//                  hits are compacted IN RAY ORDER by an exclusive scan of the hit flags into the slot's buffer, then cloud_finish
//   k_vis          one point of the slot's sorted cloud per lane, the origins in turn: any hit on the segment origin -> point
// tests/_ray_ref.py restates ray_tri, the winner, the scan and the visibility rule operation by operation without any box.
#include <cmath>
#include <cstring>
#include <vector>

#include "me_internal.hpp"
#include "me_philox.hpp"

namespace me {

namespace {

constexpr unsigned int kDegBit = 0x80000000u;  // in Mesh::orig: the triangle is degenerate (me_mesh.hip)
constexpr double kGrazeGate = 0x1p-40;         // c*c < kGrazeGate * (dot(n,n) * dot(d,d)) : a miss
constexpr double kSlabWiden = 0x1p-48;         // relative widening of a box's parameter interval (DESIGN.md 4.25 "Pruning")

struct MeshView {  // the tree me_mesh_upload built (me_mesh.hip has the same view)
    const double *tri;         // [nt][9] sorted triangles
    const unsigned int *orig;  // [nt] caller index | kDegBit
    const double *boxes;       // [nodes][6] lo xyz, hi xyz; level l at lv[l].x
    const int2 *lv;            // per level: offset into boxes, node count
    long long nt;
    int n_levels;
};

#define ME_RD __device__ __forceinline__
ME_RD double sel3(int k, double x, double y, double z) { return k == 0 ? x : (k == 1 ? y : z); }

// the per-ray constants of ray_tri.  Only the dominant component divides: a zero component of d gives a zero shear, never an infinity.
struct Ray {
    double ox, oy, oz, dx, dy, dz;
    double okx, oky, okz;  // the origin permuted by (kx, ky, kz)
    double Sx, Sy, Sz, dd;
    int kx, ky, kz;
};

// false: the ray is INVALID (a non-finite component of o or d, or d = 0) and hits nothing
ME_RD bool ray_setup(Ray &r, double ox, double oy, double oz, double dx, double dy, double dz) {
    r.ox = ox, r.oy = oy, r.oz = oz, r.dx = dx, r.dy = dy, r.dz = dz;
    const bool fin = isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz);
    const double a0 = fabs(dx), a1 = fabs(dy), a2 = fabs(dz);
    int kz = 0;
    double am = a0;
    if (a1 > am) kz = 1, am = a1;
    if (a2 > am) kz = 2, am = a2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const double dkz = sel3(kz, dx, dy, dz);
    if (dkz < 0.0) {
        const int t = kx;
        kx = ky, ky = t;
    }
    r.kx = kx, r.ky = ky, r.kz = kz;
    r.Sx = sel3(kx, dx, dy, dz) / dkz, r.Sy = sel3(ky, dx, dy, dz) / dkz, r.Sz = 1.0 / dkz;
    r.okx = sel3(kx, ox, oy, oz), r.oky = sel3(ky, ox, oy, oz), r.okz = sel3(kz, ox, oy, oz);
    r.dd = (dx * dx + dy * dy) + dz * dz;
    return fin && am > 0.0;
}

// ---- the ray-triangle routine: ONE sequence of fp64 operations (tests/_ray_ref.py restates it) ----
// true: the triangle is a hit with t_lo <= t <= t_hi; then t, the barycentric weights u (of B) and v (of C), back = det < 0
ME_RD bool ray_tri(const Ray &r, const double *__restrict__ p, bool degenerate, double t_lo, double t_hi, double &t, double &u, double &v,
                   bool &back) {
    if (degenerate) return false;
    const double a0 = p[0], a1 = p[1], a2 = p[2], b0 = p[3], b1 = p[4], b2 = p[5], c0 = p[6], c1 = p[7], c2 = p[8];
    {   // the grazing gate: n = (B - A) x (C - A), c = dot(n, d)
        const double u0 = b0 - a0, u1 = b1 - a1, u2 = b2 - a2, v0 = c0 - a0, v1 = c1 - a1, v2 = c2 - a2;
        const double n0 = u1 * v2 - u2 * v1, n1 = u2 * v0 - u0 * v2, n2 = u0 * v1 - u1 * v0;
        const double c = (n0 * r.dx + n1 * r.dy) + n2 * r.dz;
        const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
        if (c * c < kGrazeGate * (nn * r.dd)) return false;
    }
    const double Akx = sel3(r.kx, a0, a1, a2) - r.okx, Aky = sel3(r.ky, a0, a1, a2) - r.oky, Akz = sel3(r.kz, a0, a1, a2) - r.okz;
    const double Bkx = sel3(r.kx, b0, b1, b2) - r.okx, Bky = sel3(r.ky, b0, b1, b2) - r.oky, Bkz = sel3(r.kz, b0, b1, b2) - r.okz;
    const double Ckx = sel3(r.kx, c0, c1, c2) - r.okx, Cky = sel3(r.ky, c0, c1, c2) - r.oky, Ckz = sel3(r.kz, c0, c1, c2) - r.okz;
    const double Ax = Akx - r.Sx * Akz, Ay = Aky - r.Sy * Akz;
    const double Bx = Bkx - r.Sx * Bkz, By = Bky - r.Sy * Bkz;
    const double Cx = Ckx - r.Sx * Ckz, Cy = Cky - r.Sy * Ckz;
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;
    const double det = (U + V) + W;
    if (det == 0.0) return false;
    const double T = (U * (r.Sz * Akz) + V * (r.Sz * Bkz)) + W * (r.Sz * Ckz);
    t = T / det;
    if (!(t_lo <= t && t <= t_hi)) return false;
    u = V / det, v = W / det, back = det < 0.0;
    return true;
}

// The cull of a box (DESIGN.md 4.25 "Pruning"): true only if NO triangle with all corners inside the box can be a computed hit of
// ray_tri with t_lo <= t <= t_hi.  Every quantity is the one ray_tri computes for a corner, evaluated at the box faces; each rounded
// operation is monotone in its operand, so the sheared coordinates and the kz-parameters of every corner inside the box lie EXACTLY
// inside [X0, X1], [Y0, Y1] and [z0, z1].  A hit needs the origin of the sheared plane inside the triangle: not with X0 > 0 etc.
// The computed t is a convex combination of the corners' Sz * (P[kz] - o[kz]) up to 7 roundings: kSlabWiden covers them.
// `entry` is the widened lower end of the parameter interval.  A NaN anywhere compares false: the box is opened.
ME_RD bool box_cull(const Ray &r, const double *__restrict__ b, double t_lo, double t_hi, double &entry) {
    const double l0 = b[0], l1 = b[1], l2 = b[2], h0 = b[3], h1 = b[4], h2 = b[5];
    const double zl = sel3(r.kz, l0, l1, l2) - r.okz, zh = sel3(r.kz, h0, h1, h2) - r.okz;
    const double xl = sel3(r.kx, l0, l1, l2) - r.okx, xh = sel3(r.kx, h0, h1, h2) - r.okx;
    const double yl = sel3(r.ky, l0, l1, l2) - r.oky, yh = sel3(r.ky, h0, h1, h2) - r.oky;
    const double sxl = r.Sx * zl, sxh = r.Sx * zh, syl = r.Sy * zl, syh = r.Sy * zh;
    const double X0 = xl - fmax(sxl, sxh), X1 = xh - fmin(sxl, sxh);
    const double Y0 = yl - fmax(syl, syh), Y1 = yh - fmin(syl, syh);
    const double ta = r.Sz * zl, tb = r.Sz * zh;
    const double z0 = fmin(ta, tb), z1 = fmax(ta, tb);
    const double w = kSlabWiden * fmax(fabs(z0), fabs(z1));
    entry = z0 - w;
    return X0 > 0.0 || X1 < 0.0 || Y0 > 0.0 || Y1 < 0.0 || entry > t_hi || z1 + w < t_lo;
}

// the taken-children byte of level l (1 ..): levels 1-8 in `a`, 9-16 in `b` (as in k_mesh_dist)
ME_RD unsigned int taken_get(unsigned long long a, unsigned long long b, int l) {
    const int s = 8 * (l - 1);
    return (unsigned int) ((s < 64 ? a >> s : b >> (s - 64)) & 0xffull);
}
ME_RD void taken_set(unsigned long long &a, unsigned long long &b, int l, unsigned int v) {
    const int s = 8 * (l - 1);
    if (s < 64) a = (a & ~(0xffull << s)) | ((unsigned long long) v << s);
    else b = (b & ~(0xffull << (s - 64))) | ((unsigned long long) v << (s - 64));
}

struct Hit {
    double t, u, v;
    unsigned int o;  // caller index, 0xffffffff: none
    bool back;
};

// The walk.  ANY = false: the lexicographic minimum of (t, caller index) over the hits in [t_lo, t_hi]; ANY = true: left at the first hit,
// only `h.o != none` means anything.  A culled child is marked taken: a cull is final, since the bound only ever shrinks.
template <bool ANY>
ME_RD void mesh_walk(const MeshView &m, const Ray &r, double t_lo, double t_hi, Hit &h) {
    h.t = INFINITY, h.u = 0.0, h.v = 0.0, h.o = 0xffffffffu, h.back = false;
    double bound = t_hi;  // min(t_hi, best t)
    int level = m.n_levels - 1;
    long long j = 0;
    unsigned long long ta = 0, tb = 0;
    if (m.n_levels > 1) {  // (a single leaf has no box above it: its triangles are tested directly)
        double e;
        if (box_cull(r, m.boxes + 6 * (long long) m.lv[level].x, t_lo, bound, e)) return;
    }
    for (;;) {
        if (level == 0) {
            const long long t1 = min(j * 8 + 8, m.nt);
            for (long long t = j * 8; t < t1; ++t) {
                const unsigned int og = m.orig[t], o = og & ~kDegBit;
                double tt, uu, vv;
                bool bk;
                if (!ray_tri(r, m.tri + 9 * t, (og & kDegBit) != 0, t_lo, t_hi, tt, uu, vv, bk)) continue;
                if (ANY) {
                    h.o = o;
                    return;
                }
                if (tt < h.t || (tt == h.t && o < h.o)) h.t = tt, h.u = uu, h.v = vv, h.o = o, h.back = bk, bound = tt;
            }
            if (m.n_levels == 1) return;
            level = 1;
            j >>= 3;
            continue;
        }
        const int2 cl = m.lv[level - 1];
        const int nch = (int) min(8ll, (long long) cl.y - j * 8);
        unsigned int taken = taken_get(ta, tb, level);
        const double *cb = m.boxes + 6 * ((long long) cl.x + j * 8);
        double be = INFINITY;
        int bc = -1;
        for (int c = 0; c < nch; ++c) {
            if ((taken >> c) & 1u) continue;
            double e;
            if (box_cull(r, cb + 6 * c, t_lo, bound, e)) {
                taken |= 1u << c;
                continue;
            }
            if (bc < 0 || e < be) be = e, bc = c;
        }
        if (bc < 0) {
            if (level == m.n_levels - 1) return;
            taken_set(ta, tb, level, 0u);
            ++level;
            j >>= 3;
            continue;
        }
        taken_set(ta, tb, level, taken | (1u << bc));
        j = j * 8 + bc;
        --level;
    }
}

// the integer totals of a call: atomics on integers, whose result does not depend on the order of arrival
struct RayTotals {
    unsigned long long n_hit, n_backface, n_invalid, n_tests, n_visible, n_in_range;
    unsigned long long min_key, max_key;  // bit patterns of t + 0.0 >= +0.0: their order is the numeric one
};
ME_RD void count1(unsigned long long *c, bool on) {
    if (on) atomicAdd(c, 1ull);
}

__global__ void __launch_bounds__(256)
k_mesh_ray(const double *__restrict__ org, const double *__restrict__ dir, long long n, MeshView m, double t_lo, double t_hi,
           double *__restrict__ t_out, int *__restrict__ tri_out, double *__restrict__ u_out, double *__restrict__ v_out,
           unsigned char *__restrict__ fl_out, RayTotals *__restrict__ tot) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Ray r;
    const bool valid = ray_setup(r, org[3 * i], org[3 * i + 1], org[3 * i + 2], dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
    Hit h;
    h.t = INFINITY, h.u = 0.0, h.v = 0.0, h.o = 0xffffffffu, h.back = false;
    if (valid) mesh_walk<false>(m, r, t_lo, t_hi, h);
    const bool hit = h.o != 0xffffffffu;
    t_out[i] = h.t, tri_out[i] = hit ? (int) h.o : -1, u_out[i] = h.u, v_out[i] = h.v;
    fl_out[i] = (unsigned char) ((hit ? ME_RAY_HIT : 0) | (hit && h.back ? ME_RAY_BACKFACE : 0) | (valid ? 0 : ME_RAY_INVALID));
    count1(&tot->n_hit, hit);
    count1(&tot->n_backface, hit && h.back);
    count1(&tot->n_invalid, !valid);
    if (hit) {
        const unsigned long long key = (unsigned long long) __double_as_longlong(h.t + 0.0);
        atomicMin(&tot->min_key, key);
        atomicMax(&tot->max_key, key);
    }
}

__global__ void __launch_bounds__(256)
k_mesh_occl(const double *__restrict__ org, const double *__restrict__ dir, long long n, MeshView m, double t_lo, double t_hi,
            double *__restrict__ t_out, int *__restrict__ tri_out, double *__restrict__ u_out, double *__restrict__ v_out,
            unsigned char *__restrict__ fl_out, RayTotals *__restrict__ tot) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Ray r;
    const bool valid = ray_setup(r, org[3 * i], org[3 * i + 1], org[3 * i + 2], dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
    Hit h;
    h.o = 0xffffffffu;
    if (valid) mesh_walk<true>(m, r, t_lo, t_hi, h);
    const bool hit = h.o != 0xffffffffu;
    t_out[i] = INFINITY, tri_out[i] = -1, u_out[i] = 0.0, v_out[i] = 0.0;  // (which triangle the walk met first is not a result)
    fl_out[i] = (unsigned char) ((hit ? ME_RAY_HIT : 0) | (valid ? 0 : ME_RAY_INVALID));
    count1(&tot->n_hit, hit);
    count1(&tot->n_invalid, !valid);
}

// ---- the simulated sensor ----
struct ScanK {
    double min_range, max_range, noise_std;
    u64 seed;
    long long m, nd;
};

// ray r = p * nd + b: o = the pose's translation, d_w[k] = (R[k][0] dx + R[k][1] dy) + R[k][2] dz
ME_RD void scan_ray(const double *__restrict__ poses, const double *__restrict__ dirs, long long nd, long long r, double o[3], double d[3]) {
    const long long p = r / nd, b = r - p * nd;
    const double *P = poses + 16 * p;
    const double dx = dirs[3 * b], dy = dirs[3 * b + 1], dz = dirs[3 * b + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = P[4 * k + 3];
        d[k] = (P[4 * k] * dx + P[4 * k + 1] * dy) + P[4 * k + 2] * dz;
    }
}

// flag (1 hit, 0 none) and the hit parameter of every ray
__global__ void __launch_bounds__(256)
k_scan_trace(const double *__restrict__ poses, const double *__restrict__ dirs, ScanK k, MeshView m, unsigned int *__restrict__ flag,
             double *__restrict__ t_out, RayTotals *__restrict__ tot) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= k.m * k.nd) return;
    double o[3], d[3];
    scan_ray(poses, dirs, k.nd, i, o, d);
    Ray r;
    const bool valid = ray_setup(r, o[0], o[1], o[2], d[0], d[1], d[2]);
    Hit h;
    h.t = INFINITY, h.o = 0xffffffffu, h.back = false;
    if (valid) {
        const double len = sqrt(r.dd);  // |d_w|: the ranges are metres, t is in units of |d_w|
        mesh_walk<false>(m, r, k.min_range / len, k.max_range / len, h);
    }
    const bool hit = h.o != 0xffffffffu;
    flag[i] = hit ? 1u : 0u;
    t_out[i] = h.t;
    count1(&tot->n_backface, hit && h.back);
}

// the hits to their scanned places: x[k] = o[k] + t d_w[k], t = the hit parameter (+ noise_std z / |d_w|)
__global__ void __launch_bounds__(256)
k_scan_emit(const double *__restrict__ poses, const double *__restrict__ dirs, ScanK k, const unsigned int *__restrict__ flag,
            const unsigned int *__restrict__ pos, const double *__restrict__ t_in, double *__restrict__ xyz, long long *__restrict__ ray_id) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= k.m * k.nd || !flag[i]) return;
    double o[3], d[3];
    scan_ray(poses, dirs, k.nd, i, o, d);
    double t = t_in[i];
    if (k.noise_std > 0.0) {
        u64 w[4];
        philox_block(k.seed, (u64) i, 6, 0, w);
        const double rad = sqrt(-2.0 * log(u01_open0(w[0])));
        const double z = rad * cos((2.0 * M_PI) * u01(w[1]));
        const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        t = t + (k.noise_std * z) / len;
    }
    const long long q = pos[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) xyz[3 * q + c] = o[c] + t * d[c];
    ray_id[q] = i;
}

// hits of pose p = pos[(p + 1) nd] - pos[p nd] (the last pose ends at n_hit)
__global__ void __launch_bounds__(256)
k_scan_pose_counts(const unsigned int *__restrict__ pos, long long m, long long nd, long long n_hit, long long *__restrict__ cnt) {
    const long long p = (long long) blockIdx.x * 256 + threadIdx.x;
    if (p >= m) return;
    const long long a = pos[p * nd], b = p + 1 < m ? (long long) pos[(p + 1) * nd] : n_hit;
    cnt[p] = b - a;
}

// ---- observability ----
struct VisK {
    double min_range, max_range, tol;
    int first_only;
    long long m;
};

// one point of the SORTED cloud per lane; n_seen / first_seen in sorted order, the keep byte in cloud order
__global__ void __launch_bounds__(256)
k_vis(const SPoint *__restrict__ sp, long long n, const double *__restrict__ org, VisK k, MeshView m, int *__restrict__ n_seen,
      int *__restrict__ first_seen, unsigned char *__restrict__ keep, RayTotals *__restrict__ tot) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double px = sp[i].x, py = sp[i].y, pz = sp[i].z;
    int ns = 0, first = -1;
    bool in_range = false;
    unsigned long long tests = 0;
    for (long long j = 0; j < k.m; ++j) {
        const double ox = org[3 * j], oy = org[3 * j + 1], oz = org[3 * j + 2];
        const double dx = px - ox, dy = py - oy, dz = pz - oz;
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        if (!(k.min_range <= len && len <= k.max_range)) continue;
        in_range = true;
        bool seen = true;
        if (!(len <= k.tol)) {
            Ray r;
            if (ray_setup(r, ox, oy, oz, dx, dy, dz)) {
                Hit h;
                ++tests;
                mesh_walk<true>(m, r, 0.0, (len - k.tol) / len, h);
                seen = h.o == 0xffffffffu;
            } else {
                seen = false;  // (a non-finite origin or point sees nothing)
            }
        }
        if (seen) {
            if (first < 0) first = (int) j;
            ++ns;
            if (k.first_only) break;
        }
    }
    n_seen[i] = ns, first_seen[i] = first;
    keep[sp[i].idx] = ns > 0;  // (idx: a permutation of [0, n))
    count1(&tot->n_visible, ns > 0);
    count1(&tot->n_in_range, in_range);
    if (tests) atomicAdd(&tot->n_tests, tests);
}

__global__ void __launch_bounds__(256)
k_vis_unpermute(const SPoint *__restrict__ sp, long long n, const int *__restrict__ ns_s, const int *__restrict__ fs_s, int *__restrict__ ns,
                int *__restrict__ fs) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long o = sp[i].idx;
    if (ns) ns[o] = ns_s[i];
    if (fs) fs[o] = fs_s[i];
}

__global__ void k_totals_init(RayTotals *tot) {
    RayTotals z{};
    z.min_key = ~0ull;
    *tot = z;
}

MeshView view_of(const Mesh &m) {
    return MeshView{m.tri_s.as<double>(), m.orig.as<unsigned int>(), m.boxes.as<double>(), m.lv.as<int2>(), m.nt, m.n_levels};
}

// the totals block at the head of ctx->red, cleared on the stream
int totals_reset(me_ctx *ctx, RayTotals *&tot) {
    ME_CHECK(ctx, ctx->red.ensure(sizeof(RayTotals)));
    tot = ctx->red.as<RayTotals>();
    hipLaunchKernelGGL(k_totals_init, dim3(1), dim3(1), 0, ctx->stream, tot);
    ME_CHECK(ctx, hipGetLastError());
    return ME_OK;
}

int totals_read(me_ctx *ctx, const RayTotals *tot, RayTotals &h) {
    MailGuard mg(ctx);
    ME_TRY(mail_post(ctx, &h, tot, sizeof(h)));
    return mg.sync();
}

}  // namespace

int mesh_raycast(me_ctx *ctx, const double *origins, const double *dirs, long long n, double t_min, double t_max, int mode, double *t,
                 int32_t *tri, double *u, double *v, uint8_t *flags, me_ray_out *out) {
    if (!origins || !dirs || !out) return ctx->fail(ME_ERR_ARG, "me_mesh_raycast: NULL argument");
    if (n < 1 || n >= (1LL << 31)) return ctx->fail(ME_ERR_ARG, "me_mesh_raycast: needs 1 <= n_rays < 2^31");
    if (!(t_min >= 0) || !std::isfinite(t_min)) return ctx->fail(ME_ERR_ARG, "me_mesh_raycast: t_min must be finite and >= 0");
    if (!(t_max >= t_min)) return ctx->fail(ME_ERR_ARG, "me_mesh_raycast: t_max must be >= t_min (+inf: unbounded)");
    if (mode != ME_RAY_CLOSEST && mode != ME_RAY_ANY) return ctx->fail(ME_ERR_ARG, "me_mesh_raycast: mode must be ME_RAY_CLOSEST or ME_RAY_ANY");
    if (ctx->shard_world != 1 || ctx->slab.axis >= 0) return ctx->fail(ME_ERR_ARG, "me_mesh_raycast: single GPU only (no slab or shard mode)");
    const Mesh &m = *ctx->mesh;
    if (!m.have) return ctx->fail(ME_ERR_STATE, "me_mesh_raycast: no mesh (me_mesh_upload)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    DevBuf &in = ctx->tmp[0], &res = ctx->tmp[1];  // origins | dirs ; t | u | v | tri | flags
    ME_CHECK(ctx, in.ensure((size_t) n * 48));
    ME_CHECK(ctx, res.ensure((size_t) n * (24 + 4 + 1)));
    double *d_org = in.as<double>(), *d_dir = d_org + 3 * n;
    double *d_t = res.as<double>(), *d_u = d_t + n, *d_v = d_u + n;
    int *d_tri = reinterpret_cast<int *>(d_v + n);
    unsigned char *d_fl = reinterpret_cast<unsigned char *>(d_tri + n);
    ME_TRY(copy_h2d(ctx, d_org, origins, (size_t) n * 24));
    ME_TRY(copy_h2d(ctx, d_dir, dirs, (size_t) n * 24));
    RayTotals *tot = nullptr;
    ME_TRY(totals_reset(ctx, tot));
    const MeshView mv = view_of(m);
    if (mode == ME_RAY_CLOSEST) {
        TimerScope ts(ctx, "ray_cast");
        hipLaunchKernelGGL(k_mesh_ray, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, d_org, d_dir, n, mv, t_min, t_max, d_t, d_tri, d_u, d_v,
                           d_fl, tot);
    } else {
        TimerScope ts(ctx, "ray_occl");
        hipLaunchKernelGGL(k_mesh_occl, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, d_org, d_dir, n, mv, t_min, t_max, d_t, d_tri, d_u, d_v,
                           d_fl, tot);
    }
    ME_CHECK(ctx, hipGetLastError());
    RayTotals h{};
    ME_TRY(totals_read(ctx, tot, h));
    if (t) ME_TRY(copy_d2h(ctx, t, d_t, (size_t) n * 8));
    if (u) ME_TRY(copy_d2h(ctx, u, d_u, (size_t) n * 8));
    if (v) ME_TRY(copy_d2h(ctx, v, d_v, (size_t) n * 8));
    if (tri) ME_TRY(copy_d2h(ctx, tri, d_tri, (size_t) n * 4));
    if (flags) ME_TRY(copy_d2h(ctx, flags, d_fl, (size_t) n));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    std::memset(out, 0, sizeof(*out));
    out->n_rays = n;
    out->n_hit = (int64_t) h.n_hit, out->n_backface = (int64_t) h.n_backface, out->n_invalid = (int64_t) h.n_invalid;
    out->min_t = INFINITY, out->max_t = -INFINITY;
    if (mode == ME_RAY_CLOSEST && h.n_hit > 0) {
        std::memcpy(&out->min_t, &h.min_key, 8);
        std::memcpy(&out->max_t, &h.max_key, 8);
    }
    return ME_OK;
}

int mesh_scan(me_ctx *ctx, int dst_slot, const double *poses, long long m_poses, const double *dirs, long long nd, const me_scan_params *p,
              int64_t *pose_hits, me_scan_out *out) {
    if (dst_slot < 0 || dst_slot > 1) return ctx->fail(ME_ERR_ARG, "me_mesh_scan: bad slot");
    if (!poses || !dirs || !p || !out) return ctx->fail(ME_ERR_ARG, "me_mesh_scan: NULL argument");
    if (m_poses < 1 || nd < 1 || m_poses >= (1LL << 31) || nd >= (1LL << 31) || m_poses * nd >= (1LL << 31))
        return ctx->fail(ME_ERR_ARG, "me_mesh_scan: needs n_poses >= 1, n_dirs >= 1 and n_poses * n_dirs < 2^31");
    if (!(p->min_range >= 0) || !std::isfinite(p->min_range)) return ctx->fail(ME_ERR_ARG, "me_mesh_scan: min_range must be finite and >= 0");
    if (!(p->max_range >= p->min_range)) return ctx->fail(ME_ERR_ARG, "me_mesh_scan: max_range must be >= min_range (+inf: unbounded)");
    if (!(p->noise_std >= 0) || !std::isfinite(p->noise_std)) return ctx->fail(ME_ERR_ARG, "me_mesh_scan: noise_std must be finite and >= 0");
    if (ctx->shard_world != 1 || ctx->slab.axis >= 0) return ctx->fail(ME_ERR_ARG, "me_mesh_scan: single GPU only (no slab or shard mode)");
    const Mesh &m = *ctx->mesh;
    if (!m.have) return ctx->fail(ME_ERR_STATE, "me_mesh_scan: no mesh (me_mesh_upload)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = m_poses * nd;
    const ScanK k{p->min_range, p->max_range, p->noise_std, p->seed, m_poses, nd};
    DevBuf &in = ctx->tmp[0], &flag = ctx->tmp[1], &pos = ctx->tmp[2], &tt = ctx->tmp[3], &cnt = ctx->tmp[4];
    ME_CHECK(ctx, in.ensure((size_t) m_poses * 128 + (size_t) nd * 24));
    ME_CHECK(ctx, flag.ensure((size_t) n * 4));
    ME_CHECK(ctx, pos.ensure((size_t) n * 4));
    ME_CHECK(ctx, tt.ensure((size_t) n * 8));
    ME_CHECK(ctx, cnt.ensure((size_t) m_poses * 8));
    double *d_pose = in.as<double>(), *d_dir = d_pose + 16 * m_poses;
    ME_TRY(copy_h2d(ctx, d_pose, poses, (size_t) m_poses * 128));
    ME_TRY(copy_h2d(ctx, d_dir, dirs, (size_t) nd * 24));
    RayTotals *tot = nullptr;
    ME_TRY(totals_reset(ctx, tot));
    {
        TimerScope ts(ctx, "scan");
        hipLaunchKernelGGL(k_scan_trace, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, d_pose, d_dir, k, view_of(m), flag.as<unsigned int>(),
                           tt.as<double>(), tot);
    }
    ME_CHECK(ctx, hipGetLastError());
    ME_TRY(exclusive_scan_u32(ctx, flag.as<unsigned int>(), pos.as<unsigned int>(), n));
    unsigned int last_pos = 0, last_flag = 0;
    RayTotals h{};
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &last_pos, pos.as<unsigned int>() + (n - 1), 4));
        ME_TRY(mail_post(ctx, &last_flag, flag.as<unsigned int>() + (n - 1), 4));
        ME_TRY(mail_post(ctx, &h, tot, sizeof(h)));
        ME_TRY(mg.sync());
    }
    const long long n_hit = (long long) last_pos + last_flag;
    if (pose_hits) {
        hipLaunchKernelGGL(k_scan_pose_counts, dim3(blocks_of(m_poses)), dim3(256), 0, ctx->stream, pos.as<unsigned int>(), m_poses, nd, n_hit,
                           cnt.as<long long>());
        ME_CHECK(ctx, hipGetLastError());
        ME_TRY(copy_d2h(ctx, pose_hits, cnt.p, (size_t) m_poses * 8));
    }
    std::memset(out, 0, sizeof(*out));
    out->n_rays = n, out->n_hit = n_hit, out->n_backface = (int64_t) h.n_backface;
    Cloud &D = ctx->cloud[dst_slot];
    const Cloud &O = ctx->cloud[1 - dst_slot];
    const double cell_req = O.uploaded ? O.cell_size_req : 0.0;  // (the other cloud's cell: aligned grids for the 1-NN)
    D.scan_have = false;
    if (n_hit == 0) {  // an empty slot, as an upload whose slab holds nothing of the cloud leaves it
        ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        cloud_reset_replaced(ctx, dst_slot, 0, cell_req);
        D.uploaded = true;
        return ME_OK;
    }
    ME_CHECK(ctx, D.xyz.ensure((size_t) n_hit * 24));  // (a borrowed buffer is the caller's: ensure() replaces it by an own one)
    ME_CHECK(ctx, D.scan_ray.ensure((size_t) n_hit * 8));
    {
        TimerScope ts(ctx, "scan");
        hipLaunchKernelGGL(k_scan_emit, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, d_pose, d_dir, k, flag.as<unsigned int>(),
                           pos.as<unsigned int>(), tt.as<double>(), D.xyz.as_mut<double>(), D.scan_ray.as<long long>());
    }
    ME_CHECK(ctx, hipGetLastError());
    cloud_reset_replaced(ctx, dst_slot, n_hit, cell_req);
    ME_TRY(cloud_finish(ctx, dst_slot));
    D.scan_have = true;
    return ME_OK;
}

int mesh_scan_fetch(me_ctx *ctx, int slot, int64_t *ray_id) {
    if (slot < 0 || slot > 1) return ctx->fail(ME_ERR_ARG, "me_mesh_scan_fetch: bad slot");
    if (!ray_id) return ctx->fail(ME_ERR_ARG, "me_mesh_scan_fetch: NULL argument");
    Cloud &c = ctx->cloud[slot];
    if (!c.uploaded || !c.scan_have)
        return ctx->fail(ME_ERR_STATE, "me_mesh_scan_fetch: the slot's cloud is not the result of me_mesh_scan (a changed cloud discards the ray ids)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    ME_TRY(copy_d2h(ctx, ray_id, c.scan_ray.p, (size_t) c.n * 8));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

int cloud_visibility(me_ctx *ctx, int slot, const double *origins, long long m_org, const me_vis_params *p, me_vis_out *out) {
    if (slot < 0 || slot > 1) return ctx->fail(ME_ERR_ARG, "me_cloud_visibility: bad slot");
    if (!origins || !p || !out) return ctx->fail(ME_ERR_ARG, "me_cloud_visibility: NULL argument");
    if (m_org < 1 || m_org > ME_VIS_MAX_ORIGINS) return ctx->fail(ME_ERR_ARG, "me_cloud_visibility: needs 1 <= n_origins <= 65536");
    if (!(p->min_range >= 0) || !std::isfinite(p->min_range))
        return ctx->fail(ME_ERR_ARG, "me_cloud_visibility: min_range must be finite and >= 0");
    if (!(p->max_range >= p->min_range)) return ctx->fail(ME_ERR_ARG, "me_cloud_visibility: max_range must be >= min_range (+inf: unbounded)");
    if (!(p->tolerance >= 0) || !std::isfinite(p->tolerance))
        return ctx->fail(ME_ERR_ARG, "me_cloud_visibility: tolerance must be finite and >= 0");
    if (p->first_only != 0 && p->first_only != 1) return ctx->fail(ME_ERR_ARG, "me_cloud_visibility: first_only must be 0 or 1");
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_cloud_visibility"));
    const Mesh &m = *ctx->mesh;
    if (!m.have) return ctx->fail(ME_ERR_STATE, "me_cloud_visibility: no mesh (me_mesh_upload)");
    Cloud &c = ctx->cloud[slot];
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    c.vis_have = false;
    c.outlier_keep_valid = false;
    if (!c.index_valid) ME_TRY(cloud_build_index(ctx, slot, c.cell_size_req));  // (a slot whose points a device pass has just replaced)
    const long long n = c.n;
    ME_CHECK(ctx, c.vis_n.ensure((size_t) n * 4));
    ME_CHECK(ctx, c.vis_first.ensure((size_t) n * 4));
    ME_CHECK(ctx, c.outlier_keep.ensure((size_t) n));
    DevBuf &org = ctx->tmp[0];
    ME_CHECK(ctx, org.ensure((size_t) m_org * 24));
    ME_TRY(copy_h2d(ctx, org.p, origins, (size_t) m_org * 24));
    RayTotals *tot = nullptr;
    ME_TRY(totals_reset(ctx, tot));
    const VisK k{p->min_range, p->max_range, p->tolerance, (int) p->first_only, m_org};
    {
        TimerScope ts(ctx, "ray_occl");
        hipLaunchKernelGGL(k_vis, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, c.sp.as<SPoint>(), n, org.as<double>(), k, view_of(m),
                           c.vis_n.as<int>(), c.vis_first.as<int>(), c.outlier_keep.as<unsigned char>(), tot);
    }
    ME_CHECK(ctx, hipGetLastError());
    RayTotals h{};
    ME_TRY(totals_read(ctx, tot, h));
    c.vis_have = true;
    c.outlier_keep_valid = true;
    std::memset(out, 0, sizeof(*out));
    out->n_points = n;
    out->n_visible = (int64_t) h.n_visible, out->n_in_range = (int64_t) h.n_in_range, out->n_tests = (int64_t) h.n_tests;
    return ME_OK;
}

int cloud_visibility_fetch(me_ctx *ctx, int slot, int32_t *n_seen, int32_t *first_seen) {
    ME_TRY(need_single_gpu_cloud(ctx, slot, "me_cloud_visibility_fetch"));
    Cloud &c = ctx->cloud[slot];
    if (!c.vis_have || !c.index_valid || !ctx->mesh->have)
        return ctx->fail(ME_ERR_STATE,
                         "me_cloud_visibility_fetch: no result for this slot (run me_cloud_visibility; a changed cloud, a new index or a new mesh discards it)");
    if (!n_seen && !first_seen) return ME_OK;
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = c.n;
    DevBuf &buf = ctx->tmp[2];
    ME_CHECK(ctx, buf.ensure((size_t) n * 8));
    int *dn = buf.as<int>(), *df = dn + n;
    hipLaunchKernelGGL(k_vis_unpermute, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, c.sp.as<SPoint>(), n, c.vis_n.as<int>(),
                       c.vis_first.as<int>(), n_seen ? dn : nullptr, first_seen ? df : nullptr);
    ME_CHECK(ctx, hipGetLastError());
    if (n_seen) ME_TRY(copy_d2h(ctx, n_seen, dn, (size_t) n * 4));
    if (first_seen) ME_TRY(copy_d2h(ctx, first_seen, df, (size_t) n * 4));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

}  // namespace me
