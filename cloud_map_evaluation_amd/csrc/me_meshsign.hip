// me_meshsign.hip — the sign of the cloud-to-mesh distance at edges and vertices: the mesh's connectivity, the pseudo-normals of
// Baerentzen and Aanaes (2005) and a sign pass over the resident me_mesh_distance result.  Definitions: include/mapeval_hip.h,
// DESIGN.md section 4.23.  Everything is formed from the resident corners (me_mesh.hip: tri_in, after the upload's T) and the caller's
// index array, in fp64 without contraction; tests/_mesh_sign_ref.py restates it operation by operation.
//   k_topo_face     one triangle per lane, caller's order: n = (B-A) x (C-A), len, n^ = n / len, the three corner angles, the degenerate
//                   byte; the 3 edge records (key = lo << bits | hi, value = 3 t + e) and the 3 corner records (key = v, value = 3 t + c).
//                   A triangle that names a vertex twice emits edge keys above every real one: it has no edges.
//   the library's stable radix sort of either record list: the records are emitted in triangle order, so a run of equal keys is in
//   ascending (triangle, local index) order
//   k_topo_heads    the first record of every run; an exclusive scan of the flags numbers the unique edges
//   k_topo_edges    the lane of a run's first record walks the run serially: N_e, m, the flags, the edge id of every (triangle, edge)
//   k_topo_verts    the same over the corner records: N_v = sum ang * n^, ZERO, TAINTED from the flags of the incident edges
//   k_mesh_sign     one query per lane, sorted order: N by the region of the closest point, g = dot(p - c, N), signed_d and the flag byte
//   k_sign_final    the gate and the totals: block partials and the one-block total are me_reduce.hpp's; launched once for the largest
//                   and once for the smallest signed distance (the pair of me_reduce.hpp is a maximum: the second pass negates)
// Counts are integers: the per-block sums of the topology kernels are added with integer atomics, which commute exactly.
#include <cmath>
#include <cstring>

#include "me_internal.hpp"
#include "me_reduce.hpp"

namespace me {

namespace {

constexpr unsigned int kMsBlocks = 1024;
constexpr int kMsD = 3;    // sum_signed, sum_abs_signed, sum_signed2
constexpr int kMsNI = 10;  // n_matched, n_signed, n_inside, n_outside, n_on, n_unsigned, n_unreliable, n_by_region[3]
typedef RedBufs<kMsD, kMsNI> MsRed;
constexpr unsigned char kUnreliableMask =
    ME_MESH_TOPO_BOUNDARY | ME_MESH_TOPO_NONMANIFOLD | ME_MESH_TOPO_INCONSISTENT | ME_MESH_TOPO_TAINTED;
constexpr unsigned char kEdgeBadMask = ME_MESH_TOPO_BOUNDARY | ME_MESH_TOPO_NONMANIFOLD | ME_MESH_TOPO_INCONSISTENT;
// counters of the build (uint64): [0] unique edges, [1] boundary, [2] non-manifold, [3] inconsistent, [4] zero edges,
// [5] referenced vertices, [6] zero referenced vertices, [7] tainted vertices
constexpr int kTopoCounters = 8;

__global__ void __launch_bounds__(256)
k_topo_face(const double *__restrict__ tri_in, const int *__restrict__ idx, long long nt, int bits, unsigned long long no_edge,
            double *__restrict__ nhat, double *__restrict__ ang, unsigned char *__restrict__ deg, unsigned long long *__restrict__ ekey,
            unsigned long long *__restrict__ vkey, unsigned int *__restrict__ val) {
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const double *v = tri_in + 9 * t;
    const double A[3] = {v[0], v[1], v[2]}, B[3] = {v[3], v[4], v[5]}, C[3] = {v[6], v[7], v[8]};
    const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    double n[3];
    cross3(ab, ac, n);
    const bool d = n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0;
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const double bc[3] = {C[0] - B[0], C[1] - B[1], C[2] - B[2]}, ba[3] = {A[0] - B[0], A[1] - B[1], A[2] - B[2]};
    const double ca[3] = {A[0] - C[0], A[1] - C[1], A[2] - C[2]}, cb[3] = {B[0] - C[0], B[1] - C[1], B[2] - C[2]};
    deg[t] = d;
#pragma unroll
    for (int k = 0; k < 3; ++k) nhat[3 * t + k] = d ? 0.0 : n[k] / len;
    ang[3 * t] = d ? 0.0 : atan2(len, dot3(ab, ac));
    ang[3 * t + 1] = d ? 0.0 : atan2(len, dot3(bc, ba));
    ang[3 * t + 2] = d ? 0.0 : atan2(len, dot3(ca, cb));
    const int i0 = idx[3 * t], i1 = idx[3 * t + 1], i2 = idx[3 * t + 2];
    const int iv[3] = {i0, i1, i2};
    const bool twice = i0 == i1 || i1 == i2 || i2 == i0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const unsigned long long a = (unsigned long long) iv[e], b = (unsigned long long) iv[(e + 1) % 3];
        const unsigned long long lo = a < b ? a : b, hi = a < b ? b : a;
        ekey[3 * t + e] = twice ? no_edge : ((lo << bits) | hi);
        vkey[3 * t + e] = (unsigned long long) iv[e];
        val[3 * t + e] = (unsigned int) (3 * t + e);
    }
}

__global__ void __launch_bounds__(256)
k_topo_heads(const unsigned long long *__restrict__ key, long long n, unsigned long long no_edge, unsigned int *__restrict__ head,
             unsigned long long *__restrict__ counters, int counter) {
    __shared__ long long sm[4];
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    long long h = 0;
    if (i < n) {
        const unsigned long long k = key[i];
        h = k != no_edge && (i == 0 || key[i - 1] != k);
        head[i] = (unsigned int) h;
    }
    const long long s = block_sum_256_ll(h, sm);
    if (threadIdx.x == 0 && s) atomicAdd(counters + counter, (unsigned long long) s);
}

// key / val: the sorted edge records; head / rank: the first-of-run flags and their exclusive scan (= the edge id)
__global__ void __launch_bounds__(256)
k_topo_edges(const unsigned long long *__restrict__ key, const unsigned int *__restrict__ val, const unsigned int *__restrict__ head,
             const unsigned int *__restrict__ rank, long long n, const int *__restrict__ idx, const double *__restrict__ nhat,
             const unsigned char *__restrict__ deg, double *__restrict__ e_n, unsigned char *__restrict__ e_fl, int *__restrict__ eid,
             unsigned long long *__restrict__ counters) {
    __shared__ long long sm[4];
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    long long c[4] = {0, 0, 0, 0};  // boundary, non-manifold, inconsistent, zero
    if (i < n && head[i]) {
        const unsigned long long k = key[i];
        const int id = (int) rank[i];
        double s[3] = {0.0, 0.0, 0.0};
        long long m = 0, n_face = 0;
        int dir0 = 0, same = 0;
        for (long long j = i; j < n && key[j] == k; ++j) {
            const unsigned int r = val[j];
            const long long t = r / 3;
            const int e = (int) (r % 3);
            const int dir = idx[3 * t + e] < idx[3 * t + (e + 1) % 3];
            if (m == 0) dir0 = dir;
            else if (m == 1) same = dir == dir0;
            ++m;
            if (!deg[t]) {
                ++n_face;
                s[0] += nhat[3 * t], s[1] += nhat[3 * t + 1], s[2] += nhat[3 * t + 2];
            }
            eid[3 * t + e] = id;
        }
        unsigned char f = 0;
        if (m == 1) f |= ME_MESH_TOPO_BOUNDARY, c[0] = 1;
        if (m > 2) f |= ME_MESH_TOPO_NONMANIFOLD, c[1] = 1;
        if (m == 2 && same) f |= ME_MESH_TOPO_INCONSISTENT, c[2] = 1;
        if (n_face == 0 || (s[0] == 0.0 && s[1] == 0.0 && s[2] == 0.0)) f |= ME_MESH_TOPO_ZERO, c[3] = 1;
        e_n[3 * (long long) id] = s[0], e_n[3 * (long long) id + 1] = s[1], e_n[3 * (long long) id + 2] = s[2];
        e_fl[id] = f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long s = block_sum_256_ll(c[q], sm);
        if (threadIdx.x == 0 && s) atomicAdd(counters + 1 + q, (unsigned long long) s);
    }
}

// key / val: the sorted corner records.  v_n / v_fl were preset to zero / ZERO: an unreferenced vertex keeps that.
__global__ void __launch_bounds__(256)
k_topo_verts(const unsigned long long *__restrict__ key, const unsigned int *__restrict__ val, long long n, const double *__restrict__ nhat,
             const double *__restrict__ ang, const unsigned char *__restrict__ deg, const int *__restrict__ eid,
             const unsigned char *__restrict__ e_fl, double *__restrict__ v_n, unsigned char *__restrict__ v_fl,
             unsigned long long *__restrict__ counters) {
    __shared__ long long sm[4];
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    long long c[3] = {0, 0, 0};  // referenced, zero, tainted
    if (i < n && (i == 0 || key[i - 1] != key[i])) {
        const unsigned long long k = key[i];
        double s[3] = {0.0, 0.0, 0.0};
        long long n_face = 0;
        unsigned char bad = 0;
        for (long long j = i; j < n && key[j] == k; ++j) {
            const unsigned int r = val[j];
            const long long t = r / 3;
            const int cn = (int) (r % 3);
            if (!deg[t]) {
                const double a = ang[r];
                ++n_face;
                s[0] += a * nhat[3 * t], s[1] += a * nhat[3 * t + 1], s[2] += a * nhat[3 * t + 2];
            }
            const int e0 = eid[3 * t + cn], e1 = eid[3 * t + (cn + 2) % 3];  // the two edges of the triangle that meet in this corner
            if (e0 >= 0) bad |= e_fl[e0];
            if (e1 >= 0) bad |= e_fl[e1];
        }
        unsigned char f = 0;
        c[0] = 1;
        if (n_face == 0 || (s[0] == 0.0 && s[1] == 0.0 && s[2] == 0.0)) f |= ME_MESH_TOPO_ZERO, c[1] = 1;
        if (bad & kEdgeBadMask) f |= ME_MESH_TOPO_TAINTED, c[2] = 1;
        v_n[3 * k] = s[0], v_n[3 * k + 1] = s[1], v_n[3 * k + 2] = s[2];
        v_fl[k] = f;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const long long s = block_sum_256_ll(c[q], sm);
        if (threadIdx.x == 0 && s) atomicAdd(counters + 5 + q, (unsigned long long) s);
    }
}

// the edge tables per (triangle, local edge), for the fetch; a triangle without edges: zero normal, ZERO
__global__ void __launch_bounds__(256)
k_topo_expand(const int *__restrict__ eid, const double *__restrict__ e_n, const unsigned char *__restrict__ e_fl, long long n3,
              double *__restrict__ out_n, unsigned char *__restrict__ out_fl) {
    const long long r = (long long) blockIdx.x * 256 + threadIdx.x;
    if (r >= n3) return;
    const int id = eid[r];
#pragma unroll
    for (int k = 0; k < 3; ++k) out_n[3 * r + k] = id >= 0 ? e_n[3 * (long long) id + k] : 0.0;
    out_fl[r] = id >= 0 ? e_fl[id] : (unsigned char) ME_MESH_TOPO_ZERO;
}

struct SignView {
    const double *tri_in;       // [nt][9] caller's order
    const int *idx;             // [nt][3]
    const int *eid;             // [nt][3]
    const double *e_n, *v_n;    // [E][3], [nv][3]
    const unsigned char *e_fl, *v_fl;
    long long nt;
};

// results in SORTED order: sd[n], fl[n]
__global__ void __launch_bounds__(256)
k_mesh_sign(const SPoint *__restrict__ sp, long long n, const double *__restrict__ d2_s, const int *__restrict__ tri_s,
            const unsigned char *__restrict__ reg_s, const double *__restrict__ cp_s, SignView m, double *__restrict__ sd,
            unsigned char *__restrict__ fl) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double d2 = d2_s[i];
    const long long t = tri_s[i];
    const int r = reg_s[i];
    if (t < 0 || t >= m.nt) {  // (a query without a winner: a NaN coordinate)
        sd[i] = NAN, fl[i] = ME_MESH_SIGN_UNSIGNED;
        return;
    }
    const double *v = m.tri_in + 9 * t;
    const double ab[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, ac[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
    double nn[3];
    cross3(ab, ac, nn);
    const bool degenerate = nn[0] == 0.0 && nn[1] == 0.0 && nn[2] == 0.0;
    unsigned char tf = 0;  // the feature's topology flags
    if (r >= 1 && r <= 3) {
        const int id = m.eid[3 * t + (r - 1)];
        if (id >= 0) {
            nn[0] = m.e_n[3 * (long long) id], nn[1] = m.e_n[3 * (long long) id + 1], nn[2] = m.e_n[3 * (long long) id + 2];
            tf = m.e_fl[id];
        } else {
            nn[0] = nn[1] = nn[2] = 0.0;
            tf = ME_MESH_TOPO_ZERO;
        }
    } else if (r >= 4) {
        const long long vi = m.idx[3 * t + (r - 4)];
        nn[0] = m.v_n[3 * vi], nn[1] = m.v_n[3 * vi + 1], nn[2] = m.v_n[3 * vi + 2];
        tf = m.v_fl[vi];
    }
    const double e[3] = {sp[i].x - cp_s[i], sp[i].y - cp_s[n + i], sp[i].z - cp_s[2 * n + i]};
    const double g = dot3(e, nn);
    double s = NAN;
    unsigned char f = (tf & kUnreliableMask) ? ME_MESH_SIGN_UNRELIABLE : 0;
    if (d2 == 0.0) s = 0.0, f |= ME_MESH_SIGN_ON;
    else if (degenerate || (tf & ME_MESH_TOPO_ZERO)) f |= ME_MESH_SIGN_UNSIGNED;
    else if (g > 0.0) s = sqrt(d2);
    else if (g < 0.0) s = -sqrt(d2);
    else f |= ME_MESH_SIGN_UNSIGNED;
    sd[i] = s;
    fl[i] = f;
}

// a double as an unsigned key of the same order (no NaN comes here)
__device__ __forceinline__ unsigned long long ordered_key(double x) {
    const unsigned long long b = (unsigned long long) __double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double ordered_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    std::memcpy(&x, &b, 8);
    return x;
}

// negate: the pair is the largest of -signed_d (the smallest signed distance)
__global__ void __launch_bounds__(256)
k_sign_final(const SPoint *__restrict__ sp, long long n, const double *__restrict__ d2_s, const unsigned char *__restrict__ reg_s,
             const double *__restrict__ sd_s, const unsigned char *__restrict__ fl_s, double max2, int negate, double *__restrict__ pd,
             long long *__restrict__ pi) {
    long long arg = -1, ci[kMsNI];
#pragma unroll
    for (int k = 0; k < kMsNI; ++k) ci[k] = 0;
    unsigned long long mx = 0ull;
    double sd[kMsD] = {0.0, 0.0, 0.0};
    const long long stride = (long long) gridDim.x * 256;
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        if (!(d2_s[i] <= max2)) continue;
        const double s = sd_s[i];
        const unsigned char f = fl_s[i];
        const int r = reg_s[i];
        ci[0] += 1;
        ci[6] += (f & ME_MESH_SIGN_UNRELIABLE) ? 1 : 0;
        ci[7] += r == 0, ci[8] += r >= 1 && r <= 3, ci[9] += r >= 4;
        if (f & ME_MESH_SIGN_UNSIGNED) {
            ci[5] += 1;
            continue;
        }
        ci[1] += 1;
        if (f & ME_MESH_SIGN_ON) ci[4] += 1;
        else if (s < 0.0) ci[2] += 1;
        else ci[3] += 1;
        sd[0] += s;
        sd[1] += fabs(s);
        sd[2] += s * s;
        take_max(mx, arg, ordered_key(negate ? -s : s), sp[i].idx);
    }
    red_store_partial<kMsD, kMsNI, false>(sd, ci, mx, arg, 0ull, pd + (size_t) blockIdx.x * kMsD, pi + (size_t) blockIdx.x * MsRed::Totals::NR);
}

// every output is nullable
__global__ void __launch_bounds__(256)
k_sign_unpermute(const SPoint *__restrict__ sp, long long n, const double *__restrict__ sd_s, const unsigned char *__restrict__ fl_s,
                 double *__restrict__ sd, unsigned char *__restrict__ fl) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long o = sp[i].idx;  // a permutation of [0, n)
    if (sd) sd[o] = sd_s[i];
    if (fl) fl[o] = fl_s[i];
}

int need_mesh_ctx(me_ctx *ctx, const char *who) {
    if (ctx->shard_world != 1 || ctx->slab.axis >= 0) return ctx->fail(ME_ERR_ARG, std::string(who) + ": single GPU only (no slab or shard mode)");
    if (!ctx->mesh->have) return ctx->fail(ME_ERR_STATE, std::string(who) + ": no mesh (me_mesh_upload)");
    return ME_OK;
}

int topo_build(me_ctx *ctx, const char *who) {
    Mesh &m = *ctx->mesh;
    if (m.topo_have) return ME_OK;
    const long long nt = m.nt, nv = m.nv, n3 = 3 * nt;
    if (n3 >= (1LL << 32)) return ctx->fail(ME_ERR_ARG, std::string(who) + ": the topology needs 3 * n_triangles < 2^32");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    int bits = 1;
    while ((1LL << bits) <= nv) ++bits;  // nv < 2^bits <= 2^31: `nv` itself is a free value
    const unsigned long long no_edge = ((unsigned long long) nv << bits) | (unsigned long long) nv;
    DevBuf &fbuf = ctx->tmp[0], &kbuf = ctx->tmp[1], &vbuf = ctx->tmp[2], &hbuf = ctx->tmp[3], &dbuf = ctx->tmp[4];
    ME_CHECK(ctx, fbuf.ensure((size_t) nt * 48));  // n^ | angles
    ME_CHECK(ctx, kbuf.ensure((size_t) n3 * 24));  // edge keys | corner keys | sorted keys
    ME_CHECK(ctx, vbuf.ensure((size_t) n3 * 8));   // values | sorted values
    ME_CHECK(ctx, hbuf.ensure((size_t) n3 * 8));   // first-of-run flags | their scan
    ME_CHECK(ctx, dbuf.ensure((size_t) nt));       // degenerate bytes
    ME_CHECK(ctx, m.eid.ensure((size_t) n3 * 4));
    ME_CHECK(ctx, m.v_n.ensure((size_t) nv * 24));
    ME_CHECK(ctx, m.v_fl.ensure((size_t) nv));
    ME_CHECK(ctx, m.topo_cnt.ensure(kTopoCounters * 8));
    double *nhat = fbuf.as<double>(), *ang = nhat + 3 * nt;
    unsigned long long *ekey = kbuf.as<unsigned long long>(), *vkey = ekey + n3, *skey = vkey + n3;
    unsigned int *val = vbuf.as<unsigned int>(), *sval = val + n3;
    unsigned int *head = hbuf.as<unsigned int>(), *rank = head + n3;
    unsigned char *deg = dbuf.as<unsigned char>();
    unsigned long long *cnt = m.topo_cnt.as<unsigned long long>();
    const int *idx = m.idx.as<int>();
    ME_CHECK(ctx, hipMemsetAsync(cnt, 0, kTopoCounters * 8, ctx->stream));
    ME_CHECK(ctx, hipMemsetAsync(m.eid.p, 0xff, (size_t) n3 * 4, ctx->stream));  // -1: a triangle without edges
    ME_CHECK(ctx, hipMemsetAsync(m.v_n.p, 0, (size_t) nv * 24, ctx->stream));
    ME_CHECK(ctx, hipMemsetAsync(m.v_fl.p, ME_MESH_TOPO_ZERO, (size_t) nv, ctx->stream));
    {
        TimerScope ts(ctx, "mesh_topology");
        hipLaunchKernelGGL(k_topo_face, dim3(blocks_of(nt)), dim3(256), 0, ctx->stream, m.tri_in.as<double>(), idx, nt, bits, no_edge, nhat, ang,
                           deg, ekey, vkey, val);
    }
    ME_TRY(sort_pairs_u64_u32(ctx, ekey, skey, val, sval, n3, 0, 2 * bits));
    {
        TimerScope ts(ctx, "mesh_topology");
        hipLaunchKernelGGL(k_topo_heads, dim3(blocks_of(n3)), dim3(256), 0, ctx->stream, (const unsigned long long *) skey, n3, no_edge, head,
                           cnt, 0);
    }
    ME_TRY(exclusive_scan_u32(ctx, head, rank, n3));
    unsigned long long n_edges = 0;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &n_edges, cnt, 8));
        ME_TRY(mg.sync());
    }
    ME_CHECK(ctx, m.e_n.ensure(std::max<size_t>(1, (size_t) n_edges) * 24));
    ME_CHECK(ctx, m.e_fl.ensure(std::max<size_t>(1, (size_t) n_edges)));
    {
        TimerScope ts(ctx, "mesh_topology");
        hipLaunchKernelGGL(k_topo_edges, dim3(blocks_of(n3)), dim3(256), 0, ctx->stream, (const unsigned long long *) skey,
                           (const unsigned int *) sval, (const unsigned int *) head, (const unsigned int *) rank, n3, idx,
                           (const double *) nhat, (const unsigned char *) deg, m.e_n.as<double>(), m.e_fl.as<unsigned char>(), m.eid.as<int>(),
                           cnt);
    }
    ME_TRY(sort_pairs_u64_u32(ctx, vkey, skey, val, sval, n3, 0, bits));
    {
        TimerScope ts(ctx, "mesh_topology");
        hipLaunchKernelGGL(k_topo_verts, dim3(blocks_of(n3)), dim3(256), 0, ctx->stream, (const unsigned long long *) skey,
                           (const unsigned int *) sval, n3, (const double *) nhat, (const double *) ang, (const unsigned char *) deg,
                           (const int *) m.eid.as<int>(), (const unsigned char *) m.e_fl.as<unsigned char>(), m.v_n.as<double>(),
                           m.v_fl.as<unsigned char>(), cnt);
    }
    ME_CHECK(ctx, hipGetLastError());
    unsigned long long h[kTopoCounters];
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, h, cnt, sizeof(h)));
        ME_TRY(mg.sync());
    }
    me_mesh_topo_out &o = m.topo;
    std::memset(&o, 0, sizeof(o));
    o.n_edges = (int64_t) h[0], o.n_boundary_edges = (int64_t) h[1], o.n_nonmanifold_edges = (int64_t) h[2];
    o.n_inconsistent_edges = (int64_t) h[3], o.n_zero_edges = (int64_t) h[4];
    o.n_unreferenced_vertices = nv - (int64_t) h[5];
    o.n_zero_vertices = (int64_t) h[6] + o.n_unreferenced_vertices;
    o.n_tainted_vertices = (int64_t) h[7];
    o.closed = h[1] == 0;
    o.oriented_manifold = h[1] == 0 && h[2] == 0 && h[3] == 0;
    m.n_edges = (long long) h[0];
    m.topo_have = true;
    return ME_OK;
}

}  // namespace

int mesh_topology(me_ctx *ctx, me_mesh_topo_out *out) {
    if (!out) return ctx->fail(ME_ERR_ARG, "me_mesh_topology: NULL argument");
    ME_TRY(need_mesh_ctx(ctx, "me_mesh_topology"));
    ME_TRY(topo_build(ctx, "me_mesh_topology"));
    *out = ctx->mesh->topo;
    return ME_OK;
}

int mesh_topology_fetch(me_ctx *ctx, double *vertex_normal, uint8_t *vertex_flags, double *edge_normal, uint8_t *edge_flags) {
    ME_TRY(need_mesh_ctx(ctx, "me_mesh_topology_fetch"));
    ME_TRY(topo_build(ctx, "me_mesh_topology_fetch"));
    Mesh &m = *ctx->mesh;
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    if (vertex_normal) ME_TRY(copy_d2h(ctx, vertex_normal, m.v_n.p, (size_t) m.nv * 24));
    if (vertex_flags) ME_TRY(copy_d2h(ctx, vertex_flags, m.v_fl.p, (size_t) m.nv));
    if (edge_normal || edge_flags) {
        const long long n3 = 3 * m.nt;
        DevBuf &buf = ctx->tmp[2];  // normals | flags
        ME_CHECK(ctx, buf.ensure((size_t) n3 * 25));
        double *dn = buf.as<double>();
        unsigned char *df = reinterpret_cast<unsigned char *>(dn + 3 * n3);
        hipLaunchKernelGGL(k_topo_expand, dim3(blocks_of(n3)), dim3(256), 0, ctx->stream, (const int *) m.eid.as<int>(),
                           (const double *) m.e_n.as<double>(), (const unsigned char *) m.e_fl.as<unsigned char>(), n3, dn, df);
        ME_CHECK(ctx, hipGetLastError());
        if (edge_normal) ME_TRY(copy_d2h(ctx, edge_normal, dn, (size_t) n3 * 24));
        if (edge_flags) ME_TRY(copy_d2h(ctx, edge_flags, df, (size_t) n3));
    }
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

int mesh_signed_distance(me_ctx *ctx, int qslot, const me_mesh_sign_params *p, me_mesh_sign_out *out) {
    if (qslot < 0 || qslot > 1) return ctx->fail(ME_ERR_ARG, "me_mesh_signed_distance: bad slot");
    if (!p || !out) return ctx->fail(ME_ERR_ARG, "me_mesh_signed_distance: NULL argument");
    if (!(p->max_distance >= 0)) return ctx->fail(ME_ERR_ARG, "me_mesh_signed_distance: max_distance must be >= 0 (+inf: every point)");
    ME_TRY(need_single_gpu_cloud(ctx, qslot, "me_mesh_signed_distance"));
    Mesh &m = *ctx->mesh;
    Cloud &q = ctx->cloud[qslot];
    if (!m.have) return ctx->fail(ME_ERR_STATE, "me_mesh_signed_distance: no mesh (me_mesh_upload)");
    if (!q.mesh_have || !q.index_valid)
        return ctx->fail(ME_ERR_STATE, "me_mesh_signed_distance: no mesh-distance result for this slot (run me_mesh_distance first)");
    ME_TRY(topo_build(ctx, "me_mesh_signed_distance"));
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    q.mesh_sign_have = false;
    const long long n = q.n;
    ME_CHECK(ctx, q.mesh_ssd.ensure((size_t) n * 8));
    ME_CHECK(ctx, q.mesh_sfl.ensure((size_t) n));
    const int nb = (int) std::min<long long>(kMsBlocks, blocks_of(n));
    ME_CHECK(ctx, ctx->red.ensure(MsRed::bytes(kMsBlocks)));
    const MsRed red(ctx, kMsBlocks);
    const SignView sv{m.tri_in.as<double>(), m.idx.as<int>(),           m.eid.as<int>(),          m.e_n.as<double>(),
                      m.v_n.as<double>(),    m.e_fl.as<unsigned char>(), m.v_fl.as<unsigned char>(), m.nt};
    {
        TimerScope ts(ctx, "mesh_sign");
        hipLaunchKernelGGL(k_mesh_sign, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, q.mesh_d2.as<double>(),
                           q.mesh_tri.as<int>(), q.mesh_reg.as<unsigned char>(), q.mesh_cp.as<double>(), sv, q.mesh_ssd.as<double>(),
                           q.mesh_sfl.as<unsigned char>());
    }
    const double max2 = p->max_distance * p->max_distance;
    MsRed::Totals h[2];
    {
        MailGuard mg(ctx);
        for (int negate = 0; negate < 2; ++negate) {  // (the stream orders the second pass behind the first one's post)
            hipLaunchKernelGGL(k_sign_final, dim3(nb), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, q.mesh_d2.as<double>(),
                               q.mesh_reg.as<unsigned char>(), q.mesh_ssd.as<double>(), q.mesh_sfl.as<unsigned char>(), max2, negate, red.pd,
                               red.pi);
            red.total(ctx, nb, red.tot);
            ME_CHECK(ctx, hipGetLastError());
            ME_TRY(mail_post(ctx, &h[negate], red.tot, sizeof(h[0])));
        }
        ME_TRY(mg.sync());
    }
    q.mesh_sign_have = true;
    std::memset(out, 0, sizeof(*out));
    out->n_query = n;
    out->n_matched = h[0].i[0], out->n_signed = h[0].i[1], out->n_inside = h[0].i[2], out->n_outside = h[0].i[3];
    out->n_on = h[0].i[4], out->n_unsigned = h[0].i[5], out->n_unreliable = h[0].i[6];
    for (int k = 0; k < 3; ++k) out->n_by_region[k] = h[0].i[7 + k];
    out->sum_signed = h[0].d[0], out->sum_abs_signed = h[0].d[1], out->sum_signed2 = h[0].d[2];
    out->argmax = out->argmin = -1;
    if (h[0].i[1] > 0) {
        out->max_signed = ordered_value((unsigned long long) h[0].i[kMsNI]);
        out->argmax = h[0].i[kMsNI + 1];
        out->min_signed = -ordered_value((unsigned long long) h[1].i[kMsNI]);
        out->argmin = h[1].i[kMsNI + 1];
    }
    return ME_OK;
}

int mesh_signed_fetch(me_ctx *ctx, int qslot, double *signed_d, uint8_t *flags) {
    ME_TRY(need_single_gpu_cloud(ctx, qslot, "me_mesh_signed_fetch"));
    Cloud &q = ctx->cloud[qslot];
    if (!q.mesh_have || !q.mesh_sign_have || !q.index_valid || !ctx->mesh->have)
        return ctx->fail(ME_ERR_STATE,
                         "me_mesh_signed_fetch: no result for this slot (run me_mesh_signed_distance; whatever discards the mesh-distance "
                         "result, and a new me_mesh_distance, discards it)");
    if (!signed_d && !flags) return ME_OK;
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = q.n;
    DevBuf &buf = ctx->tmp[2];  // signed | flags
    ME_CHECK(ctx, buf.ensure((size_t) n * 9));
    double *ds = buf.as<double>();
    unsigned char *df = reinterpret_cast<unsigned char *>(ds + n);
    hipLaunchKernelGGL(k_sign_unpermute, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, q.sp.as<SPoint>(), n, q.mesh_ssd.as<double>(),
                       q.mesh_sfl.as<unsigned char>(), signed_d ? ds : nullptr, flags ? df : nullptr);
    ME_CHECK(ctx, hipGetLastError());
    if (signed_d) ME_TRY(copy_d2h(ctx, signed_d, ds, (size_t) n * 8));
    if (flags) ME_TRY(copy_d2h(ctx, flags, df, (size_t) n));
    ME_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ME_OK;
}

}  // namespace me
