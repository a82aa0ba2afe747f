// me_recon.hip — surface reconstruction of a resident cloud into a triangle mesh: an implicit-moving-least-squares (IMLS) signed-distance
// field on a sparse voxel lattice, from the points and their resident normals, and its zero set by marching tetrahedra.  The definition
// is in include/mapeval_hip.h and DESIGN.md section 4.19; tests/_recon_ref.py restates it.
//   lattice        the cell floor(p / h) of every point, as a Morton key in the LATTICE frame (origin = the smallest active cell per
//                  axis, 21 bits per axis) -> radix sort -> unique = the occupied cells; dilated by `band` one axis at a time (a
//                  Chebyshev ball is a product of intervals: expand, sort, unique, three times), then the 8 corners the same way = the
//                  nodes, in Morton order.  Nothing is sized as a dense grid.                                   (k_rc_point_keys, k_rc_expand)
//   k_recon_field  one node per lane, nodes in Morton order, so that a wave's 64 nodes are lattice neighbours.  The node x = (i h, j h,
//                  k h) is placed in the cloud's cell table as k_m3_stream<true> places a foreign query (fine_coord, clamped; a node a
//                  cell or more outside the frame is settled with k = 0) and streams the 27-cell neighbourhood through the wave's LDS
//                  tile (me_wave_stream.hpp).  The stage callback puts the candidate's normal into a second LDS tile beside the
//                  coordinates (3 doubles per entry: 1.5 KB per wave on top of the 1.5 KB of coordinates and the 2.7 KB run table;
//                  every read of either tile is a wave-uniform address, i.e. a broadcast, and lane j writes entry j: no bank conflict)
//                  and, where the normal is the zero vector or not finite, overwrites the staged x by NaN: d2 is then NaN, the strict
//                  test d2 < R*R fails and the point contributes nothing and is not counted — at no cost in the candidate loop.
//                  The slot's index cell edge must be >= R: me_m3c2's rule (rebuilt at R unless R (1 + 2^-20) <= cell_h <= 1.5 R (1 +
//                  2^-20)), and a rebuild re-sorts the slot: the 1-NN results of both slots, the slot's local-geometry, M3C2 and
//                  mesh-distance results are dropped (drop_sorted_results); the points, the normals (cloud order) and the other
//                  slot's M3C2 result stay.
//   extraction     k_rc_cells: a node finds its 7 neighbours a + dir by binary search in the sorted node keys, decides whether the cell
//                  it is corner 0 of is extracted, packs the 8 inside bits, marks the crossed ones of the cell's 19 Kuhn edges (plain
//                  byte stores of 1 into a zeroed array: every writer writes the same value) and counts the cell's triangles;
//                  the marked edges are compacted in ascending (node, dir) order = the vertex ids; the counts are scanned;
//                  k_rc_vertices computes every vertex from its edge's origin node; k_rc_emit writes the triangles of cell after cell,
//                  looking the vertex ids up by binary search in the sorted edge list.  The case table (6 tetrahedra x 16 sign
//                  patterns, winding from integer determinants) is built at compile time.  Counts are integer atomics only: the
//                  result is a pure function of the input, identical bytes from call to call.
// The file is compiled with -ffp-contract=off.  Device timers: "recon_field", "recon_extract"; the sorts report under "sort".
#include <cmath>
#include <cstring>

#include "me_internal.hpp"
#include "me_wave_stream.hpp"

namespace me {

namespace {

typedef unsigned long long u64;

constexpr long long kRcMaxRel = (1LL << kMortonBits) - 1;  // largest node coordinate of the lattice frame
constexpr double kRcMaxCell = 1073741824.0;                // |floor(p / h)| must stay below 2^30: the indices are int32

// counters of one call (u64 each)
enum { RC_VALID = 0, RC_SUMK, RC_CELLS, RC_NTRI, RC_NDEG, RC_NVERT, RC_NDUP, RC_NUNIQ, RC_COUNT };

// ---- the marching-tetrahedra case table, built at compile time -------------------------------------------------------------------------
// corner code = x | y << 1 | z << 2; dir (0 .. 6) = 100 010 001 110 101 011 111 as (dx dy dz)
struct ReconTab {
    unsigned char dir_mask[7];       // dir -> corner code of the offset
    unsigned char mask_dir[8];       // corner code of an offset -> dir (0 unused)
    unsigned char corner[6][4];      // corner codes of the 4 corners of every Kuhn tetrahedron (a chain 0 = v0 < v1 < v2 < v3 = 7)
    unsigned char ntri[6][16];       // triangles of a tetrahedron by its 4 inside bits (bit j = corner j inside)
    unsigned char tri[6][16][2][3];  // their edges: origin corner code << 3 | dir
};

constexpr int rc_vec(int code, int d) { return (code >> d) & 1; }
constexpr int rc_det(const unsigned char *c, int p, int a, int b, int q) {  // det[a - p, b - p, q - p] of the tetrahedron's corners
    int u[3] = {0, 0, 0}, v[3] = {0, 0, 0}, w[3] = {0, 0, 0};
    for (int d = 0; d < 3; ++d) {
        u[d] = rc_vec(c[a], d) - rc_vec(c[p], d);
        v[d] = rc_vec(c[b], d) - rc_vec(c[p], d);
        w[d] = rc_vec(c[q], d) - rc_vec(c[p], d);
    }
    return u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0]);
}

constexpr ReconTab make_recon_tab() {
    ReconTab t{};
    const unsigned char dm[7] = {1, 2, 4, 3, 5, 6, 7};
    for (int d = 0; d < 7; ++d) {
        t.dir_mask[d] = dm[d];
        t.mask_dir[dm[d]] = (unsigned char) d;
    }
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};  // lexicographic
    for (int k = 0; k < 6; ++k) {
        unsigned char *c = t.corner[k];
        c[0] = 0;
        c[1] = (unsigned char) (1 << perm[k][0]);
        c[2] = (unsigned char) (c[1] | (1 << perm[k][1]));
        c[3] = (unsigned char) (c[2] | (1 << perm[k][2]));
        for (int m = 0; m < 16; ++m) {
            int ins[4] = {0, 0, 0, 0}, outs[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int j = 0; j < 4; ++j) {
                if ((m >> j) & 1) ins[ni++] = j;
                else outs[no++] = j;
            }
            // an edge between the tetrahedron-local corners x and y: its origin is the lower one (componentwise smaller)
            int e[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, tri[2][3] = {{0, 1, 2}, {0, 2, 3}}, nt = 0;
            bool keep = true;
            if (ni == 1 || ni == 3) {
                const int p = ni == 1 ? ins[0] : outs[0];
                int q[3] = {0, 0, 0}, nq = 0;
                for (int j = 0; j < 4; ++j)
                    if (j != p) q[nq++] = j;
                for (int j = 0; j < 3; ++j) e[j][0] = p, e[j][1] = q[j];
                const int det = rc_det(c, p, q[0], q[1], q[2]);
                keep = ni == 1 ? det > 0 : det < 0;
                nt = 1;
            } else if (ni == 2) {
                const int p = ins[0], q = ins[1], r = outs[0], s = outs[1];
                e[0][0] = p, e[0][1] = r;
                e[1][0] = p, e[1][1] = s;
                e[2][0] = q, e[2][1] = s;
                e[3][0] = q, e[3][1] = r;
                keep = rc_det(c, p, r, s, q) > 0;
                nt = 2;
            }
            t.ntri[k][m] = (unsigned char) nt;
            for (int a = 0; a < nt; ++a)
                for (int b = 0; b < 3; ++b) {
                    const int which = tri[a][keep ? b : (b == 0 ? 0 : 3 - b)];
                    const int lo = e[which][0] < e[which][1] ? e[which][0] : e[which][1];
                    const int hi = e[which][0] < e[which][1] ? e[which][1] : e[which][0];
                    t.tri[k][m][a][b] = (unsigned char) ((c[lo] << 3) | t.mask_dir[c[hi] ^ c[lo]]);
                }
        }
    }
    return t;
}

__constant__ ReconTab c_rtab = make_recon_tab();

// ---- keys ----
__device__ __forceinline__ u64 rc_key(long long x, long long y, long long z) {
    return spread21((u64) x) | (spread21((u64) y) << 1) | (spread21((u64) z) << 2);
}
__device__ __forceinline__ void rc_unkey(u64 k, int &x, int &y, int &z) {
    x = (int) compact21(k);
    y = (int) compact21(k >> 1);
    z = (int) compact21(k >> 2);
}
// position of `key` in the ascending array keys[0 .. n), or -1
__device__ __forceinline__ long long rc_find(const u64 *__restrict__ keys, long long n, u64 key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && keys[lo] == key) ? lo : -1;
}

// the cell of every point, getVoxelIndex's division, relative to the lattice frame (the host has checked the range from the bbox)
__global__ void __launch_bounds__(256) k_rc_point_keys(const double *__restrict__ xyz, long long n, double h, long long bx, long long by,
                                                       long long bz, u64 *__restrict__ keys) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long cx = (long long) floor(xyz[3 * i] / h), cy = (long long) floor(xyz[3 * i + 1] / h), cz = (long long) floor(xyz[3 * i + 2] / h);
    keys[i] = rc_key(cx - bx, cy - by, cz - bz);
}

// out[i * cnt + j] = keys[i] moved by (off + j) along `axis`; the frame holds every result (the host sized it)
__global__ void __launch_bounds__(256) k_rc_expand(const u64 *__restrict__ keys, long long n, int axis, int off, int cnt, u64 *__restrict__ out) {
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t >= n * cnt) return;
    const u64 k = keys[t / cnt];
    const int j = (int) (t % cnt);
    const u64 lane_mask = 0x1249249249249249ULL << axis;
    const long long c = (long long) compact21(k >> axis) + off + j;
    out[t] = (k & ~lane_mask) | (spread21((u64) c) << axis);
}

__global__ void __launch_bounds__(256) k_rc_heads(const u64 *__restrict__ sorted, long long n, unsigned char *__restrict__ head) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_rc_gather_keys(const u64 *__restrict__ sorted, const unsigned int *__restrict__ idx, long long m,
                                                        u64 *__restrict__ out) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i < m) out[i] = sorted[idx[i]];
}

// cell_ok[i] = the node i is corner 0 of an active cell (a cell and its corner 0 have the same key)
__global__ void __launch_bounds__(256) k_rc_cell_ok(const u64 *__restrict__ nkeys, long long n, const u64 *__restrict__ act, long long n_act,
                                                    unsigned char *__restrict__ cell_ok) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i < n) cell_ok[i] = rc_find(act, n_act, nkeys[i]) >= 0 ? 1 : 0;
}

// ---- the field ----
__global__ void __launch_bounds__(256)
k_recon_field(const u64 *__restrict__ nkeys, long long n, long long bx, long long by, long long bz, double h, const SPoint *__restrict__ sp,
              GridView g, FrameView fr, const double *__restrict__ nrm, double R2, int min_k, double *__restrict__ f_out,
              int *__restrict__ k_out, unsigned char *__restrict__ valid_out, u64 *__restrict__ counters) {
    __shared__ WaveTile s_tile[4];
    __shared__ WaveTile s_nrm[4];
    __shared__ int2 s_tab[4][kGroupTab + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const bool active = i < n;
    double qx = 0, qy = 0, qz = 0;
    if (active) {
        int rx, ry, rz;
        rc_unkey(nkeys[i], rx, ry, rz);
        qx = (double) (bx + rx) * h;
        qy = (double) (by + ry) * h;
        qz = (double) (bz + rz) * h;
    }
    bool pending = active;
    int cx = 0, cy = 0, cz = 0;
    if (pending) {
        const int cell_lim = 1 << (kMortonBits - g.shift);
        const double sc = ldexp(1.0, -g.shift), lim = (double) cell_lim;
        // the cell as a double first: a far node's coordinate does not fit an int
        const double ux = floor(fine_coord(qx, fr.ox, fr.fine_h) * sc), uy = floor(fine_coord(qy, fr.oy, fr.fine_h) * sc),
                     uz = floor(fine_coord(qz, fr.oz, fr.fine_h) * sc);
        if (ux < -1.0 || uy < -1.0 || uz < -1.0 || ux > lim || uy > lim || uz > lim) {
            pending = false;  // more than one cell outside the frame: nothing within R
        } else {
            cx = min(max((int) ux, 0), cell_lim - 1);
            cy = min(max((int) uy, 0), cell_lim - 1);
            cz = min(max((int) uz, 0), cell_lim - 1);
        }
    }
    WaveTile *tile = &s_tile[w], *tn = &s_nrm[w];
    int cnt = 0;
    double W = 0.0, S = 0.0;
    wave_stream_staged(
        pending, cx, cy, cz, sp, g, lane, s_tab[w], tile,
        [&](int j, int pos) {
            const long long o = sp[pos].idx;  // a permutation of [0, n_points)
            const double nx = nrm[3 * o], ny = nrm[3 * o + 1], nz = nrm[3 * o + 2];
            const bool zero = nx == 0.0 && ny == 0.0 && nz == 0.0;
            if (zero || !isfinite(nx) || !isfinite(ny) || !isfinite(nz)) tile->x[j] = NAN;  // never inside the ball
            tn->x[j] = nx;
            tn->y[j] = ny;
            tn->z[j] = nz;
        },
        [&](double px, double py, double pz, int, int j) {
            const double dx = qx - px, dy = qy - py, dz = qz - pz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < R2) {
                const double q = 1.0 - d2 / R2;
                const double wgt = (q * q) * (q * q);
                const double s = (tn->x[j] * dx + tn->y[j] * dy) + tn->z[j] * dz;
                ++cnt;
                W += wgt;
                S += wgt * s;
            }
        });
    const bool valid = active && cnt >= min_k && W > 0.0;
    if (active) {
        f_out[i] = valid ? S / W : 0.0;
        k_out[i] = cnt;
        valid_out[i] = valid ? 1 : 0;
    }
    const long long nv = wave_sum_ll(valid ? 1 : 0), sk = wave_sum_ll((long long) cnt);
    if (lane == 0) {
        if (nv) atomicAdd(&counters[RC_VALID], (u64) nv);
        if (sk) atomicAdd(&counters[RC_SUMK], (u64) sk);
    }
}

// ---- the extraction ----
// nb: int[n][7] position of the node a + dir, or -1; cellx: the cell with corner 0 here is extracted; cmask: bit c = corner c inside
__global__ void __launch_bounds__(256)
k_rc_cells(const u64 *__restrict__ nkeys, long long n, const double *__restrict__ f, const unsigned char *__restrict__ valid,
           const unsigned char *__restrict__ cell_ok, int *__restrict__ nb, unsigned char *__restrict__ cellx, unsigned char *__restrict__ cmask,
           unsigned char *__restrict__ emark, int *__restrict__ tcount, u64 *__restrict__ counters) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int rx, ry, rz;
    rc_unkey(nkeys[i], rx, ry, rz);
    long long cn[8];
    cn[0] = i;
    bool all = valid[i] != 0;
    unsigned int mask = (all && f[i] < 0.0) ? 1u : 0u;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        constexpr int dm[7] = {1, 2, 4, 3, 5, 6, 7};
        const int m = dm[d];
        const long long x = rx + (m & 1), y = ry + ((m >> 1) & 1), z = rz + ((m >> 2) & 1);
        long long j = -1;
        if (x <= kRcMaxRel && y <= kRcMaxRel && z <= kRcMaxRel) j = rc_find(nkeys, n, rc_key(x, y, z));
        nb[i * 7 + d] = (int) j;
        cn[m] = j;
        const bool ok = j >= 0 && valid[j] != 0;
        all = all && ok;
        if (ok && f[j] < 0.0) mask |= 1u << m;
    }
    const bool ext = all && (!cell_ok || cell_ok[i]);
    cellx[i] = ext ? 1 : 0;
    cmask[i] = (unsigned char) (ext ? mask : 0u);
    int nt = 0;
    if (ext) {
        constexpr int md[8] = {0, 0, 1, 3, 2, 4, 5, 6};
        // the 19 Kuhn edges of the cell: every pair of corners u < v with u's bits a subset of v's
#pragma unroll
        for (int u = 0; u < 7; ++u)
#pragma unroll
            for (int v = u + 1; v < 8; ++v)
                if ((u & v) == u && (((mask >> u) ^ (mask >> v)) & 1u)) emark[cn[u] * 7 + md[v ^ u]] = 1;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            unsigned int lm = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) lm |= ((mask >> c_rtab.corner[t][j]) & 1u) << j;
            nt += c_rtab.ntri[t][lm];
        }
        atomicAdd(&counters[RC_CELLS], 1ull);
    }
    tcount[i] = nt;
}

__global__ void k_rc_total(const long long *__restrict__ toff, const int *__restrict__ tcount, long long n, u64 *__restrict__ counters) {
    if (threadIdx.x == 0 && blockIdx.x == 0) counters[RC_NTRI] = (u64) (toff[n - 1] + tcount[n - 1]);
}

// vertex v lies on the edge elist[v] = node * 7 + dir, computed from the edge's origin node whichever end is inside
__global__ void __launch_bounds__(256)
k_rc_vertices(const unsigned int *__restrict__ elist, long long nv, const u64 *__restrict__ nkeys, const int *__restrict__ nb,
              const double *__restrict__ f, long long bx, long long by, long long bz, double h, double *__restrict__ verts,
              int *__restrict__ vedge) {
    const long long v = (long long) blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const unsigned int e = elist[v];
    const long long a = e / 7u;
    const int dir = (int) (e % 7u);
    long long b = nb[a * 7 + dir];  // >= 0: the edge was marked by an extracted cell
    if (b < 0) b = a;
    const double fa = f[a], fb = f[b];
    double t = fa / (fa - fb);
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    int rx, ry, rz;
    rc_unkey(nkeys[a], rx, ry, rz);
    const int m = c_rtab.dir_mask[dir];
    const long long ia[3] = {bx + rx, by + ry, bz + rz};
    const int step[3] = {m & 1, (m >> 1) & 1, (m >> 2) & 1};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double xa = (double) ia[d] * h, xb = (double) (ia[d] + step[d]) * h;
        verts[3 * v + d] = xa + t * (xb - xa);
        vedge[4 * v + d] = (int) ia[d];
    }
    vedge[4 * v + 3] = dir;
}

__device__ __forceinline__ long long rc_find_u32(const unsigned int *__restrict__ a, long long n, unsigned int key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n ? lo : n - 1;  // the key is present: k_rc_cells marked every edge k_rc_emit asks for
}

__global__ void __launch_bounds__(256)
k_rc_emit(long long n, const int *__restrict__ nb, const unsigned char *__restrict__ cellx, const unsigned char *__restrict__ cmask,
          const long long *__restrict__ toff, const unsigned int *__restrict__ elist, long long nv, const double *__restrict__ verts,
          long long nt_total, int *__restrict__ tris, u64 *__restrict__ counters) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !cellx[i]) return;
    const unsigned int mask = cmask[i];
    long long o = toff[i];
    int ndeg = 0;
    for (int t = 0; t < 6; ++t) {
        unsigned int lm = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) lm |= ((mask >> c_rtab.corner[t][j]) & 1u) << j;
        const int nt = c_rtab.ntri[t][lm];
        for (int a = 0; a < nt; ++a, ++o) {
            if (o >= nt_total) return;  // (cannot happen: the offsets are the scan of the same counts)
            int id[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const unsigned int code = c_rtab.tri[t][lm][a][b];
                const unsigned int u = code >> 3, d = code & 7u;
                const long long node = u == 0 ? i : (long long) nb[i * 7 + c_rtab.mask_dir[u]];
                id[b] = (int) rc_find_u32(elist, nv, (unsigned int) (node * 7 + d));
                tris[3 * o + b] = id[b];
            }
            // degenerate as me_mesh_upload counts it: (B - A) x (C - A) is exactly the zero vector
            const double *A = verts + 3 * (long long) id[0], *B = verts + 3 * (long long) id[1], *Cc = verts + 3 * (long long) id[2];
            const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {Cc[0] - A[0], Cc[1] - A[1], Cc[2] - A[2]};
            const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
            if (nx == 0.0 && ny == 0.0 && nz == 0.0) ++ndeg;
        }
    }
    if (ndeg) atomicAdd(&counters[RC_NDEG], (u64) ndeg);
}

// me_isosurface: adjacent equal keys of the sorted node list, and the caller's field in sorted order
__global__ void __launch_bounds__(256)
k_rc_iso_gather(const u64 *__restrict__ sorted, const unsigned int *__restrict__ perm, long long n, const double *__restrict__ f_in,
                const unsigned char *__restrict__ valid_in, double *__restrict__ f, unsigned char *__restrict__ valid, u64 *__restrict__ counters) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i > 0 && sorted[i] == sorted[i - 1]) atomicAdd(&counters[RC_NDUP], 1ull);
    const unsigned int o = perm[i];
    f[i] = f_in[o];
    valid[i] = valid_in[o] ? 1 : 0;
}

inline u64 host_spread21(u64 x) {
    x &= 0x1fffffULL;
    x = (x | x << 32) & 0x1f00000000ffffULL;
    x = (x | x << 16) & 0x1f0000ff0000ffULL;
    x = (x | x << 8) & 0x100f00f00f00f00fULL;
    x = (x | x << 4) & 0x10c30c30c30c30c3ULL;
    x = (x | x << 2) & 0x1249249249249249ULL;
    return x;
}
inline unsigned int host_compact21(u64 x) {
    x &= 0x1249249249249249ULL;
    x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ULL;
    x = (x ^ (x >> 4)) & 0x100f00f00f00f00fULL;
    x = (x ^ (x >> 8)) & 0x1f0000ff0000ffULL;
    x = (x ^ (x >> 16)) & 0x1f00000000ffffULL;
    x = (x ^ (x >> 32)) & 0x1fffffULL;
    return (unsigned int) x;
}

int read_counters(me_ctx *ctx, Recon &R, u64 h[RC_COUNT]) {
    MailGuard mg(ctx);
    ME_TRY(mail_post(ctx, h, R.counters.p, sizeof(u64) * RC_COUNT));
    return mg.sync();
}

// in[0 .. n) -> sorted, unique keys in out[0 .. *m); R.s[4 .. 6] are the scratch of the pass
int sort_unique(me_ctx *ctx, Recon &R, const DevBuf &in, long long n, DevBuf &out, long long *m, const char *who) {
    if (n >= (1LL << 32)) return ctx->fail(ME_ERR_ARG, std::string(who) + ": the lattice has 2^32 or more cells at this voxel size and band");
    DevBuf &sorted = R.s[4], &head = R.s[5], &idx = R.s[6];
    ME_CHECK(ctx, sorted.ensure((size_t) n * 8));
    ME_CHECK(ctx, head.ensure((size_t) n));
    ME_CHECK(ctx, idx.ensure((size_t) n * 4));
    ME_TRY(sort_keys_u64(ctx, in.as<u64>(), sorted.as<u64>(), n, 0, 3 * kMortonBits));
    hipLaunchKernelGGL(k_rc_heads, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, sorted.as<u64>(), n, head.as<unsigned char>());
    unsigned int *cnt = reinterpret_cast<unsigned int *>(R.counters.as<u64>() + RC_NUNIQ);
    ME_TRY(select_flagged_u32(ctx, head.as<unsigned char>(), n, idx.as<unsigned int>(), cnt));
    ME_CHECK(ctx, hipGetLastError());
    unsigned int h = 0;
    {
        MailGuard mg(ctx);
        ME_TRY(mail_post(ctx, &h, cnt, sizeof(h)));
        ME_TRY(mg.sync());
    }
    *m = (long long) h;
    ME_CHECK(ctx, out.ensure((size_t) h * 8));
    hipLaunchKernelGGL(k_rc_gather_keys, dim3(blocks_of(h)), dim3(256), 0, ctx->stream, sorted.as<u64>(), idx.as<unsigned int>(), (long long) h,
                       out.as<u64>());
    ME_CHECK(ctx, hipGetLastError());
    return ME_OK;
}

// keys[0 .. *n) (sorted, unique) moved by off .. off + cnt - 1 along every axis in turn, sorted and unique again; a and b ping-pong
int expand_all_axes(me_ctx *ctx, Recon &R, DevBuf *a, DevBuf *b, long long *n, int off, int cnt, DevBuf **result, const char *who) {
    for (int axis = 0; axis < 3; ++axis) {
        const long long m = *n * cnt;
        if (m >= (1LL << 32)) return ctx->fail(ME_ERR_ARG, std::string(who) + ": the lattice has 2^32 or more cells at this voxel size and band");
        ME_CHECK(ctx, R.s[7].ensure((size_t) m * 8));
        hipLaunchKernelGGL(k_rc_expand, dim3(blocks_of(m)), dim3(256), 0, ctx->stream, a->as<u64>(), *n, axis, off, cnt, R.s[7].as<u64>());
        ME_CHECK(ctx, hipGetLastError());
        ME_TRY(sort_unique(ctx, R, R.s[7], m, *b, n, who));
        std::swap(a, b);
    }
    *result = a;
    return ME_OK;
}

// The extraction stage on the sorted, unique node keys R.node_key[0 .. n) with R.node_f / R.node_valid (and cell_ok, or nullptr: every
// node may be corner 0 of a cell).  Fills R.verts / R.vedge / R.tris and the counts of `out` it owns.
int extract(me_ctx *ctx, Recon &R, long long n, const unsigned char *cell_ok, double h, me_recon_out *out, const char *who) {
    R.nv = R.nt = 0;
    if (n <= 0) return ME_OK;
    if (n * 7 >= (1LL << 32)) return ctx->fail(ME_ERR_ARG, std::string(who) + ": more than 2^32 / 7 nodes");
    DevBuf &nb = R.s[0], &flags = R.s[1], &emark = R.s[2], &tcount = R.s[3], &toff = R.s[4], &elist = R.s[5];
    ME_CHECK(ctx, nb.ensure((size_t) n * 7 * 4));
    ME_CHECK(ctx, flags.ensure((size_t) n * 2));
    ME_CHECK(ctx, emark.ensure((size_t) n * 7));
    ME_CHECK(ctx, tcount.ensure((size_t) n * 4));
    ME_CHECK(ctx, toff.ensure((size_t) n * 8));
    ME_CHECK(ctx, elist.ensure((size_t) n * 7 * 4));
    unsigned char *cellx = flags.as<unsigned char>(), *cmask = cellx + n;
    u64 *cnt = R.counters.as<u64>();
    unsigned int *nvert = reinterpret_cast<unsigned int *>(cnt + RC_NVERT);
    ME_CHECK(ctx, hipMemsetAsync(emark.p, 0, (size_t) n * 7, ctx->stream));
    {
        TimerScope ts(ctx, "recon_extract");
        hipLaunchKernelGGL(k_rc_cells, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, R.node_key.as<u64>(), n, R.node_f.as<double>(),
                           R.node_valid.as<unsigned char>(), cell_ok, nb.as<int>(), cellx, cmask, emark.as<unsigned char>(), tcount.as<int>(), cnt);
        ME_TRY(select_flagged_u32(ctx, emark.as<unsigned char>(), n * 7, elist.as<unsigned int>(), nvert));
        ME_TRY(exclusive_scan_i32_i64(ctx, tcount.as<int>(), toff.as<long long>(), n));
        hipLaunchKernelGGL(k_rc_total, dim3(1), dim3(64), 0, ctx->stream, toff.as<long long>(), tcount.as<int>(), n, cnt);
    }
    ME_CHECK(ctx, hipGetLastError());
    u64 hc[RC_COUNT];
    ME_TRY(read_counters(ctx, R, hc));
    const long long V = (long long) (hc[RC_NVERT] & 0xffffffffULL), T = (long long) hc[RC_NTRI];
    if (V >= (1LL << 31) || T >= (1LL << 31))
        return ctx->fail(ME_ERR_ARG, std::string(who) + ": the surface has 2^31 or more vertices or triangles (" + std::to_string(V) + ", " +
                                         std::to_string(T) + "): use a larger voxel");
    ME_CHECK(ctx, R.verts.ensure((size_t) V * 24));
    ME_CHECK(ctx, R.vedge.ensure((size_t) V * 16));
    ME_CHECK(ctx, R.tris.ensure((size_t) T * 12));
    if (V > 0) {
        TimerScope ts(ctx, "recon_extract");
        hipLaunchKernelGGL(k_rc_vertices, dim3(blocks_of(V)), dim3(256), 0, ctx->stream, elist.as<unsigned int>(), V, R.node_key.as<u64>(),
                           nb.as<int>(), R.node_f.as<double>(), R.base[0], R.base[1], R.base[2], h, R.verts.as<double>(), R.vedge.as<int>());
        hipLaunchKernelGGL(k_rc_emit, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, n, nb.as<int>(), cellx, cmask, toff.as<long long>(),
                           elist.as<unsigned int>(), V, R.verts.as<double>(), T, R.tris.as<int>(), cnt);
    }
    ME_CHECK(ctx, hipGetLastError());
    ME_TRY(read_counters(ctx, R, hc));
    R.nv = V, R.nt = T;
    out->n_cells_extracted = (int64_t) hc[RC_CELLS];
    out->n_vertices = V;
    out->n_triangles = T;
    out->n_degenerate = (int64_t) hc[RC_NDEG];
    return ME_OK;
}

int need_recon_ctx(me_ctx *ctx, const char *who) {
    if (ctx->shard_world != 1 || ctx->slab.axis >= 0) return ctx->fail(ME_ERR_ARG, std::string(who) + ": single GPU only (no slab or shard mode)");
    return ME_OK;
}

}  // namespace

int reconstruct(me_ctx *ctx, int slot, const me_recon_params *p, me_recon_out *out) {
    const char *who = "me_reconstruct";
    if (slot < 0 || slot > 1) return ctx->fail(ME_ERR_ARG, "me_reconstruct: bad slot");
    if (!p || !out) return ctx->fail(ME_ERR_ARG, "me_reconstruct: NULL argument");
    const double h = p->voxel, Rr = p->radius;
    if (!(h > 0) || !std::isfinite(h)) return ctx->fail(ME_ERR_ARG, "me_reconstruct: voxel must be finite and > 0");
    if (!(Rr >= h) || !std::isfinite(Rr) || !std::isfinite(Rr * Rr)) return ctx->fail(ME_ERR_ARG, "me_reconstruct: radius must be finite and >= voxel");
    if (p->min_k < 1) return ctx->fail(ME_ERR_ARG, "me_reconstruct: min_k must be >= 1");
    if (p->band < 0 || p->band > 2) return ctx->fail(ME_ERR_ARG, "me_reconstruct: band must be 0, 1 or 2");
    ME_TRY(need_single_gpu_cloud(ctx, slot, who));
    Cloud &c = ctx->cloud[slot];
    if (!c.have_normals)
        return ctx->fail(ME_ERR_STATE, "me_reconstruct: the slot has no normals (me_radius_normals / me_estimate_normals / me_set_normals)");
    Recon &R = *ctx->recon;
    R.have = R.have_nodes = false;
    std::memset(out, 0, sizeof(*out));
    const int band = (int) p->band;
    // the lattice frame from the bounding box: floor(x / h) is monotone in x
    long long cmin[3], cmax[3];
    for (int d = 0; d < 3; ++d) {
        const double lo = std::floor(c.bbox_lo[d] / h), hi = std::floor(c.bbox_hi[d] / h);
        if (!(std::fabs(lo) < kRcMaxCell) || !(std::fabs(hi) < kRcMaxCell))
            return ctx->fail(ME_ERR_ARG, "me_reconstruct: a cell index floor(p / voxel) does not fit 2^30");
        cmin[d] = (long long) lo, cmax[d] = (long long) hi;
        R.base[d] = cmin[d] - band;
        if (cmax[d] + band + 1 - R.base[d] > kRcMaxRel)
            return ctx->fail(ME_ERR_ARG, "me_reconstruct: the active cells span more than 2^21 - 1 cells on an axis (the 21-bit Morton frame): use a larger voxel");
    }
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    // the slot's index at the level of R (me_m3c2's rule): the 27-cell stencil is exact when the cell edge is >= R
    const double want_h = Rr * (1.0 + 0x1p-20);
    if (!c.index_valid || c.cell_h < want_h || c.cell_h > 1.5 * want_h) {
        const double req = c.cell_size_req;
        ME_TRY(cloud_build_index(ctx, slot, Rr));
        c.cell_size_req = req;
    }
    ME_CHECK(ctx, R.counters.ensure(sizeof(u64) * RC_COUNT));
    ME_CHECK(ctx, hipMemsetAsync(R.counters.p, 0, sizeof(u64) * RC_COUNT, ctx->stream));
    const long long np = c.n;
    if (np <= 0) {
        R.n_nodes = R.nv = R.nt = 0;
        R.have = R.have_nodes = true;
        return ME_OK;
    }
    DevBuf &ka = R.s[8], &kb = R.s[9], &act = R.s[10];
    ME_CHECK(ctx, R.s[7].ensure((size_t) np * 8));
    hipLaunchKernelGGL(k_rc_point_keys, dim3(blocks_of(np)), dim3(256), 0, ctx->stream, c.xyz.as<double>(), np, h, R.base[0], R.base[1], R.base[2],
                       R.s[7].as<u64>());
    ME_CHECK(ctx, hipGetLastError());
    long long n_occ = 0;
    ME_TRY(sort_unique(ctx, R, R.s[7], np, ka, &n_occ, who));
    long long n_act = n_occ;
    DevBuf *cells = &ka;
    if (band > 0) ME_TRY(expand_all_axes(ctx, R, &ka, &kb, &n_act, -band, 2 * band + 1, &cells, who));
    ME_CHECK(ctx, act.ensure((size_t) n_act * 8));
    ME_CHECK(ctx, hipMemcpyAsync(act.p, cells->p, (size_t) n_act * 8, hipMemcpyDeviceToDevice, ctx->stream));
    long long n = n_act;
    DevBuf *nodes = nullptr;
    ME_TRY(expand_all_axes(ctx, R, cells, cells == &ka ? &kb : &ka, &n, 0, 2, &nodes, who));
    if (n * 7 >= (1LL << 32)) return ctx->fail(ME_ERR_ARG, "me_reconstruct: more than 2^32 / 7 nodes: use a larger voxel");
    ME_CHECK(ctx, R.node_key.ensure((size_t) n * 8));
    ME_CHECK(ctx, R.node_f.ensure((size_t) n * 8));
    ME_CHECK(ctx, R.node_k.ensure((size_t) n * 4));
    ME_CHECK(ctx, R.node_valid.ensure((size_t) n));
    ME_CHECK(ctx, R.cell_ok.ensure((size_t) n));
    ME_CHECK(ctx, hipMemcpyAsync(R.node_key.p, nodes->p, (size_t) n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_rc_cell_ok, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, R.node_key.as<u64>(), n, act.as<u64>(), n_act,
                       R.cell_ok.as<unsigned char>());
    {
        TimerScope ts(ctx, "recon_field");
        const FrameView fr{c.origin[0], c.origin[1], c.origin[2], c.fine_h};
        hipLaunchKernelGGL(k_recon_field, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, R.node_key.as<u64>(), n, R.base[0], R.base[1], R.base[2], h,
                           c.sp.as<SPoint>(), c.grid, fr, c.normals.as<double>(), Rr * Rr, (int) p->min_k, R.node_f.as<double>(),
                           R.node_k.as<int>(), R.node_valid.as<unsigned char>(), R.counters.as<u64>());
    }
    ME_CHECK(ctx, hipGetLastError());
    R.n_nodes = n;
    R.voxel = h;
    out->n_occupied_cells = n_occ;
    out->n_active_cells = n_act;
    out->n_nodes = n;
    ME_TRY(extract(ctx, R, n, R.cell_ok.as<unsigned char>(), h, out, who));
    u64 hc[RC_COUNT];
    ME_TRY(read_counters(ctx, R, hc));
    out->n_valid_nodes = (int64_t) hc[RC_VALID];
    out->sum_k = (int64_t) hc[RC_SUMK];
    R.have = R.have_nodes = true;
    return ME_OK;
}

int isosurface(me_ctx *ctx, const int32_t *node_ijk, const double *f, const uint8_t *valid, long long n, double voxel, me_recon_out *out) {
    const char *who = "me_isosurface";
    if (!out || n < 0 || (n > 0 && (!node_ijk || !f || !valid))) return ctx->fail(ME_ERR_ARG, "me_isosurface: NULL argument or a negative node count");
    if (!(voxel > 0) || !std::isfinite(voxel)) return ctx->fail(ME_ERR_ARG, "me_isosurface: voxel must be finite and > 0");
    ME_TRY(need_recon_ctx(ctx, who));
    if (n * 7 >= (1LL << 32)) return ctx->fail(ME_ERR_ARG, "me_isosurface: more than 2^32 / 7 nodes");
    Recon &R = *ctx->recon;
    R.have = R.have_nodes = false;
    std::memset(out, 0, sizeof(*out));
    long long lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, n_valid = 0;
    for (long long i = 0; i < n; ++i) {
        for (int d = 0; d < 3; ++d) {
            const long long v = node_ijk[3 * i + d];
            if (i == 0 || v < lo[d]) lo[d] = v;
            if (i == 0 || v > hi[d]) hi[d] = v;
        }
        if (valid[i]) {
            if (!std::isfinite(f[i])) return ctx->fail(ME_ERR_ARG, "me_isosurface: a valid node has a non-finite f");
            ++n_valid;
        }
    }
    for (int d = 0; d < 3; ++d) {
        if (hi[d] - lo[d] > kRcMaxRel) return ctx->fail(ME_ERR_ARG, "me_isosurface: the nodes span more than 2^21 - 1 on an axis (the 21-bit Morton frame)");
        R.base[d] = lo[d];
    }
    out->n_nodes = n;
    out->n_valid_nodes = n_valid;
    R.n_nodes = n, R.voxel = voxel, R.nv = R.nt = 0;
    if (n == 0) {
        R.have = true;
        return ME_OK;
    }
    std::vector<u64> keys((size_t) n);
    std::vector<unsigned int> iota((size_t) n);
    for (long long i = 0; i < n; ++i) {
        keys[(size_t) i] = host_spread21((u64) (node_ijk[3 * i] - lo[0])) | (host_spread21((u64) (node_ijk[3 * i + 1] - lo[1])) << 1) |
                           (host_spread21((u64) (node_ijk[3 * i + 2] - lo[2])) << 2);
        iota[(size_t) i] = (unsigned int) i;
    }
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    ME_CHECK(ctx, R.counters.ensure(sizeof(u64) * RC_COUNT));
    ME_CHECK(ctx, hipMemsetAsync(R.counters.p, 0, sizeof(u64) * RC_COUNT, ctx->stream));
    DevBuf &k_in = R.s[7], &i_in = R.s[8], &perm = R.s[9], &f_in = R.s[10], &v_in = R.s[6];
    ME_CHECK(ctx, k_in.ensure((size_t) n * 8));
    ME_CHECK(ctx, i_in.ensure((size_t) n * 4));
    ME_CHECK(ctx, perm.ensure((size_t) n * 4));
    ME_CHECK(ctx, f_in.ensure((size_t) n * 8));
    ME_CHECK(ctx, v_in.ensure((size_t) n));
    ME_CHECK(ctx, R.node_key.ensure((size_t) n * 8));
    ME_CHECK(ctx, R.node_f.ensure((size_t) n * 8));
    ME_CHECK(ctx, R.node_valid.ensure((size_t) n));
    ME_TRY(copy_h2d(ctx, k_in.p, keys.data(), (size_t) n * 8));
    ME_TRY(copy_h2d(ctx, i_in.p, iota.data(), (size_t) n * 4));
    ME_TRY(copy_h2d(ctx, f_in.p, f, (size_t) n * 8));
    ME_TRY(copy_h2d(ctx, v_in.p, valid, (size_t) n));
    ME_TRY(sort_pairs_u64_u32(ctx, k_in.as<u64>(), R.node_key.as<u64>(), i_in.as<unsigned int>(), perm.as<unsigned int>(), n, 0, 3 * kMortonBits));
    hipLaunchKernelGGL(k_rc_iso_gather, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, R.node_key.as<u64>(), perm.as<unsigned int>(), n,
                       f_in.as<double>(), v_in.as<unsigned char>(), R.node_f.as<double>(), R.node_valid.as<unsigned char>(), R.counters.as<u64>());
    ME_CHECK(ctx, hipGetLastError());
    u64 hc[RC_COUNT];
    ME_TRY(read_counters(ctx, R, hc));  // (also: the host vectors and the caller's arrays have been read)
    if (hc[RC_NDUP] != 0) return ctx->fail(ME_ERR_ARG, "me_isosurface: a node occurs more than once");
    ME_TRY(extract(ctx, R, n, nullptr, voxel, out, who));
    R.have = true;
    return ME_OK;
}

int reconstruct_fetch(me_ctx *ctx, double *vertices, int32_t *vertex_edge, int32_t *triangles) {
    ME_TRY(need_recon_ctx(ctx, "me_reconstruct_fetch"));
    Recon &R = *ctx->recon;
    if (!R.have) return ctx->fail(ME_ERR_STATE, "me_reconstruct_fetch: no reconstruction (me_reconstruct / me_isosurface)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    if (vertices) ME_TRY(copy_d2h(ctx, vertices, R.verts.p, (size_t) R.nv * 24));
    if (vertex_edge) ME_TRY(copy_d2h(ctx, vertex_edge, R.vedge.p, (size_t) R.nv * 16));
    if (triangles) ME_TRY(copy_d2h(ctx, triangles, R.tris.p, (size_t) R.nt * 12));
    return ME_OK;
}

int reconstruct_nodes_fetch(me_ctx *ctx, int32_t *node_ijk, double *f, int32_t *k, uint8_t *valid) {
    ME_TRY(need_recon_ctx(ctx, "me_reconstruct_nodes_fetch"));
    Recon &R = *ctx->recon;
    if (!R.have || !R.have_nodes)
        return ctx->fail(ME_ERR_STATE, "me_reconstruct_nodes_fetch: no node field (me_reconstruct; me_isosurface keeps none)");
    ME_CHECK(ctx, hipSetDevice(ctx->device));
    const long long n = R.n_nodes;
    if (node_ijk) {
        std::vector<u64> keys((size_t) n);
        ME_TRY(copy_d2h(ctx, keys.data(), R.node_key.p, (size_t) n * 8));
        for (long long i = 0; i < n; ++i)
            for (int d = 0; d < 3; ++d) node_ijk[3 * i + d] = (int32_t) (R.base[d] + (long long) host_compact21(keys[(size_t) i] >> d));
    }
    if (f) ME_TRY(copy_d2h(ctx, f, R.node_f.p, (size_t) n * 8));
    if (k) ME_TRY(copy_d2h(ctx, k, R.node_k.p, (size_t) n * 4));
    if (valid) ME_TRY(copy_d2h(ctx, valid, R.node_valid.p, (size_t) n));
    return ME_OK;
}

int reconstruct_install(me_ctx *ctx) {
    ME_TRY(need_recon_ctx(ctx, "me_reconstruct_install"));
    Recon &R = *ctx->recon;
    if (!R.have || R.nt < 1) return ctx->fail(ME_ERR_STATE, "me_reconstruct_install: no reconstruction with at least one triangle");
    std::vector<double> v((size_t) R.nv * 3);
    std::vector<int32_t> t((size_t) R.nt * 3);
    ME_TRY(reconstruct_fetch(ctx, v.data(), nullptr, t.data()));
    return mesh_upload(ctx, v.data(), R.nv, t.data(), R.nt, nullptr);
}

void reconstruct_drop(me_ctx *ctx) {
    Recon &R = *ctx->recon;
    R.have = R.have_nodes = false;
    R.verts.release(), R.vedge.release(), R.tris.release();
    R.node_key.release(), R.node_f.release(), R.node_k.release(), R.node_valid.release(), R.cell_ok.release(), R.counters.release();
    for (DevBuf &b : R.s) b.release();
}

}  // namespace me
