// me_philox.hpp — counter-based randomness shared by the device passes: Philox4x64-10 (Salmon et al., SC'11; Random123
// philox4x64_R with R = 10), key (seed, 0).  Counter word 1 names the user (include/mapeval_hip.h): 1-3 me_perturb_cloud,
// 4 me_global_register, 5 me_segment_planes, 6 me_mesh_scan (range noise).
#pragma once

#include <hip/hip_runtime.h>

namespace me {

typedef unsigned long long u64;

__device__ __forceinline__ void philox4x64_10(u64 c[4], u64 k0, u64 k1) {
    const u64 M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
    const u64 W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) {
            k0 += W0;
            k1 += W1;
        }
        const u64 hi0 = __umul64hi(M0, c[0]), lo0 = M0 * c[0];
        const u64 hi1 = __umul64hi(M1, c[2]), lo1 = M1 * c[2];
        const u64 n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
    }
}

__device__ __forceinline__ void philox_block(u64 seed, u64 c0, u64 c1, u64 c2, u64 w[4]) {
    w[0] = c0;
    w[1] = c1;
    w[2] = c2;
    w[3] = 0;
    philox4x64_10(w, seed, 0);
}

__device__ __forceinline__ double u01(u64 w) { return (double) (w >> 11) * 0x1p-53; }          // [0, 1)
__device__ __forceinline__ double u01_open0(u64 w) { return (double) ((w >> 11) + 1) * 0x1p-53; }  // (0, 1]

// floor(w n / 2^64): an index in [0, n) from a 64-bit word (the high word of the 128-bit product)
__device__ __forceinline__ u64 mulhi64(u64 w, u64 n) { return __umul64hi(w, n); }

}  // namespace me
