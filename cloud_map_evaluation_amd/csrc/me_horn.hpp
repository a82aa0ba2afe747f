// me_horn.hpp — the rigid fit shared by the host (host/map_eval.cpp: point-to-point ICP) and the device (me_globreg.hip: the RANSAC
// hypotheses): a symmetric Jacobi eigen-decomposition and Horn's quaternion method.  Plain arithmetic, no library call but sqrt /
// fabs, so that tests/_globreg_ref.py restates it operation by operation (the device file is compiled with -ffp-contract=off; the
// host build targets x86-64 without FMA, so neither contracts).
//   jacobi_sym: cyclic sweeps over (p, q) = (0,1), (0,2), ... (n-2,n-1) in that order; a sweep starts with the sum of the squared
//   upper off-diagonal entries (row by row) and the decomposition stops when that sum is < 1e-300, or after 100 sweeps.  A zero
//   entry is skipped.  Eigenvalues in d, eigenvectors in the columns of V.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define ME_HD __host__ __device__
#else
#define ME_HD
#endif

namespace me {

ME_HD inline void jacobi_sym(int n, double *a, double *d, double *V) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[n * i + j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) off += a[n * p + q] * a[n * p + q];
        if (off < 1e-300) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[n * p + q];
                if (apq == 0.0) continue;
                const double theta = (a[n * q + q] - a[n * p + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = a[n * k + p], akq = a[n * k + q];
                    a[n * k + p] = c * akp - sn * akq;
                    a[n * k + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = a[n * p + k], aqk = a[n * q + k];
                    a[n * p + k] = c * apk - sn * aqk;
                    a[n * q + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[n * k + p], vkq = V[n * k + q];
                    V[n * k + p] = c * vkp - sn * vkq;
                    V[n * k + q] = sn * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < n; ++i) d[i] = a[n * i + i];
}

// Horn's closed form from S = sum (p - pb)(q - qb)^T (row-major 3x3): the rotation R (row-major) that maximises tr(R S^T), i.e. the
// rotation of Eigen::umeyama without scaling.  The eigenvector of the largest eigenvalue (first index on a tie) is the quaternion.
ME_HD inline void horn_rotation(const double S[9], double R[9]) {
    double N[16] = {S[0] + S[4] + S[8], S[5] - S[7],        S[6] - S[2],         S[1] - S[3],
                    S[5] - S[7],        S[0] - S[4] - S[8], S[1] + S[3],         S[6] + S[2],
                    S[6] - S[2],        S[1] + S[3],        -S[0] + S[4] - S[8], S[5] + S[7],
                    S[1] - S[3],        S[6] + S[2],        S[5] + S[7],         -S[0] - S[4] + S[8]};
    double d[4], V[16];
    jacobi_sym(4, N, d, V);
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (d[i] > d[best]) best = i;
    const double w = V[best], x = V[4 + best], y = V[8 + best], z = V[12 + best];
    R[0] = w * w + x * x - y * y - z * z;
    R[1] = 2 * (x * y - w * z);
    R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z);
    R[4] = w * w - x * x + y * y - z * z;
    R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y);
    R[7] = 2 * (y * z + w * x);
    R[8] = w * w - x * x - y * y + z * z;
}

// the rigid transform of three pairs p_j -> q_j: pb = ((p0 + p1) + p2) / 3 (likewise qb), S_rc = ((a0 + a1) + a2) with
// a_j = (p_jr - pb_r)(q_jc - qb_c), R = horn_rotation(S), t_r = qb_r - ((R_r0 pb_0 + R_r1 pb_1) + R_r2 pb_2).  T = [R | t], 3 x 4 row-major.
ME_HD inline void horn_fit3(const double p[9], const double q[9], double T[12]) {
    double pb[3], qb[3], S[9], R[9];
    for (int k = 0; k < 3; ++k) {
        pb[k] = ((p[k] + p[3 + k]) + p[6 + k]) / 3.0;
        qb[k] = ((q[k] + q[3 + k]) + q[6 + k]) / 3.0;
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            S[3 * r + c] = ((p[r] - pb[r]) * (q[c] - qb[c]) + (p[3 + r] - pb[r]) * (q[3 + c] - qb[c])) + (p[6 + r] - pb[r]) * (q[6 + c] - qb[c]);
    horn_rotation(S, R);
    for (int r = 0; r < 3; ++r) {
        T[4 * r] = R[3 * r];
        T[4 * r + 1] = R[3 * r + 1];
        T[4 * r + 2] = R[3 * r + 2];
        T[4 * r + 3] = qb[r] - ((R[3 * r] * pb[0] + R[3 * r + 1] * pb[1]) + R[3 * r + 2] * pb[2]);
    }
}

}  // namespace me
