// me_stat.hpp — the per-point predicate of the AC / COM / CD statistics (getDiffRegResultWithCorrespondence, map_eval.cpp:1069-1145):
// the correspondence gate and the five truncation thresholds.  Shared by the whole-cloud sums (k_nn_partial / k_nn_sigma, me_nn.hip)
// and the per-voxel breakdown (k_voxm_records, me_voxel.hip), so that a voxel's row counts exactly the points the cloud's sums count.
#pragma once

#include <cmath>

#include "me_internal.hpp"

namespace me {

struct StatParams {
    double gate;      // threshold on d2 (already squared if the mode says so); < 0 = no gate
    int gate_strict;  // 1: d2 < gate, 0: d2 <= gate
    double t2max[5];  // largest d2 whose correctly rounded sqrt is <= trunc[k]
};

#ifdef __HIPCC__
__device__ __forceinline__ bool gate_pass(const StatParams &sp, double d2) {
    if (sp.gate < 0) return true;
    return sp.gate_strict ? (d2 < sp.gate) : (d2 <= sp.gate);
}
#endif

// The largest double x with sqrt_rn(x) <= t (-1 when t is not >= 0): a device compares d2 against it, so that a count of "distance <= t"
// does not depend on the device's sqrt rounding.  me_sqrt_threshold; the thresholds of make_params and of me_errdist.hip.
inline double sqrt_threshold(double t) {
    if (!(t >= 0)) return -1.0;
    double x = t * t;
    while (std::sqrt(std::nextafter(x, INFINITY)) <= t) x = std::nextafter(x, INFINITY);
    while (x > 0 && std::sqrt(x) > t) x = std::nextafter(x, -INFINITY);
    return x;
}

inline StatParams make_params(double gate, int gate_mode, const double trunc[5]) {
    StatParams sp;
    if (gate < 0) {
        sp.gate = -1.0;
        sp.gate_strict = 0;
    } else if (gate_mode == ME_GATE_LT_SQUARED) {
        sp.gate = gate * gate;
        sp.gate_strict = 1;
    } else {
        sp.gate = gate;
        sp.gate_strict = 0;
    }
    for (int k = 0; k < 5; ++k) sp.t2max[k] = sqrt_threshold(trunc ? trunc[k] : 0.0);
    return sp;
}

}  // namespace me
