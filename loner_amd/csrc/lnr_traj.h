// The pose of a sensor trajectory at a time stamp, shared by lnr_cloud_tools.hip (lnr_cloud_trajectory_transform moves points) and
// lnr_raycast.hip (lnr_trajectory_rays turns directions): the knot search, the interpolation weight, the scaled rotation vector,
// Rodrigues' formula and R_k E, as include/loner_hip.h states every rounding.  Both sources are compiled with -ffp-contract=off
// (build.py EXACT).  The two entries differ in their sine and cosine only, which is traj_pose's template parameter.
// Everything is internal to its translation unit (the anonymous namespace), like the kernels that use it.
#pragma once
#include "lnr_cloud_grid.h"

namespace {

struct TrajView {
    const double* __restrict__ T;       // [K] times
    const double* __restrict__ P;       // [K,3] positions
    const double* __restrict__ R;       // [K,9] rotations, row-major
    const double* __restrict__ W;       // [K-1,3] log(R_k^T R_k+1)
    uint32_t K;
};

// the pose at tau in [T_0, T_K-1]: R = R_k E(alpha W_k) row-major, trans = P_k + alpha (P_k+1 - P_k).  SinCos(theta, &sin, &cos), theta > 0
template <void (*SinCos)(double, double*, double*)>
__device__ inline void traj_pose(const TrajView& tv, double tau, double* R, double* trans) {
    uint32_t lo = 0, hi = tv.K;                                 // the first knot above tau
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (tv.T[mid] <= tau) lo = mid + 1; else hi = mid;
    }
    const uint32_t k = lo - 1 < tv.K - 2 ? lo - 1 : tv.K - 2;   // T_0 <= tau: lo >= 1
    const double alpha = (tau - tv.T[k]) / (tv.T[k + 1] - tv.T[k]);
    const double *Pk = tv.P + 3 * (size_t)k, *Rk = tv.R + 9 * (size_t)k, *Wk = tv.W + 3 * (size_t)k;
    const double wx = alpha * Wk[0], wy = alpha * Wk[1], wz = alpha * Wk[2];
    const double theta = sqrt((wx * wx + wy * wy) + wz * wz);
    if (theta < 1e-9) {
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = Rk[e];
    } else {
        const double ax = wx / theta, ay = wy / theta, az = wz / theta;
        double s, cs;
        SinCos(theta, &s, &cs);
        const double v = 1.0 - cs;
        // Rodrigues: I + s K + v K^2, as lnr_motion_compensate writes it
        const double E[9] = {1.0 - v * (ay * ay + az * az), v * ax * ay - s * az, v * ax * az + s * ay,
                             v * ax * ay + s * az, 1.0 - v * (ax * ax + az * az), v * ay * az - s * ax,
                             v * ax * az - s * ay, v * ay * az + s * ax, 1.0 - v * (ax * ax + ay * ay)};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) R[3 * a + b] = (Rk[3 * a] * E[b] + Rk[3 * a + 1] * E[3 + b]) + Rk[3 * a + 2] * E[6 + b];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) trans[a] = Pk[a] + alpha * (Pk[3 + a] - Pk[a]);
}

}  // namespace
