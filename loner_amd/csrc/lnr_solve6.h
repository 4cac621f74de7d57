// The 6x6 solve and the 6-vector-to-matrix rule shared by the ICP entry points (lnr_icp.hip) and the pose graph (lnr_pose_graph.hip):
// one statement of each, so that a pose-graph step moves a pose exactly as an ICP round moves a cloud.  Both files are compiled with
// -ffp-contract=off (build.py EXACT).  Everything is internal to its translation unit (the anonymous namespace).
#pragma once
#include <float.h>
#include <math.h>

namespace {

// Eigen's LDLT (symmetric pivoting on the largest remaining |diagonal|, first index on ties; left-looking columns) and its solve with the
// pseudo-inverse of D (|D_i| <= DBL_MIN gives a zero component), for A x = b.  A is overwritten.  Every loop is unrolled and every
// runtime index (the pivot) becomes a compare against a static one, so that A stays in registers.
__device__ inline void swap_if(bool c, double& a, double& b) {
    const double t = a;
    a = c ? b : a;
    b = c ? t : b;
}

__device__ inline void ldlt_solve6(double A[6][6], const double b_in[6], double x[6]) {
    int perm[6] = {0, 1, 2, 3, 4, 5};
    bool stop = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (stop) continue;
        int p = k;
        double big = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i)
            if (fabs(A[i][i]) > big) { big = fabs(A[i][i]); p = i; }
        perm[k] = p;
#pragma unroll
        for (int q = k + 1; q < 6; ++q) {                   // the symmetric swap of rows and columns k and p
            const bool c = q == p;
#pragma unroll
            for (int j = 0; j < 6; ++j) swap_if(c, A[k][j], A[q][j]);
#pragma unroll
            for (int j = 0; j < 6; ++j) swap_if(c, A[j][k], A[j][q]);
        }
        if (k > 0) {
            double temp[6];
#pragma unroll
            for (int j = 0; j < k; ++j) temp[j] = A[j][j] * A[k][j];
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < k; ++j) s = s + A[k][j] * temp[j];
            A[k][k] = A[k][k] - s;
#pragma unroll
            for (int i = k + 1; i < 6; ++i) {
                double t = 0.0;
#pragma unroll
                for (int j = 0; j < k; ++j) t = t + A[i][j] * temp[j];
                A[i][k] = A[i][k] - t;
            }
        }
        const double akk = A[k][k];
        if (k == 0 && !(fabs(akk) > 0.0)) {                 // an all-zero diagonal: nothing is factored
            perm[0] = 0;
            stop = true;
            continue;
        }
        if (fabs(akk) > 0.0) {
#pragma unroll
            for (int i = k + 1; i < 6; ++i) A[i][k] = A[i][k] / akk;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] = b_in[i];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int q = k + 1; q < 6; ++q) swap_if(perm[k] == q, y[k], y[q]);
#pragma unroll
    for (int i = 0; i < 6; ++i) {                           // L (unit lower)
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < i; ++j) s = s + A[i][j] * y[j];
        y[i] = y[i] - s;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] = fabs(A[i][i]) > DBL_MIN ? y[i] / A[i][i] : 0.0;
#pragma unroll
    for (int i = 5; i >= 0; --i) {                          // L^T
        double s = 0.0;
#pragma unroll
        for (int j = i + 1; j < 6; ++j) s = s + A[j][i] * y[j];
        y[i] = y[i] - s;
    }
#pragma unroll
    for (int k = 5; k >= 0; --k)
#pragma unroll
        for (int q = k + 1; q < 6; ++q) swap_if(perm[k] == q, y[k], y[q]);
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = y[i];
}

// TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0), t = x[3:6]
__device__ inline void step_matrix(const double x[6], double U[16]) {
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cc = cos(x[2]), sc = sin(x[2]);
    U[0] = cc * cb; U[1] = (cc * sb) * sa - sc * ca; U[2] = (cc * sb) * ca + sc * sa; U[3] = x[3];
    U[4] = sc * cb; U[5] = (sc * sb) * sa + cc * ca; U[6] = (sc * sb) * ca - cc * sa; U[7] = x[4];
    U[8] = -sb;     U[9] = cb * sa;                  U[10] = cb * ca;                 U[11] = x[5];
    U[12] = 0.0; U[13] = 0.0; U[14] = 0.0; U[15] = 1.0;
}

}  // namespace
