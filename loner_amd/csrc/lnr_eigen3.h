// open3d's FastEigen3x3 for the smallest eigenvalue of a symmetric 3x3, shared by the normals of lnr_icp.hip and the plane refit of
// lnr_cloud_segment.hip.  Both sources are compiled with -ffp-contract=off (build.py EXACT): every fp64 expression below rounds
// operation by operation.  Everything is internal to its translation unit (the anonymous namespace).
#pragma once
#include "lnr_cloud_grid.h"

namespace {

__device__ inline void cross3(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// open3d's ComputeEigenvector0: the row cross product of largest norm, normalised
__device__ inline void eigvec0(const double A[3][3], double e, double out[3]) {
    const double r0[3] = {A[0][0] - e, A[0][1], A[0][2]}, r1[3] = {A[0][1], A[1][1] - e, A[1][2]}, r2[3] = {A[0][2], A[1][2], A[2][2] - e};
    double c01[3], c02[3], c12[3];
    cross3(r0, r1, c01);
    cross3(r0, r2, c02);
    cross3(r1, r2, c12);
    const double d0 = dot3(c01, c01), d1 = dot3(c02, c02), d2 = dot3(c12, c12);
    double dmax = d0;
    int imax = 0;
    if (d1 > dmax) { dmax = d1; imax = 1; }
    if (d2 > dmax) imax = 2;
    const double* v = imax == 0 ? c01 : (imax == 1 ? c02 : c12);
    const double s = sqrt(imax == 0 ? d0 : (imax == 1 ? d1 : d2));
    for (int a = 0; a < 3; ++a) out[a] = v[a] / s;
}

// open3d's ComputeEigenvector1: the eigenvector of e1 in the plane orthogonal to evec0
__device__ inline void eigvec1(const double A[3][3], const double v0[3], double e1, double out[3]) {
    double U[3], V[3];
    if (fabs(v0[0]) > fabs(v0[1])) {
        const double inv = 1.0 / sqrt(v0[0] * v0[0] + v0[2] * v0[2]);
        U[0] = -v0[2] * inv; U[1] = 0.0; U[2] = v0[0] * inv;
    } else {
        const double inv = 1.0 / sqrt(v0[1] * v0[1] + v0[2] * v0[2]);
        U[0] = 0.0; U[1] = v0[2] * inv; U[2] = -v0[1] * inv;
    }
    cross3(v0, U, V);
    double AU[3], AV[3];
    for (int a = 0; a < 3; ++a) {
        const double row[3] = {A[0][a], A[1][a], A[2][a]};     // A is symmetric
        AU[a] = dot3(row, U);
        AV[a] = dot3(row, V);
    }
    double m00 = dot3(U, AU) - e1, m01 = dot3(U, AV), m11 = dot3(V, AV) - e1;
    const double a00 = fabs(m00), a01 = fabs(m01), a11 = fabs(m11);
    double cu, cv;                                             // out = cu U - cv V
    if (a00 >= a11) {
        if (fmax(a00, a01) > 0.0) {
            if (a00 >= a01) { m01 = m01 / m00; m00 = 1.0 / sqrt(1.0 + m01 * m01); m01 = m01 * m00; }
            else { m00 = m00 / m01; m01 = 1.0 / sqrt(1.0 + m00 * m00); m00 = m00 * m01; }
            cu = m01; cv = m00;
        } else { cu = 1.0; cv = 0.0; }
    } else {
        if (fmax(a11, a01) > 0.0) {
            if (a11 >= a01) { m01 = m01 / m11; m11 = 1.0 / sqrt(1.0 + m01 * m01); m01 = m01 * m11; }
            else { m11 = m11 / m01; m01 = 1.0 / sqrt(1.0 + m11 * m11); m11 = m11 * m01; }
            cu = m11; cv = m01;
        } else { cu = 1.0; cv = 0.0; }
    }
    for (int a = 0; a < 3; ++a) out[a] = cu * U[a] - cv * V[a];
}

// open3d's FastEigen3x3 (robust closed form, geometrictools' RobustEigenSymmetric3x3): the unit eigenvector of the smallest eigenvalue
// of the symmetric C; (0, 0, 1) for an all-zero C (EstimateNormals' rule for a zero normal)
__device__ inline void normal_of(const double C[3][3], double n[3]) {
    double mx = C[0][0];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) mx = fmax(mx, C[a][b]);
    n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
    if (mx == 0.0) return;
    double A[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) A[a][b] = C[a][b] / mx;
    const double norm = (A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[1][2] * A[1][2];
    if (norm > 0.0) {
        const double q = ((A[0][0] + A[1][1]) + A[2][2]) / 3.0;
        const double b00 = A[0][0] - q, b11 = A[1][1] - q, b22 = A[2][2] - q;
        const double p = sqrt(((((b00 * b00 + b11 * b11) + b22 * b22) + norm * 2.0)) / 6.0);
        const double c00 = b11 * b22 - A[1][2] * A[1][2];
        const double c01 = A[0][1] * b22 - A[1][2] * A[0][2];
        const double c02 = A[0][1] * A[1][2] - b11 * A[0][2];
        const double det = ((b00 * c00 - A[0][1] * c01) + A[0][2] * c02) / ((p * p) * p);
        const double half_det = fmin(fmax(det * 0.5, -1.0), 1.0);
        const double angle = acos(half_det) / 3.0;
        const double two_thirds_pi = 2.09439510239319549;
        const double beta2 = cos(angle) * 2.0;
        const double beta0 = cos(angle + two_thirds_pi) * 2.0;
        const double beta1 = -(beta0 + beta2);
        const double ev0 = q + p * beta0, ev1 = q + p * beta1, ev2 = q + p * beta2;
        double v0[3], v1[3];
        if (half_det >= 0.0) {
            eigvec0(A, ev2, v0);                               // evec2
            if (ev2 < ev0 && ev2 < ev1) { for (int a = 0; a < 3; ++a) n[a] = v0[a]; return; }
            eigvec1(A, v0, ev1, v1);
            if (ev1 < ev0 && ev1 < ev2) { for (int a = 0; a < 3; ++a) n[a] = v1[a]; return; }
            cross3(v1, v0, n);                                 // evec1 x evec2
        } else {
            eigvec0(A, ev0, v0);                               // evec0
            if (ev0 < ev1 && ev0 < ev2) { for (int a = 0; a < 3; ++a) n[a] = v0[a]; return; }
            eigvec1(A, v0, ev1, v1);
            if (ev1 < ev0 && ev1 < ev2) { for (int a = 0; a < 3; ++a) n[a] = v1[a]; return; }
            cross3(v0, v1, n);                                 // evec0 x evec1
        }
    } else {
        n[2] = 0.0;
        if (C[0][0] < C[1][1] && C[0][0] < C[2][2]) n[0] = 1.0;
        else if (C[1][1] < C[0][0] && C[1][1] < C[2][2]) n[1] = 1.0;
        else n[2] = 1.0;
    }
}

}  // namespace
