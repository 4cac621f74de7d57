// Normals of a point cloud and point-to-plane ICP between two (gfx950), on the nearest-neighbour grid of lnr_cloud.hip.
//
// Replaces the open3d calls of analysis/evaluate_lidar_map.py:23-53 and of the tracker:
//   PointCloud.estimate_normals(KDTreeSearchParamKNN), registration_icp(TransformationEstimationPointToPlane)
// with the definitions stated in include/loner_hip.h ("normals and point-to-plane ICP").  This file is compiled with -ffp-contract=off
// (build.py EXACT): every fp64 expression below rounds operation by operation, as the numpy restatement (tests/icp_restatement.py)
// does.  The grid, its shell walk and its exact pass are lnr_cloud_grid.h's; ties are ordered by (d2, input index) everywhere.
//   kNN        (lnr_cloud_knn.h, shared with the outlier filter of lnr_cloud_tools.hip) one query per thread walks the shells with its
//              k best pairs in a 32-slot list of statically indexed registers (an unrolled insertion) and stops when the k-th best
//              lies strictly below the bound on every unvisited cell; queries still open after NN_MAX_SHELL shells take the exact
//              pass; what happens to a finished list is the caller's Finish (here NormalsFinish)
//   normals    the cumulant covariance of the neighbours in list order, then open3d's FastEigen3x3 (the robust closed form): the unit
//              eigenvector of the smallest eigenvalue, in the same launch
//   ICP        per round: icp_corr finds each source's nearest target within r and sums its 21 JTJ, 6 JTr, d2 and count terms per
//              thread, then per block in a fixed order; icp_fold (one workgroup) sums the partials, forms fitness and RMSE and tests
//              convergence; icp_solve (one thread) does Eigen's pivoted LDLT, Rz Ry Rx and update @ transformation; the working
//              source then moves by the update where the device computed it.  No float atomics: two runs are bit-identical.  Every
//              round is enqueued at once; the state's done word makes later rounds return, and the host reads the result once
//   robust,    icp_corr_w is icp_corr<true> with one weight per correspondence (Huber, Cauchy, Tukey) and, for generalized ICP, with
//   generalized   the plane-to-plane system: M = C_t + R C_s R^T from the accumulated rotation, its cofactor inverse W, J^T W J and
//              J^T W d in the same 29 slots ("robust kernels and generalized ICP" in the header; tests/gicp_restatement.py).  The
//              fold, the solve, the state machine and the host driver (icp_run) are shared; lnr_icp_point_to_plane still launches
//              icp_corr<true>
#include "lnr_cloud_knn.h"
#include "lnr_eigen3.h"
#include "lnr_solve6.h"

namespace {

// ------------------------------------------------------------------------------------------------ k nearest neighbours and normals
// lnr_cloud_knn.h's Finish: the covariance of the first min(k, found) entries from cumulants summed in list order, and its normal, both
// written at the query's input index
struct NormalsFinish {
    double* __restrict__ normals;
    double* __restrict__ cov_out;

    __device__ inline void operator()(const GridView& g, const KnnList& L, int k, uint32_t out) const {
        const uint32_t m = L.found < (uint32_t)k ? L.found : (uint32_t)k;
        double C[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        if (m >= 3) {
            double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < LNR_KNN_MAX; ++j) {
                if ((uint32_t)j < m) {
                    const double* t = g.pts + 3 * (size_t)L.pos[j];
                    const double x = t[0], y = t[1], z = t[2];
                    s[0] = s[0] + x; s[1] = s[1] + y; s[2] = s[2] + z;
                    s[3] = s[3] + x * x; s[4] = s[4] + x * y; s[5] = s[5] + x * z;
                    s[6] = s[6] + y * y; s[7] = s[7] + y * z; s[8] = s[8] + z * z;
                }
            }
            const double c = (double)m;
            for (int v = 0; v < 9; ++v) s[v] = s[v] / c;
            C[0][0] = s[3] - s[0] * s[0]; C[1][1] = s[6] - s[1] * s[1]; C[2][2] = s[8] - s[2] * s[2];
            C[0][1] = C[1][0] = s[4] - s[0] * s[1];
            C[0][2] = C[2][0] = s[5] - s[0] * s[2];
            C[1][2] = C[2][1] = s[7] - s[1] * s[2];
        }
        double nv[3];
        normal_of(C, nv);
        for (int a = 0; a < 3; ++a) normals[3 * (size_t)out + a] = nv[a];
        if (cov_out)
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) cov_out[9 * (size_t)out + 3 * a + b] = C[a][b];
    }
};

// ------------------------------------------------------------------------------------------------ point-to-plane ICP
// Terms of one correspondence's contribution, in this order: JTJ upper triangle row by row (21), JTr (6), d2, count.
#define ICP_TERMS 29
#define ICP_PART_STRIDE 32
#define ICP_MAX_BLOCKS 2048
enum { ICP_ST_NONFINITE_SOURCE = 1, ICP_ST_NONFINITE_TARGET = 2, ICP_ST_NONFINITE_NORMAL = 4, ICP_ST_NONFINITE_UPDATE = 8,
       ICP_ST_BAD_COVARIANCE = 16 };

struct IcpState {
    double T[16];                   // the accumulated transformation (row-major)
    double U[16];                   // this round's update
    double sums[ICP_TERMS];         // the last fold
    double sys[ICP_TERMS];          // the last system solved
    double x[6];                    // its step
    double fitness, rmse;
    unsigned long long n_corr, nonfinite_source, bad_normals;
    uint32_t active;                // this round runs (set by icp_solve)
    uint32_t done;
    uint32_t rounds;
    uint32_t status;
    unsigned long long bad_covariances;     // generalized ICP: correspondences whose combined covariance could not be inverted
};

// the nearest target with d2 < r2 under the (d2, index) order; the walk ends once every unvisited cell lies at r or beyond
__device__ inline bool nearest_within(const GridView& g, double qx, double qy, double qz, double r2, int64_t max_shell, double& best,
                                      uint32_t& best_id, uint32_t& best_pos) {
    best = INFINITY;
    best_id = 0xffffffffu;
    best_pos = 0;
    const ShellQuery s = shell_query(g.p, qx, qy, qz);
    auto visit = [&](uint32_t j) {
        const double d2 = sq_dist(s.q[0], s.q[1], s.q[2], g.pts + 3 * (size_t)j);
        const uint32_t id = g.orig[j];
        if (d2 < r2 && pair_less(d2, id, best, best_id)) { best = d2; best_id = id; best_pos = j; }
    };
    for (int64_t r = 0; r <= max_shell; ++r) {
        const double lb = shell_visit(g, s, r, visit);
        if (lb == INFINITY || best < lb || r2 <= lb) break;
    }
    return best_id != 0xffffffffu;
}

// SYSTEM: each thread sums the terms of its sources (i = thread, thread + stride, ...) in order, then each block writes its fixed-order
// sum to part; otherwise the index and d2 of every source are written.  Non-finite sources count and take no correspondence.
// Shells beyond ceil(r / edge) + 1 hold no target within r (the one past ceil(r / edge) covers the rounding of the cell assignments).
template <bool SYSTEM>
__global__ __launch_bounds__(CL_BLOCK) void icp_corr(GridView g, const double* __restrict__ normals, const double* __restrict__ src,
                                                     uint32_t n_src, double r, IcpState* st, double* __restrict__ part,
                                                     int32_t* __restrict__ index, double* __restrict__ d2_out,
                                                     unsigned long long* __restrict__ counters) {
    if (SYSTEM && (!st->active || st->status)) return;
    __shared__ double lds[CL_BLOCK / 64];
    const CloudParams* p = g.p;
    const double r2 = r * r;
    const double dmax = (double)(p->dims[0] > p->dims[1] ? (p->dims[0] > p->dims[2] ? p->dims[0] : p->dims[2])
                                                         : (p->dims[1] > p->dims[2] ? p->dims[1] : p->dims[2]));
    const int64_t max_shell = (int64_t)fmin(ceil(r / p->edge) + 1.0, dmax);
    const bool any = p->n > 0;
    double acc[ICP_TERMS];
#pragma unroll
    for (int v = 0; v < ICP_TERMS; ++v) acc[v] = 0.0;
    unsigned long long bad = 0, bad_n = 0;
    for (uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x; i < n_src; i += gridDim.x * CL_BLOCK) {
        const double sx = src[3 * (size_t)i], sy = src[3 * (size_t)i + 1], sz = src[3 * (size_t)i + 2];
        double best;
        uint32_t id, pos;
        const bool ok = finite3(sx, sy, sz);
        const bool hit = ok && any && nearest_within(g, sx, sy, sz, r2, max_shell, best, id, pos);
        bad += ok ? 0ull : 1ull;
        if (!SYSTEM) {
            index[i] = hit ? (int32_t)id : -1;
            d2_out[i] = ok ? (hit ? best : INFINITY) : NAN;
            continue;
        }
        if (!hit) continue;
        const double* t = g.pts + 3 * (size_t)pos;
        const double nt[3] = {normals[3 * (size_t)id], normals[3 * (size_t)id + 1], normals[3 * (size_t)id + 2]};
        if (!finite3(nt[0], nt[1], nt[2])) { ++bad_n; continue; }
        const double s3[3] = {sx, sy, sz}, dv[3] = {sx - t[0], sy - t[1], sz - t[2]};
        const double res = dot3(dv, nt);
        double J[6];
        cross3(s3, nt, J);
        J[3] = nt[0]; J[4] = nt[1]; J[5] = nt[2];
        int v = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b, ++v) acc[v] = acc[v] + J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + J[a] * res;
        acc[27] = acc[27] + best;
        acc[28] = acc[28] + 1.0;
    }
    bad = wave_sum(bad);
    bad_n = wave_sum(bad_n);
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicAdd(SYSTEM ? &st->nonfinite_source : &counters[1], bad);
        if (SYSTEM && bad_n) atomicAdd(&st->bad_normals, bad_n);
    }
    if (!SYSTEM) return;
#pragma unroll
    for (int v = 0; v < ICP_TERMS; ++v) {
        const double t = block_sum(acc[v], lds);
        if (threadIdx.x == 0) part[(size_t)ICP_PART_STRIDE * blockIdx.x + v] = t;
    }
}

// ------------------------------------------------------------------------------------------------ robust weights, generalized ICP
// The weight of a residual of magnitude m >= 0 (include/loner_hip.h, "robust kernels"): 1 Huber, 2 Cauchy, 3 Tukey.  L2 (0) has no
// weight and never comes here.
template <int KERNEL>
__device__ inline double robust_weight(double m, double k) {
    if (KERNEL == 1) return k / fmax(m, k);
    const double q = m / k;
    if (KERNEL == 2) return 1.0 / (1.0 + q * q);
    const double u = 1.0 - q * q;
    return m <= k ? u * u : 0.0;
}

// icp_corr<true> with a weight per correspondence, and for GENERALIZED with the plane-to-plane system: the same walk, the same 29 terms
// in the same order, the same per-thread and per-block sums.  attr: the targets' normals [n,3], or for GENERALIZED their covariances
// [n,3,3]; src_cov: the sources' covariances as given (they are rotated by the accumulated transformation of st here, every round,
// and never stored).  Of every covariance the upper triangle is read.  KERNEL 0 adds the terms as they are.
template <bool GENERALIZED, int KERNEL>
__global__ __launch_bounds__(CL_BLOCK) void icp_corr_w(GridView g, const double* __restrict__ attr, const double* __restrict__ src,
                                                       const double* __restrict__ src_cov, uint32_t n_src, double r, double k,
                                                       IcpState* st, double* __restrict__ part) {
    static_assert(GENERALIZED || KERNEL != 0, "point to plane with L2 is icp_corr<true>");
    if (!st->active || st->status) return;
    __shared__ double lds[CL_BLOCK / 64];
    const CloudParams* p = g.p;
    const double r2 = r * r;
    const double dmax = (double)(p->dims[0] > p->dims[1] ? (p->dims[0] > p->dims[2] ? p->dims[0] : p->dims[2])
                                                         : (p->dims[1] > p->dims[2] ? p->dims[1] : p->dims[2]));
    const int64_t max_shell = (int64_t)fmin(ceil(r / p->edge) + 1.0, dmax);
    const bool any = p->n > 0;
    double R[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) R[a][b] = GENERALIZED ? st->T[4 * a + b] : 0.0;
    double acc[ICP_TERMS];
#pragma unroll
    for (int v = 0; v < ICP_TERMS; ++v) acc[v] = 0.0;
    unsigned long long bad = 0, bad_a = 0;
    for (uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x; i < n_src; i += gridDim.x * CL_BLOCK) {
        const double sx = src[3 * (size_t)i], sy = src[3 * (size_t)i + 1], sz = src[3 * (size_t)i + 2];
        double best;
        uint32_t id, pos;
        const bool ok = finite3(sx, sy, sz);
        const bool hit = ok && any && nearest_within(g, sx, sy, sz, r2, max_shell, best, id, pos);
        bad += ok ? 0ull : 1ull;
        if (!hit) continue;
        const double* t = g.pts + 3 * (size_t)pos;
        const double s3[3] = {sx, sy, sz}, dv[3] = {sx - t[0], sy - t[1], sz - t[2]};
        double term[27], w = 1.0;
        if constexpr (GENERALIZED) {
            const double* ct = attr + 9 * (size_t)id;
            const double* cs = src_cov + 9 * (size_t)i;
            const double S[3][3] = {{cs[0], cs[1], cs[2]}, {cs[1], cs[4], cs[5]}, {cs[2], cs[5], cs[8]}};
            double B[3][3];                                    // R C_s
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) B[a][b] = (R[a][0] * S[0][b] + R[a][1] * S[1][b]) + R[a][2] * S[2][b];
            const double m00 = ct[0] + dot3(B[0], R[0]), m01 = ct[1] + dot3(B[0], R[1]), m02 = ct[2] + dot3(B[0], R[2]);
            const double m11 = ct[4] + dot3(B[1], R[1]), m12 = ct[5] + dot3(B[1], R[2]), m22 = ct[8] + dot3(B[2], R[2]);
            const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
            const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
            const double det = (m00 * c00 + m01 * c01) + m02 * c02;
            if (!(finite3(m00, m01, m02) && finite3(m11, m12, m22) && det > 0.0)) { ++bad_a; continue; }
            const double W[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
            const double Wd[3] = {dot3(W[0], dv), dot3(W[1], dv), dot3(W[2], dv)};
            if constexpr (KERNEL != 0) w = robust_weight<KERNEL>(sqrt(fmax(dot3(dv, Wd), 0.0)), k);
            double G[3][3], H[3][3];                           // G = W A (row a: s x W_a), H = A^T G (column b: s x G_.b), A = -[s]x
#pragma unroll
            for (int a = 0; a < 3; ++a) cross3(s3, W[a], G[a]);
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const double col[3] = {G[0][b], G[1][b], G[2][b]};
                double h[3];
                cross3(s3, col, h);
                H[0][b] = h[0]; H[1][b] = h[1]; H[2][b] = h[2];
            }
            int v = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = a; b < 3; ++b) term[v++] = H[a][b];
#pragma unroll
                for (int c = 0; c < 3; ++c) term[v++] = G[c][a];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = a; b < 3; ++b) term[v++] = W[a][b];
            cross3(s3, Wd, term + 21);
            term[24] = Wd[0]; term[25] = Wd[1]; term[26] = Wd[2];
        } else {
            const double nt[3] = {attr[3 * (size_t)id], attr[3 * (size_t)id + 1], attr[3 * (size_t)id + 2]};
            if (!finite3(nt[0], nt[1], nt[2])) { ++bad_a; continue; }
            const double res = dot3(dv, nt);
            w = robust_weight<KERNEL>(fabs(res), k);
            double J[6];
            cross3(s3, nt, J);
            J[3] = nt[0]; J[4] = nt[1]; J[5] = nt[2];
            int v = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) term[v++] = J[a] * J[b];
#pragma unroll
            for (int a = 0; a < 6; ++a) term[21 + a] = J[a] * res;
        }
#pragma unroll
        for (int v = 0; v < 27; ++v) acc[v] = acc[v] + (KERNEL ? w * term[v] : term[v]);
        acc[27] = acc[27] + best;
        acc[28] = acc[28] + 1.0;
    }
    bad = wave_sum(bad);
    bad_a = wave_sum(bad_a);
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicAdd(&st->nonfinite_source, bad);
        if (bad_a) atomicAdd(GENERALIZED ? &st->bad_covariances : &st->bad_normals, bad_a);
    }
#pragma unroll
    for (int v = 0; v < ICP_TERMS; ++v) {
        const double t = block_sum(acc[v], lds);
        if (threadIdx.x == 0) part[(size_t)ICP_PART_STRIDE * blockIdx.x + v] = t;
    }
}

// C_ab = delta_ab - ((1 - epsilon) n_a) n_b for a <= b, mirrored below the diagonal
__global__ __launch_bounds__(CL_BLOCK) void plane_covariances(const double* __restrict__ normals, uint32_t n, double epsilon,
                                                               double* __restrict__ cov) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double nv[3] = {normals[3 * (size_t)i], normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2]};
    const double f = 1.0 - epsilon;
    double* C = cov + 9 * (size_t)i;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            const double c = (a == b ? 1.0 : 0.0) - (f * nv[a]) * nv[b];
            C[3 * a + b] = c;
            C[3 * b + a] = c;
        }
}

// one workgroup: the partials summed in a fixed order (thread t: blocks t, t + 256, ... in turn, then the block sum), fitness and RMSE,
// and from round 1 on the convergence test against the previous pass
__global__ __launch_bounds__(CL_BLOCK) void icp_fold(const double* __restrict__ part, uint32_t n_part, IcpState* st, uint32_t n_src,
                                                     double rel_fitness, double rel_rmse, int round) {
    if (round > 0 && !st->active) return;
    __shared__ double lds[CL_BLOCK / 64];
    const bool skip = st->status != 0;
    double tot[ICP_TERMS];
#pragma unroll
    for (int v = 0; v < ICP_TERMS; ++v) {
        double a = 0.0;
        if (!skip)
            for (uint32_t b = threadIdx.x; b < n_part; b += CL_BLOCK) a = a + part[(size_t)ICP_PART_STRIDE * b + v];
        tot[v] = block_sum(a, lds);
    }
    if (threadIdx.x != 0) return;
    uint32_t status = st->status;
    if (st->nonfinite_source) status |= ICP_ST_NONFINITE_SOURCE;
    if (st->bad_normals) status |= ICP_ST_NONFINITE_NORMAL;
    if (st->bad_covariances) status |= ICP_ST_BAD_COVARIANCE;
    st->status = status;
    if (status) {
        st->done = 1;
        return;
    }
    for (int v = 0; v < ICP_TERMS; ++v) st->sums[v] = tot[v];
    const double cnt = tot[28];
    const double fitness = cnt > 0.0 ? cnt / (double)n_src : 0.0;
    const double rmse = cnt > 0.0 ? sqrt(tot[27] / cnt) : 0.0;
    if (round > 0) {
        st->rounds = round;
        if (fabs(st->fitness - fitness) < rel_fitness && fabs(st->rmse - rmse) < rel_rmse) st->done = 1;
    }
    st->fitness = fitness;
    st->rmse = rmse;
    st->n_corr = (unsigned long long)cnt;
}

// one thread: the step from the last fold's system, update @ transformation, and whether the round runs
__global__ void icp_solve(IcpState* st) {
    st->active = 0;
    if (st->done || st->status) return;
    const double* s = st->sums;
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (s[28] > 0.0) {
        double A[6][6], b[6];
        int v = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c, ++v) A[a][c] = A[c][a] = s[v];
#pragma unroll
        for (int a = 0; a < 6; ++a) b[a] = -s[21 + a];
        ldlt_solve6(A, b, x);
    }
    double U[16], T[16];
    step_matrix(x, U);
    if (s[28] == 0.0)
        for (int e = 0; e < 16; ++e) U[e] = (e % 5) == 0 ? 1.0 : 0.0;
    bool finite = true;
    for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 4; ++c) {
            T[4 * a + c] = ((U[4 * a] * st->T[c] + U[4 * a + 1] * st->T[4 + c]) + U[4 * a + 2] * st->T[8 + c]) + U[4 * a + 3] * st->T[12 + c];
            finite = finite && isfinite(T[4 * a + c]) && isfinite(U[4 * a + c]);
        }
    for (int a = 0; a < 6; ++a) finite = finite && isfinite(x[a]);
    for (int v = 0; v < ICP_TERMS; ++v) st->sys[v] = s[v];
    for (int a = 0; a < 6; ++a) st->x[a] = x[a];
    if (!finite) {
        st->status |= ICP_ST_NONFINITE_UPDATE;
        st->done = 1;
        return;
    }
    for (int e = 0; e < 16; ++e) { st->U[e] = U[e]; st->T[e] = T[e]; }
    st->active = 1;
}

// lnr_cloud_append_transformed by a matrix in device memory: T [12] is a round's update, read where icp_solve wrote it; skipped when
// *active is 0
__global__ __launch_bounds__(CL_BLOCK) void append_transformed_dev(const double* src, uint32_t n, const double* __restrict__ T,
                                                                   const uint32_t* active, double* dst) {
    if (active && !*active) return;
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i < n) transform_point(src, T, dst, i);
}

__global__ void icp_begin(IcpState* st, Affine init, const CloudParams* p, uint32_t n_targets) {
    for (int e = 0; e < 12; ++e) st->T[e] = init.t[e];
    st->T[12] = 0.0; st->T[13] = 0.0; st->T[14] = 0.0; st->T[15] = 1.0;
    for (int e = 0; e < 16; ++e) st->U[e] = (e % 5) == 0 ? 1.0 : 0.0;
    for (int v = 0; v < ICP_TERMS; ++v) { st->sums[v] = 0.0; st->sys[v] = 0.0; }
    for (int a = 0; a < 6; ++a) st->x[a] = 0.0;
    st->fitness = 0.0;
    st->rmse = 0.0;
    st->n_corr = 0;
    st->nonfinite_source = 0;
    st->bad_normals = 0;
    st->bad_covariances = 0;
    st->done = 0;
    st->rounds = 0;
    st->status = (p->status & CL_ST_NONFINITE) || p->n != n_targets ? (uint32_t)ICP_ST_NONFINITE_TARGET : 0u;
    st->active = 1;
}

__global__ void icp_end(const IcpState* st, double* result, int64_t* info) {
    for (int e = 0; e < 16; ++e) result[e] = st->T[e];
    result[16] = st->fitness;
    result[17] = st->rmse;
    for (int v = 0; v < ICP_TERMS - 1; ++v) result[18 + v] = st->sys[v];
    for (int a = 0; a < 6; ++a) result[46 + a] = st->x[a];
    for (int e = 52; e < LNR_ICP_RESULT; ++e) result[e] = 0.0;
    info[0] = st->status;
    info[1] = (int64_t)st->n_corr;
    info[2] = st->rounds;
    info[3] = (int64_t)st->nonfinite_source;
    info[4] = (int64_t)st->bad_normals;
    info[5] = (int64_t)st->sys[28];
    info[6] = st->done;
    info[7] = (int64_t)st->bad_covariances;
}

// ------------------------------------------------------------------------------------------------ information matrix
// GetInformationMatrixFromPointClouds: the source moved by T (transform_point's rounding), icp_corr's search, and per correspondence
// with the target q the 21 upper-triangle terms of G^T G, G = [-[q]x | I], each ((G0a G0b + G1a G1b) + G2a G2b); term 21 counts the
// correspondences, term 22 the non-finite source points.  Per thread in source order, then per block, as icp_corr's sums.
#define INFO_TERMS 23
__global__ __launch_bounds__(CL_BLOCK) void icp_info_corr(GridView g, const double* __restrict__ src, uint32_t n_src, Affine T, double r,
                                                          double* __restrict__ part) {
    __shared__ double lds[CL_BLOCK / 64];
    const CloudParams* p = g.p;
    const double r2 = r * r;
    const double dmax = (double)(p->dims[0] > p->dims[1] ? (p->dims[0] > p->dims[2] ? p->dims[0] : p->dims[2])
                                                         : (p->dims[1] > p->dims[2] ? p->dims[1] : p->dims[2]));
    const int64_t max_shell = (int64_t)fmin(ceil(r / p->edge) + 1.0, dmax);
    const bool any = p->n > 0;
    double acc[INFO_TERMS];
#pragma unroll
    for (int v = 0; v < INFO_TERMS; ++v) acc[v] = 0.0;
    for (uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x; i < n_src; i += gridDim.x * CL_BLOCK) {
        double s3[3];
        transform_point(src + 3 * (size_t)i, T.t, s3, 0);
        double best;
        uint32_t id, pos;
        const bool ok = finite3(s3[0], s3[1], s3[2]);
        if (!ok) acc[22] = acc[22] + 1.0;
        if (!(ok && any && nearest_within(g, s3[0], s3[1], s3[2], r2, max_shell, best, id, pos))) continue;
        const double* q = g.pts + 3 * (size_t)pos;
        const double G[3][6] = {{0.0, q[2], -q[1], 1.0, 0.0, 0.0}, {-q[2], 0.0, q[0], 0.0, 1.0, 0.0}, {q[1], -q[0], 0.0, 0.0, 0.0, 1.0}};
        int v = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b, ++v) acc[v] = acc[v] + ((G[0][a] * G[0][b] + G[1][a] * G[1][b]) + G[2][a] * G[2][b]);
        acc[21] = acc[21] + 1.0;
    }
#pragma unroll
    for (int v = 0; v < INFO_TERMS; ++v) {
        const double t = block_sum(acc[v], lds);
        if (threadIdx.x == 0) part[(size_t)ICP_PART_STRIDE * blockIdx.x + v] = t;
    }
}

// one workgroup: icp_fold's order over the partials, the symmetric 6x6 and the info words
__global__ __launch_bounds__(CL_BLOCK) void icp_info_fold(const double* __restrict__ part, uint32_t n_part, const CloudParams* p,
                                                          uint32_t n_targets, double* __restrict__ result, int64_t* __restrict__ info) {
    __shared__ double lds[CL_BLOCK / 64];
    __shared__ double tot[INFO_TERMS];
    for (int v = 0; v < INFO_TERMS; ++v) {
        double a = 0.0;
        for (uint32_t b = threadIdx.x; b < n_part; b += CL_BLOCK) a = a + part[(size_t)ICP_PART_STRIDE * b + v];
        const double t = block_sum(a, lds);
        if (threadIdx.x == 0) tot[v] = t;
    }
    if (threadIdx.x != 0) return;
    int v = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++v) result[6 * a + b] = result[6 * b + a] = tot[v];
    const bool bad_grid = (p->status & CL_ST_NONFINITE) || p->n != n_targets;
    info[0] = (tot[22] > 0.0 ? (int64_t)ICP_ST_NONFINITE_SOURCE : 0) | (bad_grid ? (int64_t)ICP_ST_NONFINITE_TARGET : 0);
    info[1] = (int64_t)tot[21];
    info[2] = (int64_t)tot[22];
    info[3] = 0;
}

// ------------------------------------------------------------------------------------------------ host
uint32_t icp_blocks(int64_t n_source) {
    const uint32_t b = blocks_for(n_source);
    return b < 1 ? 1u : (b < ICP_MAX_BLOCKS ? b : (uint32_t)ICP_MAX_BLOCKS);
}
struct IcpLayout { size_t state, part, src, total; };
IcpLayout icp_layout(int64_t n_source) {
    IcpLayout l;
    l.state = 0;
    l.part = align256(sizeof(IcpState));
    l.src = align256(l.part + sizeof(double) * ICP_PART_STRIDE * (size_t)icp_blocks(n_source));
    l.total = align256(l.src + 24 * (size_t)n_source);
    return l;
}

}  // namespace

extern "C" int lnr_cloud_normals(const void* grid, int64_t n_points, int32_t knn, double* normals, double* covariances, void* workspace,
                                 size_t workspace_bytes, int64_t* counters_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_normals", n_points, "points");
    LNR_REQUIRE(knn >= 1 && knn <= LNR_KNN_MAX, "lnr_cloud_normals: knn must be in [1, %d], got %d", LNR_KNN_MAX, (int)knn);
    LNR_REQUIRE(grid && counters_dev && workspace && (n_points == 0 || normals), "lnr_cloud_normals: null argument");
    const size_t need = lnr_cloud_workspace(n_points);
    LNR_REQUIRE(workspace_bytes >= need, "lnr_cloud_normals: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = clear_words(counters_dev, 4 * sizeof(int64_t), st, "lnr_cloud_normals", "counters")) return rc;
    if (n_points == 0) return LNR_OK;
    LnrProfScope prof("cloud_normals", st);
    const GridView g = grid_view(grid, n_points);
    uint32_t* fb = (uint32_t*)workspace;
    unsigned long long* cnt = (unsigned long long*)counters_dev;
    const uint32_t n = (uint32_t)n_points;
    enqueue_knn(g, n, (int)knn, NormalsFinish{normals, covariances}, fb, cnt, st);
    LNR_CHECK_LAUNCH("lnr_cloud_normals");
    return LNR_OK;
}

extern "C" int lnr_icp_correspondences(const void* grid, int64_t n_targets, const double* queries, int64_t n_queries, double max_distance,
                                       int32_t* index, double* sq_distance, int64_t* counters_dev, void* stream) {
    CL_REQUIRE_COUNTS("lnr_icp_correspondences", n_targets, "targets", n_queries, "queries");
    LNR_REQUIRE(isfinite(max_distance) && max_distance > 0.0, "lnr_icp_correspondences: max_distance must be finite and > 0, got %g",
                max_distance);
    LNR_REQUIRE(grid && counters_dev && (n_queries == 0 || (queries && index && sq_distance)), "lnr_icp_correspondences: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = clear_words(counters_dev, 4 * sizeof(int64_t), st, "lnr_icp_correspondences", "counters")) return rc;
    if (n_queries == 0) return LNR_OK;
    LnrProfScope prof("icp_correspondences", st);
    const GridView g = grid_view(grid, n_targets);
    hipLaunchKernelGGL(icp_corr<false>, dim3(icp_blocks(n_queries)), dim3(CL_BLOCK), 0, st, g, (const double*)nullptr, queries,
                       (uint32_t)n_queries, max_distance, (IcpState*)nullptr, (double*)nullptr, index, sq_distance,
                       (unsigned long long*)counters_dev);
    LNR_CHECK_LAUNCH("lnr_icp_correspondences");
    return LNR_OK;
}

extern "C" size_t lnr_icp_workspace(int64_t n_source) {
    if (!count_ok(n_source)) return 0;
    return icp_layout(n_source).total;
}

namespace {

// What the three ICP entry points share: the argument checks, the workspace, and every round enqueued at once.  attr: the targets'
// normals or covariances.  corr(g, pcd, ns, nb, state, part, stream) launches the entry point's correspondence kernel for one round.
struct IcpArgs {
    const void* grid; int64_t n_targets; const double* attr; const double* source; int64_t n_source; double max_distance;
    const double* init; double relative_fitness, relative_rmse; int32_t max_iteration; void* workspace; size_t workspace_bytes;
    double* result_dev; int64_t* info_dev; void* stream;
};

template <class Corr>
int icp_run(const char* fn, const IcpArgs& a, Corr corr) {
    LNR_REQUIRE(count_ok(a.n_targets) && count_ok(a.n_source), "%s: %lld targets, %lld source points, the limit is %lld each", fn,
                (long long)a.n_targets, (long long)a.n_source, (long long)CL_MAX_POINTS);
    LNR_REQUIRE(isfinite(a.max_distance) && a.max_distance > 0.0, "%s: max_distance must be finite and > 0, got %g", fn, a.max_distance);
    LNR_REQUIRE(a.max_iteration >= 0, "%s: max_iteration must be >= 0, got %d", fn, (int)a.max_iteration);
    LNR_REQUIRE(!(a.relative_fitness != a.relative_fitness) && !(a.relative_rmse != a.relative_rmse), "%s: NaN criteria", fn);
    LNR_REQUIRE(a.grid && a.init && a.workspace && a.result_dev && a.info_dev && (a.n_targets == 0 || a.attr) &&
                (a.n_source == 0 || a.source), "%s: null argument", fn);
    const IcpLayout l = icp_layout(a.n_source);
    LNR_REQUIRE(a.workspace_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed", fn, a.workspace_bytes, l.total);
    Affine T0;
    const int bad = affine_from_host(a.init, &T0);
    LNR_REQUIRE(bad < 0, "%s: non-finite init entry %d", fn, bad);
    LNR_REQUIRE(a.init[12] == 0.0 && a.init[13] == 0.0 && a.init[14] == 0.0 && a.init[15] == 1.0,
                "%s: init's bottom row must be [0, 0, 0, 1]", fn);
    hipStream_t st = (hipStream_t)a.stream;
    LnrProfScope prof(fn + 4, st);                           // the span is the entry point's name without "lnr_"
    char* ws = (char*)a.workspace;
    IcpState* s = (IcpState*)(ws + l.state);
    double* part = (double*)(ws + l.part);
    double* pcd = (double*)(ws + l.src);
    const GridView g = grid_view(a.grid, a.n_targets);
    const uint32_t ns = (uint32_t)a.n_source, nb = icp_blocks(a.n_source);
    hipLaunchKernelGGL(icp_begin, dim3(1), dim3(1), 0, st, s, T0, g.p, (uint32_t)a.n_targets);
    if (int rc = lnr_cloud_append_transformed(a.source, a.n_source, a.init, pcd, a.stream)) return rc;
    corr(g, (const double*)pcd, ns, nb, s, part, st);
    hipLaunchKernelGGL(icp_fold, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)part, nb, s, ns, a.relative_fitness, a.relative_rmse, 0);
    LNR_CHECK_LAUNCH(fn);
    for (int it = 1; it <= a.max_iteration; ++it) {
        hipLaunchKernelGGL(icp_solve, dim3(1), dim3(1), 0, st, s);
        if (ns)
            hipLaunchKernelGGL(append_transformed_dev, dim3(blocks_for(ns)), dim3(CL_BLOCK), 0, st, (const double*)pcd, ns,
                               (const double*)s->U, (const uint32_t*)&s->active, pcd);
        corr(g, (const double*)pcd, ns, nb, s, part, st);
        hipLaunchKernelGGL(icp_fold, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)part, nb, s, ns, a.relative_fitness, a.relative_rmse,
                           it);
        LNR_CHECK_LAUNCH(fn);
    }
    hipLaunchKernelGGL(icp_end, dim3(1), dim3(1), 0, st, (const IcpState*)s, a.result_dev, a.info_dev);
    LNR_CHECK_LAUNCH(fn);
    return LNR_OK;
}

// the plain point-to-plane round: icp_corr<true>, the kernel lnr_icp_point_to_plane has always run
void corr_plane_l2(const GridView& g, const double* normals, const double* pcd, uint32_t ns, uint32_t nb, double r, IcpState* s,
                   double* part, hipStream_t st) {
    hipLaunchKernelGGL(icp_corr<true>, dim3(nb), dim3(CL_BLOCK), 0, st, g, normals, pcd, ns, r, s, part, (int32_t*)nullptr,
                       (double*)nullptr, (unsigned long long*)nullptr);
}

template <bool GENERALIZED, int KERNEL>
void corr_weighted(const GridView& g, const double* attr, const double* pcd, const double* src_cov, uint32_t ns, uint32_t nb, double r,
                   double k, IcpState* s, double* part, hipStream_t st) {
    hipLaunchKernelGGL((icp_corr_w<GENERALIZED, KERNEL>), dim3(nb), dim3(CL_BLOCK), 0, st, g, attr, pcd, src_cov, ns, r, k, s, part);
}

int kernel_ok(const char* fn, int32_t kernel, double kernel_k) {
    LNR_REQUIRE(kernel >= LNR_ROBUST_L2 && kernel <= LNR_ROBUST_TUKEY, "%s: kernel must be 0 (L2), 1 (Huber), 2 (Cauchy) or 3 (Tukey), got %d",
                fn, (int)kernel);
    LNR_REQUIRE(kernel == LNR_ROBUST_L2 || (isfinite(kernel_k) && kernel_k > 0.0), "%s: kernel_k must be finite and > 0, got %g", fn,
                kernel_k);
    return LNR_OK;
}

}  // namespace

extern "C" int lnr_icp_point_to_plane(const void* grid, int64_t n_targets, const double* target_normals,
                                      const double* source, int64_t n_source, double max_distance, const double* init,
                                      double relative_fitness, double relative_rmse, int32_t max_iteration, void* workspace,
                                      size_t workspace_bytes, double* result_dev, int64_t* info_dev, void* stream) {
    const IcpArgs a = {grid, n_targets, target_normals, source, n_source, max_distance, init, relative_fitness, relative_rmse,
                       max_iteration, workspace, workspace_bytes, result_dev, info_dev, stream};
    return icp_run("lnr_icp_point_to_plane", a, [&](const GridView& g, const double* pcd, uint32_t ns, uint32_t nb, IcpState* s,
                                                    double* part, hipStream_t st) {
        corr_plane_l2(g, target_normals, pcd, ns, nb, max_distance, s, part, st);
    });
}

extern "C" int lnr_icp_point_to_plane_robust(const void* grid, int64_t n_targets, const double* target_normals, const double* source,
                                             int64_t n_source, double max_distance, const double* init, double relative_fitness,
                                             double relative_rmse, int32_t max_iteration, int32_t kernel, double kernel_k,
                                             void* workspace, size_t workspace_bytes, double* result_dev, int64_t* info_dev,
                                             void* stream) {
    if (int rc = kernel_ok("lnr_icp_point_to_plane_robust", kernel, kernel_k)) return rc;
    const IcpArgs a = {grid, n_targets, target_normals, source, n_source, max_distance, init, relative_fitness, relative_rmse,
                       max_iteration, workspace, workspace_bytes, result_dev, info_dev, stream};
    return icp_run("lnr_icp_point_to_plane_robust", a, [&](const GridView& g, const double* pcd, uint32_t ns, uint32_t nb, IcpState* s,
                                                           double* part, hipStream_t st) {
        const double* none = nullptr;
        switch (kernel) {
            case LNR_ROBUST_L2: corr_plane_l2(g, target_normals, pcd, ns, nb, max_distance, s, part, st); break;
            case LNR_ROBUST_HUBER: corr_weighted<false, 1>(g, target_normals, pcd, none, ns, nb, max_distance, kernel_k, s, part, st); break;
            case LNR_ROBUST_CAUCHY: corr_weighted<false, 2>(g, target_normals, pcd, none, ns, nb, max_distance, kernel_k, s, part, st); break;
            default: corr_weighted<false, 3>(g, target_normals, pcd, none, ns, nb, max_distance, kernel_k, s, part, st); break;
        }
    });
}

extern "C" int lnr_icp_generalized(const void* grid, int64_t n_targets, const double* target_covariances, const double* source,
                                   const double* source_covariances, int64_t n_source, double max_distance, const double* init,
                                   double relative_fitness, double relative_rmse, int32_t max_iteration, int32_t kernel,
                                   double kernel_k, void* workspace, size_t workspace_bytes, double* result_dev, int64_t* info_dev,
                                   void* stream) {
    if (int rc = kernel_ok("lnr_icp_generalized", kernel, kernel_k)) return rc;
    LNR_REQUIRE(n_source <= 0 || source_covariances, "lnr_icp_generalized: null argument");
    const IcpArgs a = {grid, n_targets, target_covariances, source, n_source, max_distance, init, relative_fitness, relative_rmse,
                       max_iteration, workspace, workspace_bytes, result_dev, info_dev, stream};
    const double* tc = target_covariances;
    const double* sc = source_covariances;
    return icp_run("lnr_icp_generalized", a, [&](const GridView& g, const double* pcd, uint32_t ns, uint32_t nb, IcpState* s,
                                                 double* part, hipStream_t st) {
        switch (kernel) {
            case LNR_ROBUST_L2: corr_weighted<true, 0>(g, tc, pcd, sc, ns, nb, max_distance, 1.0, s, part, st); break;
            case LNR_ROBUST_HUBER: corr_weighted<true, 1>(g, tc, pcd, sc, ns, nb, max_distance, kernel_k, s, part, st); break;
            case LNR_ROBUST_CAUCHY: corr_weighted<true, 2>(g, tc, pcd, sc, ns, nb, max_distance, kernel_k, s, part, st); break;
            default: corr_weighted<true, 3>(g, tc, pcd, sc, ns, nb, max_distance, kernel_k, s, part, st); break;
        }
    });
}

extern "C" int lnr_cloud_plane_covariances(const double* normals, int64_t n, double epsilon, double* covariances, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_plane_covariances", n, "normals");
    LNR_REQUIRE(isfinite(epsilon) && epsilon > 0.0, "lnr_cloud_plane_covariances: epsilon must be finite and > 0, got %g", epsilon);
    LNR_REQUIRE(n == 0 || (normals && covariances), "lnr_cloud_plane_covariances: null argument");
    if (n == 0) return LNR_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(plane_covariances, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, normals, (uint32_t)n, epsilon, covariances);
    LNR_CHECK_LAUNCH("lnr_cloud_plane_covariances");
    return LNR_OK;
}

extern "C" int lnr_icp_information(const void* grid, int64_t n_targets, const double* source, int64_t n_source, const double* transformation,
                                   double max_distance, void* workspace, size_t workspace_bytes, double* result_dev, int64_t* info_dev,
                                   void* stream) {
    CL_REQUIRE_COUNTS("lnr_icp_information", n_targets, "targets", n_source, "source points");
    LNR_REQUIRE(isfinite(max_distance) && max_distance > 0.0, "lnr_icp_information: max_distance must be finite and > 0, got %g", max_distance);
    LNR_REQUIRE(grid && transformation && workspace && result_dev && info_dev && (n_source == 0 || source), "lnr_icp_information: null argument");
    const IcpLayout l = icp_layout(n_source);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_icp_information: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    Affine T;
    const int bad = affine_from_host(transformation, &T);
    LNR_REQUIRE(bad < 0, "lnr_icp_information: non-finite transformation entry %d", bad);
    LNR_REQUIRE(transformation[12] == 0.0 && transformation[13] == 0.0 && transformation[14] == 0.0 && transformation[15] == 1.0,
                "lnr_icp_information: transformation's bottom row must be [0, 0, 0, 1]");
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("icp_information", st);
    double* part = (double*)((char*)workspace + l.part);
    const GridView g = grid_view(grid, n_targets);
    const uint32_t nb = icp_blocks(n_source);
    hipLaunchKernelGGL(icp_info_corr, dim3(nb), dim3(CL_BLOCK), 0, st, g, source, (uint32_t)n_source, T, max_distance, part);
    hipLaunchKernelGGL(icp_info_fold, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)part, nb, g.p, (uint32_t)n_targets, result_dev, info_dev);
    LNR_CHECK_LAUNCH("lnr_icp_information");
    return LNR_OK;
}
