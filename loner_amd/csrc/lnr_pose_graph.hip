// Pose-graph optimisation for multiway registration (gfx950): open3d's PoseGraph / GlobalOptimizationLevenbergMarquardt with the line
// process of Choi et al., "Robust Reconstruction of Indoor Scenes", CVPR 2015.  The contract is include/loner_hip.h, "pose graph"; the
// numpy restatement is tests/pose_graph_restatement.py.  Compiled with -ffp-contract=off (build.py EXACT).  Everything is fp64.
//
// Model.  Node i has the pose T_i (node frame to world).  Edge k = (s, t, X, L, uncertain): X takes source-frame points to the target
// frame, so ideally T_t^-1 T_s = X.  With A = X^-1 T_t^-1 and B = T_s (rigid inverses, [R^T | -R^T t]) the error matrix is E = A B and
//   e = [(E21 - E12) / 2, (E02 - E20) / 2, (E10 - E01) / 2, E03, E13, E23]        (0-based entries)
// A step moves a pose by T_i <- M(d_i) T_i with M the ICP's rule (lnr_solve6.h: Rz(d2) Ry(d1) Rx(d0), t = d[3:6]).  At d = 0,
// dM/d d_c = G_c, the generator with [e_c]x in the rotation block for c < 3 and e_(c-3) in the translation column otherwise.  Hence
//   E(d_s, d_t) = A M(d_t)^-1 M(d_s) B,     dE/d d_s,c = A G_c B,     dE/d d_t,c = -A G_c B        at 0,
// so J_t = -J_s exactly, and with J = J_s, N_c = A_R [e_c]x B_R (row r, column j: A_R[r] . (e_c x b_j), b_j column j of B_R):
//   J[0..2][c] = ((N_c)21 - (N_c)12, (N_c)02 - (N_c)20, (N_c)10 - (N_c)01) / 2,   J[3 + r][c] = A_R[r] . (e_c x B_t)        c < 3
//   J[0..2][c] = 0,                                                                J[3 + r][c] = A_R[r][c - 3]              c >= 3
// One block per edge is therefore enough: W = J^T L J and g = J^T L e give J_s^T L J_s = J_t^T L J_t = W, J_s^T L J_t = -W (and
// J_t^T L J_s = -W^T), b_s -= w g, b_t += w g.  L is read as given and is expected symmetric.
//
// Lane mapping of the 6x6 work.  One lane owns one edge (linearisation) or one node (gather, SpMV, block solve) and keeps its 6x6
// blocks in registers, as icp_solve keeps the ICP's system: the pivoted LDLT needs every entry of a block in one lane (its pivot search
// and swaps are compares against static indices), a gather in one lane adds a node's incident blocks in one fixed order without any
// hand-over, and a pose graph is small (tens of thousands of nodes fill a few hundred waves), so the launches are latency-bound and
// a 36-lanes-per-block mapping would buy cross-lane traffic for no occupancy.  Sums across lanes are block_sum's fixed order, folded by
// one workgroup in a launch of its own.  No float atomics, nothing handed between workgroups inside a launch, ordinary launches only:
// two runs give the same bytes.
//   build      keys (node << shift | slot), slot = 2 k + role (0: the node is edge k's source, 1: its target), the shared radix sort,
//              then row_start by a lower bound per node: every gather walks a node's slots in (edge index, role) order
//   linearize  pg_edge: e, q = e^T L e, W, g per edge; pg_node: H_ii = sum w W and b_i over the node's slots, identity and zero for
//              the reference node
//   solve      block-Jacobi PCG on (H + lambda I) d = b, five launches per iteration (A p, alpha, update, beta and stop, p); every
//              iteration is enqueued, the state's done word makes later ones return at once
//   optimize   Levenberg-Marquardt trials, each: solve, trial poses, their residual, the decision (one workgroup), and where the
//              step was accepted the new poses, line-process weights and linear system.  The host reads one word per trial
#include "lnr_radix_sort.h"
#include "lnr_solve6.h"

#define PG_MAX_NODES ((int64_t)LNR_PG_MAX_NODES)
#define PG_MAX_EDGES ((int64_t)LNR_PG_MAX_EDGES)

namespace {

enum { PG_ST_BAD_ID = 1, PG_ST_SELF_EDGE = 2, PG_ST_NONFINITE_POSE = 4, PG_ST_NONFINITE_EDGE = 8, PG_ST_CG_BREAKDOWN = 16 };
enum { PG_STOP_NONE = 0, PG_STOP_MAX_ITERATION = 1, PG_STOP_RELATIVE_INCREMENT = 2, PG_STOP_RIGHT_TERM = 3, PG_STOP_RESIDUAL = 4,
       PG_STOP_MAX_ITERATION_LM = 5, PG_STOP_STATUS = 6 };

struct PgHead {                     // the head of a graph buffer; row_start [n + 1] and slot [2 m] follow
    uint32_t n, m, status, n_sort;
    int32_t npasses;
    uint32_t shift;
    unsigned long long bad_ids, self_edges;
};
struct PgGraph { const PgHead* head; const uint32_t* row_start; const uint32_t* slot; };
struct PgGraphLayout { size_t head, row_start, slot, total; };
PgGraphLayout graph_layout(int64_t n, int64_t m) {
    PgGraphLayout l;
    l.head = 0;
    l.row_start = align256(sizeof(PgHead));
    l.slot = align256(l.row_start + 4 * ((size_t)n + 1));
    l.total = align256(l.slot + 8 * (size_t)m + 4);
    return l;
}
PgGraph graph_view(const void* graph, int64_t n, int64_t m) {
    const PgGraphLayout l = graph_layout(n, m);
    const char* b = (const char*)graph;
    return PgGraph{(const PgHead*)(b + l.head), (const uint32_t*)(b + l.row_start), (const uint32_t*)(b + l.slot)};
}

struct PgEdges {
    const int32_t* src; const int32_t* tgt;
    const double* meas;             // [m,16]
    const double* info;             // [m,36]
    const int32_t* uncertain;       // [m]
    const double* line;             // [m] line-process values (read for uncertain edges)
    uint32_t m;
};
__device__ inline double edge_weight(const PgEdges& E, uint32_t k) { return E.uncertain[k] ? E.line[k] : 1.0; }

struct PgCg { double rz, bb, alpha, beta, rr, lambda; uint32_t done, converged, iters, pad; };
struct PgLm {
    double lambda, nu, F, F_new, rho, b_inf, mu, max_diag;
    uint32_t stop, reason, accepted_now, accepts, rejects, consecutive, trials, status;
    uint32_t capped, pad;           // capped: trials whose solve ended on max_cg, not on rtol
    unsigned long long cg_total;
};

uint32_t pg_blocks(int64_t n) { const uint32_t b = blocks_for((uint64_t)n); return b < 1 ? 1u : b; }

__device__ inline double block_max(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = lds[0];
#pragma unroll
    for (int w = 1; w < CL_BLOCK / 64; ++w) t = fmax(t, lds[w]);
    return t;
}

// the fold of one column of per-block partials by one workgroup (icp_fold's order); valid in thread 0
__device__ inline double fold_sum(const double* part, uint32_t n_part, int stride, int col, double* lds) {
    double a = 0.0;
    for (uint32_t b = threadIdx.x; b < n_part; b += CL_BLOCK) a = a + part[(size_t)stride * b + col];
    return block_sum(a, lds);
}
__device__ inline double fold_max(const double* part, uint32_t n_part, int stride, int col, double* lds) {
    double a = 0.0;
    for (uint32_t b = threadIdx.x; b < n_part; b += CL_BLOCK) a = fmax(a, part[(size_t)stride * b + col]);
    return block_max(a, lds);
}

// ------------------------------------------------------------------------------------------------ build
__global__ void pg_begin(PgHead* h, uint32_t n, uint32_t m, int32_t npasses, uint32_t shift) {
    h->n = n; h->m = m; h->status = 0; h->n_sort = 2 * m; h->npasses = npasses; h->shift = shift;
    h->bad_ids = 0; h->self_edges = 0;
}

// a bad edge (an id out of range, a self edge) sets the status and sorts behind every node, so nothing ever indexes by it
__global__ __launch_bounds__(CL_BLOCK) void pg_keys(PgHead* h, const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= 2 * h->m) return;
    const uint32_t k = i >> 1, role = i & 1u;
    const int64_t s = src[k], t = tgt[k], n = h->n;
    const bool bad_id = s < 0 || s >= n || t < 0 || t >= n, self = !bad_id && s == t;
    if (role == 0 && bad_id) { atomicOr(&h->status, (uint32_t)PG_ST_BAD_ID); atomicAdd(&h->bad_ids, 1ull); }
    if (role == 0 && self) { atomicOr(&h->status, (uint32_t)PG_ST_SELF_EDGE); atomicAdd(&h->self_edges, 1ull); }
    const uint64_t node = bad_id || self ? (uint64_t)n : (uint64_t)(role ? t : s);
    keys[i] = node << h->shift | (uint64_t)i;
    idx[i] = i;
}

__global__ __launch_bounds__(CL_BLOCK) void pg_rows(const PgHead* h, SortedPairs sp, uint32_t* __restrict__ row_start,
                                                    uint32_t* __restrict__ slot) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    const uint32_t L = h->n_sort;
    const uint64_t* keys = sp.keys(h->npasses);
    if (i <= h->n) {                                         // the first sorted entry of node i or beyond
        const uint64_t want = (uint64_t)i << h->shift;
        uint32_t lo = 0, hi = L;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < want) lo = mid + 1; else hi = mid;
        }
        row_start[i] = lo;
    }
    if (i < L) slot[i] = sp.idx(h->npasses)[i];
}

__global__ void pg_build_end(const PgHead* h, int64_t* info) {
    info[0] = h->status; info[1] = (int64_t)h->bad_ids; info[2] = (int64_t)h->self_edges; info[3] = 0;
}

// ------------------------------------------------------------------------------------------------ linearisation
// O = T^-1 of a rigid T (rows of 4; the bottom row is never read)
__device__ inline void rigid_inverse(const double* T, double O[12]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) O[4 * a + b] = T[4 * b + a];
        O[4 * a + 3] = -((T[a] * T[3] + T[4 + a] * T[7]) + T[8 + a] * T[11]);
    }
}
// C = A B for two affine maps (top three rows)
__device__ inline void affine_mul(const double A[12], const double* B, double C[12]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) C[4 * a + b] = (A[4 * a] * B[b] + A[4 * a + 1] * B[4 + b]) + A[4 * a + 2] * B[8 + b];
        C[4 * a + 3] = ((A[4 * a] * B[3] + A[4 * a + 1] * B[7]) + A[4 * a + 2] * B[11]) + A[4 * a + 3];
    }
}
// e_c x v
__device__ inline void unit_cross(int c, const double v[3], double o[3]) {
    if (c == 0) { o[0] = 0.0; o[1] = -v[2]; o[2] = v[1]; }
    else if (c == 1) { o[0] = v[2]; o[1] = 0.0; o[2] = -v[0]; }
    else { o[0] = -v[1]; o[1] = v[0]; o[2] = 0.0; }
}

// One edge per lane.  FULL: e, W and g are written as well as q.  part [gridDim.x]: the block's sum of w q + mu (sqrt(l) - 1)^2.
// guard / want: the launch returns unless *guard == want (nullable: always runs).
template <bool FULL>
__global__ __launch_bounds__(CL_BLOCK) void pg_edge(PgEdges E, uint32_t n_nodes, const double* __restrict__ poses, const double* mu_dev,
                                                    double* __restrict__ e_out, double* __restrict__ q_out, double* __restrict__ W_out,
                                                    double* __restrict__ g_out, double* __restrict__ part, uint32_t* status,
                                                    const uint32_t* stop, const uint32_t* guard, uint32_t want) {
    if ((stop && *stop) || (guard && *guard != want)) return;
    __shared__ double lds[CL_BLOCK / 64];
    const uint32_t k = blockIdx.x * CL_BLOCK + threadIdx.x;
    double f = 0.0;
    if (k < E.m) {
        const uint32_t s = (uint32_t)E.src[k], t = (uint32_t)E.tgt[k];
        if (s < n_nodes && t < n_nodes) {
            const double* Ts = poses + 16 * (size_t)s;
            const double* Tt = poses + 16 * (size_t)t;
            const double* X = E.meas + 16 * (size_t)k;
            const double* L = E.info + 36 * (size_t)k;
            bool fin_pose = true, fin_edge = true;
            for (int v = 0; v < 12; ++v) {
                fin_pose = fin_pose && isfinite(Ts[v]) && isfinite(Tt[v]);
                fin_edge = fin_edge && isfinite(X[v]);
            }
            double Xi[12], Ti[12], A[12], Em[12];
            rigid_inverse(X, Xi);
            rigid_inverse(Tt, Ti);
            affine_mul(Xi, Ti, A);
            affine_mul(A, Ts, Em);
            const double e[6] = {(Em[9] - Em[6]) / 2.0, (Em[2] - Em[8]) / 2.0, (Em[4] - Em[1]) / 2.0, Em[3], Em[7], Em[11]};
            double Le[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double sum = 0.0;
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    fin_edge = fin_edge && isfinite(L[6 * a + b]);
                    sum = sum + L[6 * a + b] * e[b];
                }
                Le[a] = sum;
            }
            double q = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) q = q + e[a] * Le[a];
            q_out[k] = q;
            const bool unc = E.uncertain[k] != 0;
            const double l = unc ? E.line[k] : 1.0;
            const double mu = mu_dev ? *mu_dev : 0.0;
            const double sl = sqrt(l) - 1.0;
            f = unc ? l * q + mu * (sl * sl) : q;
            if (!fin_pose) atomicOr(status, (uint32_t)PG_ST_NONFINITE_POSE);
            if (!fin_edge) atomicOr(status, (uint32_t)PG_ST_NONFINITE_EDGE);
            if (FULL) {
                double J[6][6];
                const double Bt[3] = {Ts[3], Ts[7], Ts[11]};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double N[3][3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const double bj[3] = {Ts[j], Ts[4 + j], Ts[8 + j]};
                        double x[3];
                        unit_cross(c, bj, x);
#pragma unroll
                        for (int r = 0; r < 3; ++r) N[r][j] = (A[4 * r] * x[0] + A[4 * r + 1] * x[1]) + A[4 * r + 2] * x[2];
                    }
                    J[0][c] = (N[2][1] - N[1][2]) / 2.0;
                    J[1][c] = (N[0][2] - N[2][0]) / 2.0;
                    J[2][c] = (N[1][0] - N[0][1]) / 2.0;
                    double x[3];
                    unit_cross(c, Bt, x);
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        J[3 + r][c] = (A[4 * r] * x[0] + A[4 * r + 1] * x[1]) + A[4 * r + 2] * x[2];
                        J[r][3 + c] = 0.0;
                        J[3 + r][3 + c] = A[4 * r + c];
                    }
                }
#pragma unroll
                for (int a = 0; a < 6; ++a) e_out[6 * (size_t)k + a] = e[a];
                // g = J^T (L e); W = J^T (L J), one column of L J at a time
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    double sum = 0.0;
#pragma unroll
                    for (int r = 0; r < 6; ++r) sum = sum + J[r][a] * Le[r];
                    g_out[6 * (size_t)k + a] = sum;
                }
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    double LJ[6];
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        double sum = 0.0;
#pragma unroll
                        for (int b = 0; b < 6; ++b) sum = sum + L[6 * r + b] * J[b][c];
                        LJ[r] = sum;
                    }
#pragma unroll
                    for (int a = 0; a < 6; ++a) {
                        double sum = 0.0;
#pragma unroll
                        for (int r = 0; r < 6; ++r) sum = sum + J[r][a] * LJ[r];
                        W_out[36 * (size_t)k + 6 * a + c] = sum;
                    }
                }
            }
        }
    }
    const double tot = block_sum(f, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// One node per lane: H_ii = sum w W and b_i = -sum w J_i^T L e over the node's slots in order; the reference node gets the identity
// and zero.  pmax [2 gridDim.x]: the block's largest diagonal entry of H and largest |b| entry.
__global__ __launch_bounds__(CL_BLOCK) void pg_node(PgGraph G, PgEdges E, const double* __restrict__ W, const double* __restrict__ g,
                                                    int32_t reference, double* __restrict__ Hd, double* __restrict__ b,
                                                    double* __restrict__ pmax, const uint32_t* stop, const uint32_t* guard,
                                                    uint32_t want) {
    if ((stop && *stop) || (guard && *guard != want) || G.head->status) return;
    __shared__ double lds[CL_BLOCK / 64];
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    double dmax = 0.0, bmax = 0.0;
    if (i < G.head->n) {
        double H[36], bi[6];
#pragma unroll
        for (int v = 0; v < 36; ++v) H[v] = 0.0;
#pragma unroll
        for (int v = 0; v < 6; ++v) bi[v] = 0.0;
        if ((int32_t)i == reference) {
#pragma unroll
            for (int v = 0; v < 6; ++v) H[7 * v] = 1.0;
        } else {
            for (uint32_t q = G.row_start[i]; q < G.row_start[i + 1]; ++q) {
                const uint32_t sl = G.slot[q], k = sl >> 1;
                const double w = edge_weight(E, k);
                const double* Wk = W + 36 * (size_t)k;
                const double* gk = g + 6 * (size_t)k;
#pragma unroll
                for (int v = 0; v < 36; ++v) H[v] = H[v] + w * Wk[v];
                if (sl & 1u) {
#pragma unroll
                    for (int v = 0; v < 6; ++v) bi[v] = bi[v] + w * gk[v];
                } else {
#pragma unroll
                    for (int v = 0; v < 6; ++v) bi[v] = bi[v] - w * gk[v];
                }
            }
        }
#pragma unroll
        for (int v = 0; v < 36; ++v) Hd[36 * (size_t)i + v] = H[v];
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            b[6 * (size_t)i + v] = bi[v];
            dmax = fmax(dmax, H[7 * v]);
            bmax = fmax(bmax, fabs(bi[v]));
        }
    }
    dmax = block_max(dmax, lds);
    bmax = block_max(bmax, lds);
    if (threadIdx.x == 0) { pmax[2 * blockIdx.x] = dmax; pmax[2 * blockIdx.x + 1] = bmax; }
}

// ------------------------------------------------------------------------------------------------ PCG
// z = (H_ii + lambda I)^-1 r by the ICP's pivoted LDLT
__device__ inline void block_solve(const double* Hd, double lambda, const double r[6], double z[6]) {
    double A[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 6; ++c) A[a][c] = a == c ? Hd[6 * a + c] + lambda : Hd[6 * a + c];
    ldlt_solve6(A, r, z);
}

struct PgVecs { double *x, *r, *z, *p, *Ap; };

// x = 0, r = b, z = D^-1 r, p = z; partials of r.z and b.b
__global__ __launch_bounds__(CL_BLOCK) void pg_cg_begin(uint32_t n, const double* __restrict__ Hd, const double* __restrict__ b,
                                                        const double* lambda, PgVecs V, double* __restrict__ part, const uint32_t* stop) {
    if (stop && *stop) return;
    __shared__ double lds[CL_BLOCK / 64];
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    double rz = 0.0, bb = 0.0;
    if (i < n) {
        double r[6], z[6];
#pragma unroll
        for (int v = 0; v < 6; ++v) r[v] = b[6 * (size_t)i + v];
        block_solve(Hd + 36 * (size_t)i, *lambda, r, z);
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            V.x[6 * (size_t)i + v] = 0.0;
            V.r[6 * (size_t)i + v] = r[v];
            V.z[6 * (size_t)i + v] = z[v];
            V.p[6 * (size_t)i + v] = z[v];
            rz = rz + r[v] * z[v];
            bb = bb + r[v] * r[v];
        }
    }
    rz = block_sum(rz, lds);
    bb = block_sum(bb, lds);
    if (threadIdx.x == 0) { part[4 * blockIdx.x] = rz; part[4 * blockIdx.x + 1] = bb; }
}

__global__ __launch_bounds__(CL_BLOCK) void pg_cg_begin_fold(const double* __restrict__ part, uint32_t n_part, const double* lambda,
                                                             PgCg* cg, uint32_t* status, const uint32_t* stop) {
    if (stop && *stop) return;
    __shared__ double lds[CL_BLOCK / 64];
    const double rz = fold_sum(part, n_part, 4, 0, lds), bb = fold_sum(part, n_part, 4, 1, lds);
    if (threadIdx.x != 0) return;
    cg->rz = rz; cg->bb = bb; cg->rr = bb; cg->alpha = 0.0; cg->beta = 0.0; cg->lambda = *lambda;
    cg->iters = 0;
    cg->converged = bb == 0.0 ? 1u : 0u;
    cg->done = cg->converged;
    if (!isfinite(rz) || !isfinite(bb)) { atomicOr(status, (uint32_t)PG_ST_CG_BREAKDOWN); cg->done = 1; }
}

// (A p)_i = (H_ii + lambda I) p_i - sum over the node's slots of w W p_t (the node is the source) or w W^T p_s (the target); the
// reference node's row and column hold its identity block alone
__global__ __launch_bounds__(CL_BLOCK) void pg_cg_ap(PgGraph G, PgEdges E, const double* __restrict__ W, const double* __restrict__ Hd,
                                                     int32_t reference, const PgCg* cg, PgVecs V, double* __restrict__ part) {
    if (cg->done) return;
    __shared__ double lds[CL_BLOCK / 64];
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    double pAp = 0.0;
    if (i < G.head->n) {
        double p[6], y[6];
#pragma unroll
        for (int v = 0; v < 6; ++v) p[v] = V.p[6 * (size_t)i + v];
        const double* H = Hd + 36 * (size_t)i;
        const double lambda = cg->lambda;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double sum = 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c) sum = sum + H[6 * a + c] * p[c];
            y[a] = sum + lambda * p[a];
        }
        if ((int32_t)i != reference) {
            for (uint32_t q = G.row_start[i]; q < G.row_start[i + 1]; ++q) {
                const uint32_t sl = G.slot[q], k = sl >> 1;
                const bool is_target = sl & 1u;
                const int32_t other = is_target ? E.src[k] : E.tgt[k];
                if (other == reference) continue;
                const double w = edge_weight(E, k);
                const double* Wk = W + 36 * (size_t)k;
                double po[6];
#pragma unroll
                for (int v = 0; v < 6; ++v) po[v] = V.p[6 * (size_t)other + v];
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    double sum = 0.0;
#pragma unroll
                    for (int c = 0; c < 6; ++c) sum = sum + (is_target ? Wk[6 * c + a] : Wk[6 * a + c]) * po[c];
                    y[a] = y[a] - w * sum;
                }
            }
        }
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            V.Ap[6 * (size_t)i + v] = y[v];
            pAp = pAp + p[v] * y[v];
        }
    }
    pAp = block_sum(pAp, lds);
    if (threadIdx.x == 0) part[4 * blockIdx.x] = pAp;
}

__global__ __launch_bounds__(CL_BLOCK) void pg_cg_alpha(const double* __restrict__ part, uint32_t n_part, PgCg* cg, uint32_t* status) {
    if (cg->done) return;
    __shared__ double lds[CL_BLOCK / 64];
    const double pAp = fold_sum(part, n_part, 4, 0, lds);
    if (threadIdx.x != 0) return;
    if (!(pAp > 0.0) || !isfinite(pAp)) {
        atomicOr(status, (uint32_t)PG_ST_CG_BREAKDOWN);
        cg->done = 1;
        return;
    }
    cg->alpha = cg->rz / pAp;
}

__global__ __launch_bounds__(CL_BLOCK) void pg_cg_update(uint32_t n, const double* __restrict__ Hd, const PgCg* cg, PgVecs V,
                                                         double* __restrict__ part) {
    if (cg->done) return;
    __shared__ double lds[CL_BLOCK / 64];
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    double rz = 0.0, rr = 0.0;
    if (i < n) {
        const double alpha = cg->alpha;
        double r[6], z[6];
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            V.x[6 * (size_t)i + v] = V.x[6 * (size_t)i + v] + alpha * V.p[6 * (size_t)i + v];
            r[v] = V.r[6 * (size_t)i + v] - alpha * V.Ap[6 * (size_t)i + v];
        }
        block_solve(Hd + 36 * (size_t)i, cg->lambda, r, z);
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            V.r[6 * (size_t)i + v] = r[v];
            V.z[6 * (size_t)i + v] = z[v];
            rz = rz + r[v] * z[v];
            rr = rr + r[v] * r[v];
        }
    }
    rz = block_sum(rz, lds);
    rr = block_sum(rr, lds);
    if (threadIdx.x == 0) { part[4 * blockIdx.x] = rz; part[4 * blockIdx.x + 1] = rr; }
}

__global__ __launch_bounds__(CL_BLOCK) void pg_cg_beta(const double* __restrict__ part, uint32_t n_part, double rtol, PgCg* cg,
                                                       uint32_t* status) {
    if (cg->done) return;
    __shared__ double lds[CL_BLOCK / 64];
    const double rz = fold_sum(part, n_part, 4, 0, lds), rr = fold_sum(part, n_part, 4, 1, lds);
    if (threadIdx.x != 0) return;
    cg->iters += 1;
    cg->rr = rr;
    if (!isfinite(rz) || !isfinite(rr)) {
        atomicOr(status, (uint32_t)PG_ST_CG_BREAKDOWN);
        cg->done = 1;
        return;
    }
    if (sqrt(rr) <= rtol * sqrt(cg->bb)) { cg->converged = 1; cg->done = 1; return; }
    cg->beta = rz / cg->rz;
    cg->rz = rz;
}

__global__ __launch_bounds__(CL_BLOCK) void pg_cg_p(uint32_t n, const PgCg* cg, PgVecs V) {
    if (cg->done) return;
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= 6 * n) return;
    V.p[i] = V.z[i] + cg->beta * V.p[i];
}

// the standalone solve's first launch: a refused graph solves nothing (its status stops the first two launches and ends the rest)
__global__ void pg_set_lambda(double* slot, double lambda, uint32_t* status, const PgHead* h, PgCg* cg) {
    *slot = lambda;
    *status = h->status;
    cg->done = h->status ? 1u : 0u;
}

__global__ void pg_solve_end(const PgCg* cg, const uint32_t* status, int64_t* info) {
    info[0] = *status; info[1] = cg->iters; info[2] = cg->converged; info[3] = 0;
}

__global__ void pg_linearize_end(const uint32_t* status, const PgHead* h, int64_t* info) {
    info[0] = *status | h->status; info[1] = 0; info[2] = 0; info[3] = 0;
}

// ------------------------------------------------------------------------------------------------ Levenberg-Marquardt
// one workgroup: mu = preference * distance^2 * mean of L[5][5] over the uncertain edges (0 without one), and the state's first values
__global__ __launch_bounds__(CL_BLOCK) void pg_lm_begin(PgEdges E, const PgHead* h, double scale, PgLm* lm) {
    __shared__ double lds[CL_BLOCK / 64];
    double s = 0.0, c = 0.0;
    for (uint32_t k = threadIdx.x; k < E.m; k += CL_BLOCK)
        if (E.uncertain[k]) { s = s + E.info[36 * (size_t)k + 35]; c = c + 1.0; }
    s = block_sum(s, lds);
    c = block_sum(c, lds);
    if (threadIdx.x != 0) return;
    lm->mu = c > 0.0 ? scale * (s / c) : 0.0;
    lm->lambda = 0.0; lm->nu = 2.0; lm->F = 0.0; lm->F_new = 0.0; lm->rho = 0.0; lm->b_inf = 0.0; lm->max_diag = 0.0;
    lm->stop = 0; lm->reason = PG_STOP_NONE; lm->accepted_now = 0; lm->accepts = 0; lm->rejects = 0; lm->consecutive = 0; lm->trials = 0;
    lm->status = h->status;
    lm->capped = 0; lm->pad = 0;
    lm->cg_total = 0;
    if (h->status) { lm->stop = 1; lm->reason = PG_STOP_STATUS; }
}

__global__ __launch_bounds__(CL_BLOCK) void pg_fill(double* a, uint32_t n, double v) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i < n) a[i] = v;
}

// one workgroup, after a linearisation: F, |b|_inf, the largest diagonal entry; FIRST: lambda0 = 1e-5 max diag H; else the stops an
// accepted step can reach
template <bool FIRST>
__global__ __launch_bounds__(CL_BLOCK) void pg_lm_after(const double* __restrict__ partE, uint32_t nbE, const double* __restrict__ pmax,
                                                        uint32_t nbN, PgLm* lm, int32_t max_iteration, double min_right_term,
                                                        double min_residual) {
    if (lm->stop || (!FIRST && !lm->accepted_now)) return;
    __shared__ double lds[CL_BLOCK / 64];
    const double F = fold_sum(partE, nbE, 1, 0, lds);
    const double dmax = fold_max(pmax, nbN, 2, 0, lds), bmax = fold_max(pmax, nbN, 2, 1, lds);
    if (threadIdx.x != 0) return;
    lm->F = F; lm->b_inf = bmax; lm->max_diag = dmax;
    if (FIRST) lm->lambda = 1e-5 * dmax;
    uint32_t reason = PG_STOP_NONE;
    if (lm->status || !isfinite(F)) reason = PG_STOP_STATUS;
    else if (bmax < min_right_term) reason = PG_STOP_RIGHT_TERM;
    else if (!FIRST && F < min_residual) reason = PG_STOP_RESIDUAL;
    else if ((int32_t)lm->accepts >= max_iteration) reason = PG_STOP_MAX_ITERATION;
    if (reason) { lm->stop = 1; lm->reason = reason; }
}

// trial poses T' = M(d) T (the ICP's composition) and the partials of d.d, |t|^2 and d.(lambda d + b)
__global__ __launch_bounds__(CL_BLOCK) void pg_trial(uint32_t n, const double* __restrict__ poses, const double* __restrict__ delta,
                                                     const double* __restrict__ b, const PgLm* lm, double* __restrict__ trial,
                                                     double* __restrict__ part) {
    if (lm->stop) return;
    __shared__ double lds[CL_BLOCK / 64];
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    double dd = 0.0, xx = 0.0, den = 0.0;
    if (i < n) {
        const double lambda = lm->lambda;
        double d[6], U[16];
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            d[v] = delta[6 * (size_t)i + v];
            dd = dd + d[v] * d[v];
            den = den + d[v] * (lambda * d[v] + b[6 * (size_t)i + v]);
        }
        step_matrix(d, U);
        const double* T = poses + 16 * (size_t)i;
        double* O = trial + 16 * (size_t)i;
        for (int a = 0; a < 4; ++a)
            for (int c = 0; c < 4; ++c)
                O[4 * a + c] = ((U[4 * a] * T[c] + U[4 * a + 1] * T[4 + c]) + U[4 * a + 2] * T[8 + c]) + U[4 * a + 3] * T[12 + c];
        xx = (T[3] * T[3] + T[7] * T[7]) + T[11] * T[11];
    }
    dd = block_sum(dd, lds);
    xx = block_sum(xx, lds);
    den = block_sum(den, lds);
    if (threadIdx.x == 0) { part[4 * blockIdx.x] = dd; part[4 * blockIdx.x + 1] = xx; part[4 * blockIdx.x + 2] = den; }
}

// one workgroup: the gain ratio and the schedule
__global__ __launch_bounds__(CL_BLOCK) void pg_decide(const double* __restrict__ partE, uint32_t nbE, const double* __restrict__ partN,
                                                      uint32_t nbN, const PgCg* cg, PgLm* lm, const uint32_t* status,
                                                      int32_t max_iteration_lm, double min_relative_increment, int32_t* history,
                                                      int32_t history_capacity) {
    if (lm->stop) return;
    __shared__ double lds[CL_BLOCK / 64];
    const double F_new = fold_sum(partE, nbE, 1, 0, lds);
    const double dd = fold_sum(partN, nbN, 4, 0, lds), xx = fold_sum(partN, nbN, 4, 1, lds), den = fold_sum(partN, nbN, 4, 2, lds);
    if (threadIdx.x != 0) return;
    lm->accepted_now = 0;
    lm->cg_total += cg->iters;
    lm->capped += cg->converged ? 0u : 1u;
    lm->status |= *status;
    if (lm->status) { lm->stop = 1; lm->reason = PG_STOP_STATUS; return; }
    const uint32_t trial = lm->trials;
    lm->trials = trial + 1;
    lm->F_new = F_new;
    if (sqrt(dd) <= min_relative_increment * (sqrt(xx) + min_relative_increment)) {
        lm->stop = 1; lm->reason = PG_STOP_RELATIVE_INCREMENT;
        if (history && (int32_t)trial < history_capacity) history[trial] = -1;
        return;
    }
    const double rho = (lm->F - F_new) / den;
    lm->rho = rho;
    if (rho > 0.0) {
        const double u = 2.0 * rho - 1.0;
        lm->lambda = lm->lambda * fmax(1.0 / 3.0, 1.0 - (u * u) * u);
        lm->nu = 2.0;
        lm->accepted_now = 1;
        lm->accepts += 1;
        lm->consecutive = 0;
    } else {
        lm->lambda = lm->lambda * lm->nu;
        lm->nu = lm->nu * 2.0;
        lm->rejects += 1;
        lm->consecutive += 1;
        if ((int32_t)lm->consecutive >= max_iteration_lm) { lm->stop = 1; lm->reason = PG_STOP_MAX_ITERATION_LM; }
    }
    if (history && (int32_t)trial < history_capacity) history[trial] = rho > 0.0 ? 1 : 0;
}

// an accepted step: the trial poses become the poses, and every uncertain edge's line value follows its new residual
__global__ __launch_bounds__(CL_BLOCK) void pg_accept(uint32_t n, uint32_t m, const PgLm* lm, const double* __restrict__ trial,
                                                      double* __restrict__ poses, const int32_t* __restrict__ uncertain,
                                                      const double* __restrict__ q, double* __restrict__ line) {
    if (!lm->accepted_now) return;
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i < 16 * n) poses[i] = trial[i];
    if (i < m && uncertain[i]) {
        const double mu = lm->mu, f = mu > 0.0 ? mu / (mu + q[i]) : 1.0;      // mu = 0 (every uncertain L[5][5] is 0): no line process
        line[i] = f * f;
    }
}

__global__ void pg_lm_end(const PgLm* lm, double* result, int64_t* info) {
    result[0] = lm->F; result[1] = lm->b_inf; result[2] = lm->lambda; result[3] = lm->mu;
    info[0] = lm->status; info[1] = lm->trials; info[2] = (int64_t)lm->cg_total; info[3] = lm->accepts; info[4] = lm->rejects;
    info[5] = lm->reason; info[6] = lm->stop; info[7] = lm->capped;
}

// ------------------------------------------------------------------------------------------------ host
struct PgLayout { size_t lm, cg, lambda, e, q, W, g, Hd, b, delta, trial, r, z, p, Ap, partE, partN, pmax, total; SortLayout sort; };
PgLayout pg_layout(int64_t n, int64_t m) {
    PgLayout l;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = align256(o + bytes); return at; };
    const size_t N = (size_t)n, M = (size_t)m;
    l.lm = take(sizeof(PgLm)); l.cg = take(sizeof(PgCg)); l.lambda = take(16);
    l.e = take(48 * M); l.q = take(8 * M); l.W = take(288 * M); l.g = take(48 * M);
    l.Hd = take(288 * N); l.b = take(48 * N); l.delta = take(48 * N); l.trial = take(128 * N);
    l.r = take(48 * N); l.z = take(48 * N); l.p = take(48 * N); l.Ap = take(48 * N);
    l.partE = take(8 * (size_t)pg_blocks(m)); l.partN = take(32 * (size_t)pg_blocks(n)); l.pmax = take(16 * (size_t)pg_blocks(n));
    l.sort = sort_layout(o, 2 * m > 0 ? 2 * m : 1, 0);
    l.total = l.sort.end;
    return l;
}

bool sizes_ok(int64_t n, int64_t m) { return n >= 1 && n <= PG_MAX_NODES && m >= 0 && m <= PG_MAX_EDGES; }

#define PG_REQUIRE_SIZES(fn, n, m)                                                                                              \
    LNR_REQUIRE(sizes_ok(n, m), fn ": %lld nodes and %lld edges; nodes must be in [1, %lld] and edges in [0, %lld]", (long long)(n), \
                (long long)(m), (long long)PG_MAX_NODES, (long long)PG_MAX_EDGES)

int reference_ok(const char* fn, int32_t reference, int64_t n) {
    LNR_REQUIRE(reference >= -1 && reference < n, "%s: reference_node must be -1 or a node in [0, %lld), got %d", fn, (long long)n,
                (int)reference);
    return LNR_OK;
}

struct PgSolveArgs {
    PgGraph G; PgEdges E; const double* W; const double* Hd; const double* b; const double* lambda; int32_t reference; double rtol;
    int32_t max_cg; PgVecs V; double* part; PgCg* cg; uint32_t* status; const uint32_t* stop; uint32_t n;
};

// every PCG iteration, enqueued; nothing is read back
void enqueue_solve(const PgSolveArgs& a, hipStream_t st) {
    const uint32_t nb = pg_blocks(a.n);
    hipLaunchKernelGGL(pg_cg_begin, dim3(nb), dim3(CL_BLOCK), 0, st, a.n, a.Hd, a.b, a.lambda, a.V, a.part, a.stop);
    hipLaunchKernelGGL(pg_cg_begin_fold, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)a.part, nb, a.lambda, a.cg, a.status, a.stop);
    for (int it = 0; it < a.max_cg; ++it) {
        hipLaunchKernelGGL(pg_cg_ap, dim3(nb), dim3(CL_BLOCK), 0, st, a.G, a.E, a.W, a.Hd, a.reference, (const PgCg*)a.cg, a.V, a.part);
        hipLaunchKernelGGL(pg_cg_alpha, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)a.part, nb, a.cg, a.status);
        hipLaunchKernelGGL(pg_cg_update, dim3(nb), dim3(CL_BLOCK), 0, st, a.n, a.Hd, (const PgCg*)a.cg, a.V, a.part);
        hipLaunchKernelGGL(pg_cg_beta, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)a.part, nb, a.rtol, a.cg, a.status);
        hipLaunchKernelGGL(pg_cg_p, dim3(blocks_for(6ull * a.n)), dim3(CL_BLOCK), 0, st, a.n, (const PgCg*)a.cg, a.V);
    }
}

int edges_ok(const char* fn, int64_t m, const void* a, const void* b, const void* c, const void* d, const void* e, const void* f) {
    LNR_REQUIRE(m == 0 || (a && b && c && d && e && f), "%s: null argument", fn);
    return LNR_OK;
}

}  // namespace

extern "C" size_t lnr_pose_graph_bytes(int64_t n_nodes, int64_t n_edges) {
    return sizes_ok(n_nodes, n_edges) ? graph_layout(n_nodes, n_edges).total : 0;
}

extern "C" size_t lnr_pose_graph_workspace(int64_t n_nodes, int64_t n_edges) {
    return sizes_ok(n_nodes, n_edges) ? pg_layout(n_nodes, n_edges).total : 0;
}

extern "C" int lnr_pose_graph_build(const int32_t* source, const int32_t* target, int64_t n_nodes, int64_t n_edges, void* graph,
                                    size_t graph_bytes, void* workspace, size_t workspace_bytes, int64_t* info_dev, void* stream) {
    PG_REQUIRE_SIZES("lnr_pose_graph_build", n_nodes, n_edges);
    LNR_REQUIRE(graph && workspace && info_dev && (n_edges == 0 || (source && target)), "lnr_pose_graph_build: null argument");
    const PgGraphLayout gl = graph_layout(n_nodes, n_edges);
    const PgLayout l = pg_layout(n_nodes, n_edges);
    LNR_REQUIRE(graph_bytes >= gl.total, "lnr_pose_graph_build: graph of %zu bytes, %zu needed", graph_bytes, gl.total);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_pose_graph_build: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("pose_graph_build", st);
    char* gb = (char*)graph;
    PgHead* h = (PgHead*)(gb + gl.head);
    uint32_t* row_start = (uint32_t*)(gb + gl.row_start);
    uint32_t* slot = (uint32_t*)(gb + gl.slot);
    const uint32_t n = (uint32_t)n_nodes, m = (uint32_t)n_edges, L = 2 * m;
    const uint32_t shift = L > 1 ? bit_length((int64_t)L - 1) : 1u;
    const int32_t npasses = (int32_t)((shift + bit_length(n_nodes) + 7) / 8);
    hipLaunchKernelGGL(pg_begin, dim3(1), dim3(1), 0, st, h, n, m, npasses, shift);
    const RadixBuffers rb = radix_buffers((char*)workspace, l.sort, L > 0 ? (int64_t)L : 1);
    if (L > 0) {
        hipLaunchKernelGGL(pg_keys, dim3(blocks_for(L)), dim3(CL_BLOCK), 0, st, h, source, target, rb.ka, rb.ia);
        enqueue_radix_sort(rb, &h->n_sort, &h->npasses, st);
    }
    const uint32_t span = L > n + 1 ? L : n + 1;
    hipLaunchKernelGGL(pg_rows, dim3(blocks_for(span)), dim3(CL_BLOCK), 0, st, (const PgHead*)h, sorted_pairs(rb), row_start, slot);
    hipLaunchKernelGGL(pg_build_end, dim3(1), dim3(1), 0, st, (const PgHead*)h, info_dev);
    LNR_CHECK_LAUNCH("lnr_pose_graph_build");
    return LNR_OK;
}

extern "C" int lnr_pose_graph_linearize(const void* graph, int64_t n_nodes, int64_t n_edges, const int32_t* source, const int32_t* target,
                                        const double* poses, const double* measurements, const double* information,
                                        const int32_t* uncertain, const double* line, int32_t reference_node, double* e, double* q,
                                        double* W, double* g, double* H_diag, double* b, void* workspace, size_t workspace_bytes,
                                        int64_t* info_dev, void* stream) {
    PG_REQUIRE_SIZES("lnr_pose_graph_linearize", n_nodes, n_edges);
    if (int rc = reference_ok("lnr_pose_graph_linearize", reference_node, n_nodes)) return rc;
    LNR_REQUIRE(graph && poses && H_diag && b && workspace && info_dev, "lnr_pose_graph_linearize: null argument");
    if (int rc = edges_ok("lnr_pose_graph_linearize", n_edges, source, target, measurements, information, uncertain, line)) return rc;
    LNR_REQUIRE(n_edges == 0 || (e && q && W && g), "lnr_pose_graph_linearize: null argument");
    const PgLayout l = pg_layout(n_nodes, n_edges);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_pose_graph_linearize: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("pose_graph_linearize", st);
    char* ws = (char*)workspace;
    PgLm* lm = (PgLm*)(ws + l.lm);
    const PgGraph G = graph_view(graph, n_nodes, n_edges);
    const PgEdges E = {source, target, measurements, information, uncertain, line, (uint32_t)n_edges};
    const uint32_t n = (uint32_t)n_nodes, nbE = pg_blocks(n_edges), nbN = pg_blocks(n_nodes);
    const uint32_t* none = nullptr;
    if (int rc = clear_words(&lm->status, 4, st, "lnr_pose_graph_linearize", "status")) return rc;
    hipLaunchKernelGGL(pg_edge<true>, dim3(nbE), dim3(CL_BLOCK), 0, st, E, n, poses, (const double*)nullptr, e, q, W, g,
                       (double*)(ws + l.partE), &lm->status, none, none, 0u);
    hipLaunchKernelGGL(pg_node, dim3(nbN), dim3(CL_BLOCK), 0, st, G, E, (const double*)W, (const double*)g, reference_node, H_diag, b,
                       (double*)(ws + l.pmax), none, none, 0u);
    hipLaunchKernelGGL(pg_linearize_end, dim3(1), dim3(1), 0, st, (const uint32_t*)&lm->status, G.head, info_dev);
    LNR_CHECK_LAUNCH("lnr_pose_graph_linearize");
    return LNR_OK;
}

extern "C" int lnr_pose_graph_solve(const void* graph, int64_t n_nodes, int64_t n_edges, const int32_t* source, const int32_t* target,
                                    const double* W, const int32_t* uncertain, const double* line, const double* H_diag, const double* b,
                                    double lambda, int32_t reference_node, double rtol, int32_t max_cg, void* workspace,
                                    size_t workspace_bytes, double* delta, int64_t* info_dev, void* stream) {
    PG_REQUIRE_SIZES("lnr_pose_graph_solve", n_nodes, n_edges);
    if (int rc = reference_ok("lnr_pose_graph_solve", reference_node, n_nodes)) return rc;
    LNR_REQUIRE(isfinite(lambda) && lambda >= 0.0, "lnr_pose_graph_solve: lambda must be finite and >= 0, got %g", lambda);
    LNR_REQUIRE(isfinite(rtol) && rtol >= 0.0, "lnr_pose_graph_solve: rtol must be finite and >= 0, got %g", rtol);
    LNR_REQUIRE(max_cg >= 1 && max_cg <= 100000, "lnr_pose_graph_solve: max_cg must be in [1, 100000], got %d", (int)max_cg);
    LNR_REQUIRE(graph && H_diag && b && workspace && delta && info_dev, "lnr_pose_graph_solve: null argument");
    if (int rc = edges_ok("lnr_pose_graph_solve", n_edges, source, target, W, uncertain, line, W)) return rc;
    const PgLayout l = pg_layout(n_nodes, n_edges);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_pose_graph_solve: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("pose_graph_solve", st);
    char* ws = (char*)workspace;
    PgLm* lm = (PgLm*)(ws + l.lm);
    PgCg* cg = (PgCg*)(ws + l.cg);
    double* lam = (double*)(ws + l.lambda);
    const PgGraph G = graph_view(graph, n_nodes, n_edges);
    const PgEdges E = {source, target, nullptr, nullptr, uncertain, line, (uint32_t)n_edges};
    const PgVecs V = {delta, (double*)(ws + l.r), (double*)(ws + l.z), (double*)(ws + l.p), (double*)(ws + l.Ap)};
    if (int rc = clear_words(cg, sizeof(PgCg), st, "lnr_pose_graph_solve", "state")) return rc;
    if (int rc = clear_words(delta, 48 * (size_t)n_nodes, st, "lnr_pose_graph_solve", "step")) return rc;
    hipLaunchKernelGGL(pg_set_lambda, dim3(1), dim3(1), 0, st, lam, lambda, &lm->status, G.head, cg);
    const PgSolveArgs a = {G, E, W, H_diag, b, lam, reference_node, rtol, max_cg, V, (double*)(ws + l.partN), cg, &lm->status,
                           (const uint32_t*)&lm->status, (uint32_t)n_nodes};
    enqueue_solve(a, st);
    hipLaunchKernelGGL(pg_solve_end, dim3(1), dim3(1), 0, st, (const PgCg*)cg, (const uint32_t*)&lm->status, info_dev);
    LNR_CHECK_LAUNCH("lnr_pose_graph_solve");
    return LNR_OK;
}

extern "C" int lnr_pose_graph_optimize(const void* graph, int64_t n_nodes, int64_t n_edges, const int32_t* source, const int32_t* target,
                                       double* poses, const double* measurements, const double* information, const int32_t* uncertain,
                                       double* line, int32_t reference_node, double max_correspondence_distance,
                                       double preference_loop_closure, int32_t max_iteration, int32_t max_iteration_lm,
                                       double min_relative_increment, double min_right_term, double min_residual, double rtol,
                                       int32_t max_cg, void* workspace, size_t workspace_bytes, int32_t* history_dev,
                                       int32_t history_capacity, double* result_dev, int64_t* info_dev, void* stream) {
    const char* fn = "lnr_pose_graph_optimize";
    PG_REQUIRE_SIZES("lnr_pose_graph_optimize", n_nodes, n_edges);
    if (int rc = reference_ok(fn, reference_node, n_nodes)) return rc;
    LNR_REQUIRE(isfinite(max_correspondence_distance) && max_correspondence_distance > 0.0,
                "%s: max_correspondence_distance must be finite and > 0, got %g", fn, max_correspondence_distance);
    LNR_REQUIRE(isfinite(preference_loop_closure) && preference_loop_closure > 0.0,
                "%s: preference_loop_closure must be finite and > 0, got %g", fn, preference_loop_closure);
    LNR_REQUIRE(max_iteration >= 0 && max_iteration <= 10000, "%s: max_iteration must be in [0, 10000], got %d", fn, (int)max_iteration);
    LNR_REQUIRE(max_iteration_lm >= 1 && max_iteration_lm <= 1000, "%s: max_iteration_lm must be in [1, 1000], got %d", fn,
                (int)max_iteration_lm);
    LNR_REQUIRE(min_relative_increment >= 0.0 && min_right_term >= 0.0 && min_residual >= 0.0,
                "%s: min_relative_increment, min_right_term and min_residual must be >= 0", fn);
    LNR_REQUIRE(isfinite(rtol) && rtol >= 0.0, "%s: rtol must be finite and >= 0, got %g", fn, rtol);
    LNR_REQUIRE(max_cg >= 1 && max_cg <= 100000, "%s: max_cg must be in [1, 100000], got %d", fn, (int)max_cg);
    LNR_REQUIRE(history_capacity >= 0 && (history_capacity == 0 || history_dev), "%s: history_capacity without history_dev", fn);
    LNR_REQUIRE(graph && poses && workspace && result_dev && info_dev, "%s: null argument", fn);
    if (int rc = edges_ok(fn, n_edges, source, target, measurements, information, uncertain, line)) return rc;
    const PgLayout l = pg_layout(n_nodes, n_edges);
    LNR_REQUIRE(workspace_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("pose_graph_optimize", st);
    char* ws = (char*)workspace;
    PgLm* lm = (PgLm*)(ws + l.lm);
    PgCg* cg = (PgCg*)(ws + l.cg);
    double *e = (double*)(ws + l.e), *q = (double*)(ws + l.q), *W = (double*)(ws + l.W), *g = (double*)(ws + l.g);
    double *Hd = (double*)(ws + l.Hd), *b = (double*)(ws + l.b), *delta = (double*)(ws + l.delta), *trial = (double*)(ws + l.trial);
    double *partE = (double*)(ws + l.partE), *partN = (double*)(ws + l.partN), *pmax = (double*)(ws + l.pmax);
    const PgGraph G = graph_view(graph, n_nodes, n_edges);
    const PgEdges E = {source, target, measurements, information, uncertain, line, (uint32_t)n_edges};
    const uint32_t n = (uint32_t)n_nodes, m = (uint32_t)n_edges, nbE = pg_blocks(n_edges), nbN = pg_blocks(n_nodes);
    const PgVecs V = {delta, (double*)(ws + l.r), (double*)(ws + l.z), (double*)(ws + l.p), (double*)(ws + l.Ap)};
    const uint32_t* none = nullptr;
    const double scale = preference_loop_closure * (max_correspondence_distance * max_correspondence_distance);
    if (history_capacity > 0)
        if (int rc = clear_words(history_dev, 4 * (size_t)history_capacity, st, fn, "history")) return rc;
    if (int rc = clear_words(cg, sizeof(PgCg), st, fn, "state")) return rc;
    if (m) hipLaunchKernelGGL(pg_fill, dim3(blocks_for(m)), dim3(CL_BLOCK), 0, st, line, m, 1.0);
    hipLaunchKernelGGL(pg_lm_begin, dim3(1), dim3(CL_BLOCK), 0, st, E, G.head, scale, lm);
    hipLaunchKernelGGL(pg_edge<true>, dim3(nbE), dim3(CL_BLOCK), 0, st, E, n, (const double*)poses, (const double*)&lm->mu, e, q, W, g,
                       partE, &lm->status, (const uint32_t*)&lm->stop, none, 0u);
    hipLaunchKernelGGL(pg_node, dim3(nbN), dim3(CL_BLOCK), 0, st, G, E, (const double*)W, (const double*)g, reference_node, Hd, b, pmax,
                       (const uint32_t*)&lm->stop, none, 0u);
    hipLaunchKernelGGL(pg_lm_after<true>, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)partE, nbE, (const double*)pmax, nbN, lm,
                       max_iteration, min_right_term, min_residual);
    LNR_CHECK_LAUNCH(fn);
    const PgSolveArgs sa = {G, E, W, Hd, b, &lm->lambda, reference_node, rtol, max_cg, V, partN, cg, &lm->status,
                            (const uint32_t*)&lm->stop, n};
    const uint32_t span = 16 * n > m ? 16 * n : m;
    const int64_t max_trials = (int64_t)max_iteration * ((int64_t)max_iteration_lm + 1);
    for (int64_t trial_no = 0; trial_no < max_trials; ++trial_no) {
        uint32_t stop = 0;                                   // the one host read of this trial
        if (hipMemcpyAsync(&stop, &lm->stop, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            lnr_set_error("%s: reading the stop word failed", fn);
            return LNR_ERR_LAUNCH;
        }
        if (stop) break;
        enqueue_solve(sa, st);
        hipLaunchKernelGGL(pg_trial, dim3(nbN), dim3(CL_BLOCK), 0, st, n, (const double*)poses, (const double*)delta, (const double*)b,
                           (const PgLm*)lm, trial, partN);
        hipLaunchKernelGGL(pg_edge<false>, dim3(nbE), dim3(CL_BLOCK), 0, st, E, n, (const double*)trial, (const double*)&lm->mu, e, q, W, g,
                           partE, &lm->status, (const uint32_t*)&lm->stop, none, 0u);
        hipLaunchKernelGGL(pg_decide, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)partE, nbE, (const double*)partN, nbN, (const PgCg*)cg,
                           lm, (const uint32_t*)&lm->status, max_iteration_lm, min_relative_increment, history_dev, history_capacity);
        hipLaunchKernelGGL(pg_accept, dim3(blocks_for(span)), dim3(CL_BLOCK), 0, st, n, m, (const PgLm*)lm, (const double*)trial, poses,
                           uncertain, (const double*)q, line);
        hipLaunchKernelGGL(pg_edge<true>, dim3(nbE), dim3(CL_BLOCK), 0, st, E, n, (const double*)poses, (const double*)&lm->mu, e, q, W, g,
                           partE, &lm->status, (const uint32_t*)&lm->stop, (const uint32_t*)&lm->accepted_now, 1u);
        hipLaunchKernelGGL(pg_node, dim3(nbN), dim3(CL_BLOCK), 0, st, G, E, (const double*)W, (const double*)g, reference_node, Hd, b, pmax,
                           (const uint32_t*)&lm->stop, (const uint32_t*)&lm->accepted_now, 1u);
        hipLaunchKernelGGL(pg_lm_after<false>, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)partE, nbE, (const double*)pmax, nbN, lm,
                           max_iteration, min_right_term, min_residual);
        LNR_CHECK_LAUNCH(fn);
    }
    hipLaunchKernelGGL(pg_lm_end, dim3(1), dim3(1), 0, st, (const PgLm*)lm, result_dev, info_dev);
    LNR_CHECK_LAUNCH(fn);
    return LNR_OK;
}
