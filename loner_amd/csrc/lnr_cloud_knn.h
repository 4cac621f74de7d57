// The k nearest neighbours of every point of a nearest-neighbour grid, shared by lnr_icp.hip (normals) and lnr_cloud_tools.hip (the mean
// neighbour distance of the outlier filter): the sorted list of one query, the shell walk with the k-th best in its stop rule, and the
// exact pass for queries still open after NN_MAX_SHELL shells.  What is done with a finished list is the caller's `Finish`:
//   fin(g, L, k, out)    L holds the min(k, n) smallest (d2, input index) pairs ascending; out is the query's input index
// Both sources are compiled with -ffp-contract=off (build.py EXACT).
#pragma once
#include "lnr_cloud_grid.h"

namespace {

// The k best (d2, input index) of one query, ascending, in statically indexed registers (every loop over the list is unrolled: a
// runtime-indexed private array would live in scratch).  pos: the sorted grid slot of each entry, for its coordinates.
struct KnnList {
    double d[LNR_KNN_MAX];
    uint32_t id[LNR_KNN_MAX], pos[LNR_KNN_MAX];
    uint32_t found;

    __device__ inline void clear() {
#pragma unroll
        for (int j = 0; j < LNR_KNN_MAX; ++j) { d[j] = INFINITY; id[j] = 0xffffffffu; pos[j] = 0; }
        found = 0;
    }
    // insertion into the sorted list: slot j takes its predecessor, the candidate or itself (top down, so each step reads old values)
    __device__ inline void insert(double cd, uint32_t cid, uint32_t cpos) {
        if (!pair_less(cd, cid, d[LNR_KNN_MAX - 1], id[LNR_KNN_MAX - 1])) return;
        found += found < LNR_KNN_MAX ? 1u : 0u;
#pragma unroll
        for (int j = LNR_KNN_MAX - 1; j > 0; --j) {
            const bool before_prev = pair_less(cd, cid, d[j - 1], id[j - 1]);
            const bool before_here = pair_less(cd, cid, d[j], id[j]);
            d[j] = before_prev ? d[j - 1] : (before_here ? cd : d[j]);
            id[j] = before_prev ? id[j - 1] : (before_here ? cid : id[j]);
            pos[j] = before_prev ? pos[j - 1] : (before_here ? cpos : pos[j]);
        }
        const bool first = pair_less(cd, cid, d[0], id[0]);
        d[0] = first ? cd : d[0];
        id[0] = first ? cid : id[0];
        pos[0] = first ? cpos : pos[0];
    }
    // d2 of the k-th entry (INFINITY while fewer than k are known), by selects rather than a runtime index
    __device__ inline double kth(int k) const {
        double v = INFINITY;
#pragma unroll
        for (int j = 0; j < LNR_KNN_MAX; ++j) v = j == k - 1 ? d[j] : v;
        return v;
    }
};

// one query per thread: sorted target i (consecutive threads take neighbouring points), finished at its input index.
// counters: [0] queries left to the exact pass (their sorted slots go to fallback), [2] shells visited
template <class Finish>
__global__ __launch_bounds__(CL_BLOCK) void knn_shells(GridView g, int k, Finish fin, uint32_t* __restrict__ fallback,
                                                       unsigned long long* __restrict__ counters) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    unsigned long long shells = 0;
    if (i < g.p->n) {
        const double* qp = g.pts + 3 * (size_t)i;
        const ShellQuery s = shell_query(g.p, qp[0], qp[1], qp[2]);
        KnnList L;
        L.clear();
        auto visit = [&](uint32_t j) { L.insert(sq_dist(s.q[0], s.q[1], s.q[2], g.pts + 3 * (size_t)j), g.orig[j], j); };
        bool done = false;
        for (int r = 0; r <= NN_MAX_SHELL && !done; ++r) {
            ++shells;
            const double lb = shell_visit(g, s, r, visit);
            done = lb == INFINITY || L.kth(k) < lb;             // strict: an unvisited target at the same d2 could have a lower index
        }
        if (done) fin(g, L, k, g.orig[i]);
        else fallback[atomicAdd(&counters[0], 1ull)] = i;
    }
    shells = wave_sum(shells);
    if ((threadIdx.x & 63) == 0 && shells) atomicAdd(&counters[2], shells);
}

// the exact fallback: nn_brute's tile loop (lnr_cloud.hip) with each target's input index beside it
template <class Finish>
__global__ __launch_bounds__(CL_BLOCK) void knn_brute(GridView g, int k, Finish fin, const uint32_t* __restrict__ fallback,
                                                      const unsigned long long* __restrict__ counters) {
    __shared__ double tile[NN_FB_TILE * 3];
    __shared__ uint32_t tile_id[NN_FB_TILE];
    const uint32_t n_fb = (uint32_t)counters[0];
    if ((uint64_t)blockIdx.x * CL_BLOCK >= n_fb) return;
    const uint32_t f = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool active = f < n_fb;
    const uint32_t i = active ? fallback[f] : 0u;
    const double qx = g.pts[3 * (size_t)i], qy = g.pts[3 * (size_t)i + 1], qz = g.pts[3 * (size_t)i + 2];
    const uint32_t n = g.p->n;
    KnnList L;
    L.clear();
    for (uint32_t t0 = 0; t0 < n; t0 += NN_FB_TILE) {
        const uint32_t m = n - t0 < NN_FB_TILE ? n - t0 : NN_FB_TILE;
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < 3 * m; e += CL_BLOCK) tile[e] = g.pts[3 * (size_t)t0 + e];
        for (uint32_t e = threadIdx.x; e < m; e += CL_BLOCK) tile_id[e] = g.orig[t0 + e];
        __syncthreads();
        for (uint32_t j = 0; j < m; ++j) L.insert(sq_dist(qx, qy, qz, tile + 3 * j), tile_id[j], t0 + j);
    }
    if (active) fin(g, L, k, g.orig[i]);
}

// a grid unusable for its own points (a non-finite target, or another count than the call's): counters[1] = 1
__global__ void grid_status(const CloudParams* __restrict__ p, uint32_t n, unsigned long long* __restrict__ counters) {
    if (p->status || p->n != n) counters[1] = 1ull;
}

// the whole search on the stream: shells, the exact pass, the grid's status.  fallback: n uint32
template <class Finish>
void enqueue_knn(const GridView& g, uint32_t n, int k, const Finish& fin, uint32_t* fallback, unsigned long long* counters, hipStream_t st) {
    hipLaunchKernelGGL(knn_shells<Finish>, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, g, k, fin, fallback, counters);
    hipLaunchKernelGGL(knn_brute<Finish>, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, g, k, fin, (const uint32_t*)fallback,
                       (const unsigned long long*)counters);
    hipLaunchKernelGGL(grid_status, dim3(1), dim3(1), 0, st, g.p, n, counters);
}

}  // namespace
