// What lnr_cloud.hip (the sort, the grid build, the distance query) and lnr_icp.hip (kNN normals, point-to-plane ICP) share: the
// parameters and the layout of a nearest-neighbour grid, the walk over its cells, the fixed-order sums, the affine transform of a point,
// and the host prologue of the entry points.  Both sources are compiled with -ffp-contract=off (build.py EXACT): every fp64 expression
// below rounds operation by operation, as the numpy restatements (tests/cloud_restatement.py, tests/icp_restatement.py) do.
//
// A grid (lnr_nn_grid_build) is one buffer: the CloudParams of its build, the targets gathered in key order, one (key, first target) per
// occupied cell with an end sentinel, and each sorted target's input index, which orders ties.
//   shells     a query walks Chebyshev shells of cells around its own (clamped) cell, one binary search per z-row, and after each shell
//              gets a lower bound on the squared distance of every target in a cell not yet visited.  The bound subtracts a slack of
//              1e-14 of the coordinates' magnitude, which covers the rounding of both cell assignments; the caller's stop rule compares
//              its best (or k-th best) d2 against it
// Queries still open after NN_MAX_SHELL shells stream every target through LDS in tiles of NN_FB_TILE (nn_brute, knn_brute).
// It is also the lowest header of the tools' family (lnr_radix_sort.h, lnr_mesh_args.h and lnr_traj.h include it), so the pieces every
// tool may need live here and define no kernel: align256, finite3, dot3, the block sum and the block scan, the count checks.
// Everything is internal to its translation unit (the anonymous namespace), like the kernels that use it.
#pragma once
#include "lnr_common.h"

#include <float.h>
#include <math.h>

#define CL_BLOCK 256
#define CL_SORT_TILE (CL_BLOCK * 16)
#define NN_MAX_SHELL 4
#define NN_FB_TILE 1024

enum { CL_ST_NONFINITE = 1, CL_ST_TOO_SMALL = 2, CL_ST_TOO_WIDE = 4 };

// The parameters of one call, computed on the device.  For a grid they stay at the head of the grid buffer for its queries.
struct CloudParams {
    double origin[3];
    double edge;
    double lo[3], hi[3];            // min / max of the finite points
    int64_t dims[3];                // cells per axis (largest index + 1)
    uint32_t shift[3];              // key = ix << shift[0] | iy << shift[1] | iz
    uint32_t bits;                  // sum of the per-axis bit lengths
    int32_t npasses;                // digit passes the sort runs
    uint32_t status;                // CL_ST_*
    uint32_t n;                     // points the call works on (0 after an error)
    uint32_t n_seg;                 // occupied voxels / cells
    unsigned long long nonfinite;
};

namespace {

// ------------------------------------------------------------------------------------------------ the grid
struct GridView {
    const CloudParams* p;
    const double* pts;
    const uint64_t* cell_key;
    const uint32_t* cell_start;
    const uint32_t* orig;           // input index of each sorted target
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct GridLayout { size_t params, pts, cell_key, cell_start, orig, total; };
GridLayout grid_layout(int64_t n) {
    GridLayout l;
    l.params = 0;
    l.pts = align256(sizeof(CloudParams));
    l.cell_key = align256(l.pts + 24 * (size_t)n);
    l.cell_start = align256(l.cell_key + 8 * (size_t)n);
    l.orig = align256(l.cell_start + 4 * ((size_t)n + 1));
    l.total = align256(l.orig + 4 * (size_t)n);
    return l;
}

GridView grid_view(const void* grid, int64_t n) {
    const GridLayout gl = grid_layout(n);
    const char* gb = (const char*)grid;
    return GridView{(const CloudParams*)(gb + gl.params), (const double*)(gb + gl.pts), (const uint64_t*)(gb + gl.cell_key),
                    (const uint32_t*)(gb + gl.cell_start), (const uint32_t*)(gb + gl.orig)};
}

__device__ inline bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__device__ inline double sq_dist(double qx, double qy, double qz, const double* t) {
    const double dx = qx - t[0], dy = qy - t[1], dz = qz - t[2];
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ inline double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// (d2, index) order: the lower input index wins a tie
__device__ inline bool pair_less(double ad, uint32_t ai, double bd, uint32_t bi) { return ad < bd || (ad == bd && ai < bi); }

// ------------------------------------------------------------------------------------------------ shells
// Chebyshev shells of cells around the query's (clamped) cell, and after each shell a rounding-safe lower bound on the squared distance
// of every target in a cell not yet visited.  Each cell is visited once.
struct ShellQuery {
    double q[3], slack[3];
    int64_t c[3];
};

__device__ inline ShellQuery shell_query(const CloudParams* p, double qx, double qy, double qz) {
    ShellQuery s;
    s.q[0] = qx; s.q[1] = qy; s.q[2] = qz;
    const double h = p->edge;
    for (int a = 0; a < 3; ++a) {
        double f = floor((s.q[a] - p->origin[a]) / h);
        f = fmin(fmax(f, 0.0), (double)(p->dims[a] - 1));
        s.c[a] = (int64_t)f;
        s.slack[a] = 1e-14 * ((fabs(p->origin[a]) + fabs(s.q[a])) + (double)(p->dims[a] + 1) * h);
    }
    return s;
}

// visit(j) for every sorted target j of the cells of row (x, y) with z in [z0, z1]: lower_bound on the sorted cell keys, then forward
// while the key is in the row
template <class F>
__device__ inline void shell_row(const GridView& g, uint32_t n_cells, int64_t x, int64_t y, int64_t z0, int64_t z1, F& visit) {
    const CloudParams* p = g.p;
    const uint64_t k0 = ((uint64_t)x << p->shift[0]) | ((uint64_t)y << p->shift[1]) | (uint64_t)z0;
    const uint64_t k1 = ((uint64_t)x << p->shift[0]) | ((uint64_t)y << p->shift[1]) | (uint64_t)z1;
    uint32_t lo = 0, hi = n_cells;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g.cell_key[mid] < k0) lo = mid + 1; else hi = mid;
    }
    for (uint32_t c = lo; c < n_cells && g.cell_key[c] <= k1; ++c)
        for (uint32_t j = g.cell_start[c]; j < g.cell_start[c + 1]; ++j) visit(j);
}

// the cells at Chebyshev distance r from the query's cell; returns bound^2 (1 - 1e-14) with bound the gap, per axis and side, to the
// first unvisited layer of cells less the slack (INFINITY when no cell is left): every target outside shells 0..r has d2 >= the value
// returned
template <class F>
__device__ inline double shell_visit(const GridView& g, const ShellQuery& s, int64_t r, F& visit) {
    const CloudParams* p = g.p;
    const uint32_t n_cells = p->n_seg;
    const int64_t* c = s.c;
    const int64_t x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < p->dims[0] - 1 ? c[0] + r : p->dims[0] - 1;
    const int64_t y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < p->dims[1] - 1 ? c[1] + r : p->dims[1] - 1;
    const int64_t zl = c[2] - r, zh = c[2] + r, zmax = p->dims[2] - 1;
    for (int64_t x = x0; x <= x1; ++x)
        for (int64_t y = y0; y <= y1; ++y) {
            const bool ring = x == c[0] - r || x == c[0] + r || y == c[1] - r || y == c[1] + r;
            if (ring) {
                shell_row(g, n_cells, x, y, zl > 0 ? zl : 0, zh < zmax ? zh : zmax, visit);
            } else {
                if (zl >= 0) shell_row(g, n_cells, x, y, zl, zl, visit);
                if (zh <= zmax && zh != zl) shell_row(g, n_cells, x, y, zh, zh, visit);
            }
        }
    const double h = p->edge;
    double bound = INFINITY;
    for (int a = 0; a < 3; ++a) {
        if (c[a] - r - 1 >= 0) bound = fmin(bound, fmax((s.q[a] - (p->origin[a] + (double)(c[a] - r) * h)) - s.slack[a], 0.0));
        if (c[a] + r + 1 <= p->dims[a] - 1) bound = fmin(bound, fmax(((p->origin[a] + (double)(c[a] + r + 1) * h) - s.q[a]) - s.slack[a], 0.0));
    }
    return bound == INFINITY ? INFINITY : (bound * bound) * (1.0 - 1e-14);
}

// ------------------------------------------------------------------------------------------------ sums
// the sum over the 64 lanes of a wave, in every lane (xor butterfly; for a double, v = v + other in this order)
template <class T>
__device__ inline T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

__device__ inline double block_sum(double v, double* lds) {   // lds: CL_BLOCK / 64 doubles; the fixed-order sum, valid in thread 0
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = lds[0];
#pragma unroll
    for (int w = 1; w < CL_BLOCK / 64; ++w) t = t + lds[w];
    return t;
}

// exclusive prefix of v over a 256-thread block; *total gets the block's sum.  lds: 4 words.
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < CL_BLOCK / 64; ++k) {
        const uint32_t s = lds[k];
        pre += k < w ? s : 0u;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return pre + x - v;
}

// ------------------------------------------------------------------------------------------------ the affine transform
struct Affine { double t[12]; };                              // the top three rows of a 4x4, row-major

// dst_i = T src_i with T [12]: ((T0 x + T1 y) + T2 z) + T3 per row.  dst may be src.
__device__ inline void transform_point(const double* src, const double* T, double* dst, uint32_t i) {
    const double x = src[3 * (size_t)i], y = src[3 * (size_t)i + 1], z = src[3 * (size_t)i + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) dst[3 * (size_t)i + a] = ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
}

// ------------------------------------------------------------------------------------------------ host
uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + CL_BLOCK - 1) / CL_BLOCK); }

const int64_t CL_MAX_POINTS = ((int64_t)1 << 31) - CL_SORT_TILE;

bool count_ok(int64_t n) { return n >= 0 && n <= CL_MAX_POINTS; }

// the point-count range checks of the entry points: "<fn>: <n> <noun>, the limit is <limit>"
#define CL_REQUIRE_COUNT(fn, n, noun) \
    LNR_REQUIRE(count_ok(n), fn ": %lld " noun ", the limit is %lld", (long long)(n), (long long)CL_MAX_POINTS)
#define CL_REQUIRE_COUNTS(fn, a, a_noun, b, b_noun)                                                                               \
    LNR_REQUIRE(count_ok(a) && count_ok(b), fn ": %lld " a_noun ", %lld " b_noun ", the limit is %lld each", (long long)(a), \
                (long long)(b), (long long)CL_MAX_POINTS)

// clears device words on the stream, or fails with "<fn>: clearing the <what> failed"
int clear_words(void* words, size_t bytes, hipStream_t st, const char* fn, const char* what) {
    if (hipMemsetAsync(words, 0, bytes, st) == hipSuccess) return LNR_OK;
    lnr_set_error("%s: clearing the %s failed", fn, what);
    return LNR_ERR_LAUNCH;
}

// a caller's 12 doubles as an Affine; returns the first entry that is not finite, or -1
int affine_from_host(const double* t12, Affine* T) {
    for (int k = 0; k < 12; ++k) {
        T->t[k] = t12[k];
        if (!isfinite(T->t[k])) return k;
    }
    return -1;
}

}  // namespace
