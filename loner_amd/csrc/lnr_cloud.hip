// Point clouds of a rendered map (gfx950): scan points, voxel down-sampling, the rigid transform of a merged scan, and exact
// nearest-neighbour distances between two clouds.
//
// Replaces the open3d calls of analysis/renderer_lidar.py:71-91, :296-349 and analysis/evaluate_lidar_map.py:16-98:
//   PointCloud.voxel_down_sample, PointCloud.transform, PointCloud.compute_point_cloud_distance
// with the definitions stated in include/loner_hip.h ("point clouds").  This file is compiled with -ffp-contract=off (build.py EXACT):
// every fp64 expression below rounds operation by operation, as the numpy restatement (tests/cloud_restatement.py) does; the divides
// and square roots are IEEE (no fast-math).
//
// Everything is built from one device-wide stable sort of (uint64 key, uint32 index) pairs:
//   bound      per-block min / max of the finite points and a count of the others, then one workgroup folds them into the
//              parameters of the call (origin, edge, bits per axis, digit passes, status) in device memory
//   key        per point: the packed cell index (x highest, z lowest), only as many bits as the bound needs
//   sort       LSD radix, 8-bit digits: count (per-block histograms), exclusive scan of the [digit][block] table, stable scatter
//              (rank within a 256-element chunk from eight ballots per wave).  All 8 passes are enqueued; those the key does not
//              need return at once (the pass count is on the device, the host never waits for it)
//   segments   heads (key differs from its predecessor), their exclusive scan and the start of each run
//   voxel      one thread per occupied voxel sums its points in input order (the sort is stable) and divides by the count
//   grid       the targets gathered in key order, one (key, start) per occupied cell
// The nearest-neighbour query walks Chebyshev shells of cells around the query's cell and stops when its best squared distance is
// below a rounding-safe lower bound on every unvisited cell; queries still open after NN_MAX_SHELL shells stream every target
// through LDS.
#include "lnr_common.h"

#include <float.h>
#include <math.h>

#define CL_BLOCK 256
#define CL_SCAN_PER_THREAD 8
#define CL_SCAN_TILE (CL_BLOCK * CL_SCAN_PER_THREAD)
#define CL_SORT_TILE (CL_BLOCK * 16)
#define CL_RADIX 256
#define CL_MAX_PASSES 8
#define CL_BOUND_BLOCKS 1024
#define NN_MAX_SHELL 4
#define NN_FB_TILE 1024

enum { CL_MODE_VOXEL = 0, CL_MODE_GRID = 1 };
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

__device__ inline uint32_t live_count(const int32_t* n_dev, uint32_t n_cap) {
    if (!n_dev) return n_cap;
    const int32_t v = *n_dev;
    return v < 0 ? 0u : ((uint32_t)v < n_cap ? (uint32_t)v : n_cap);
}

__device__ inline bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

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

// ------------------------------------------------------------------------------------------------ device-wide exclusive scan (uint32)
// In place over a[0, L).  guard (nullable): the kernels return at once when pass >= *guard (a radix pass the key does not need).
__global__ __launch_bounds__(CL_BLOCK) void scan_tile_sums(const uint32_t* __restrict__ a, uint32_t L, uint32_t* __restrict__ sums,
                                                           const int32_t* guard, int pass) {
    if (guard && pass >= *guard) return;
    __shared__ uint32_t lds[CL_BLOCK / 64];
    const uint64_t base = (uint64_t)blockIdx.x * CL_SCAN_TILE + (uint64_t)threadIdx.x * CL_SCAN_PER_THREAD;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < CL_SCAN_PER_THREAD; ++k) s += base + k < L ? a[base + k] : 0u;
    uint32_t tot;
    block_exclusive_scan(s, lds, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(CL_BLOCK) void scan_block_sums(uint32_t* __restrict__ sums, uint32_t n_tiles, uint32_t* total,
                                                            const int32_t* guard, int pass) {
    if (guard && pass >= *guard) return;
    __shared__ uint32_t lds[CL_BLOCK / 64];
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < n_tiles; c0 += CL_BLOCK) {
        const uint32_t b = c0 + threadIdx.x;
        const uint32_t v = b < n_tiles ? sums[b] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan(v, lds, &tot);
        if (b < n_tiles) sums[b] = carry + ex;
        carry += tot;
    }
    if (total && threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(CL_BLOCK) void scan_tile_apply(uint32_t* __restrict__ a, uint32_t L, const uint32_t* __restrict__ sums,
                                                            const int32_t* guard, int pass) {
    if (guard && pass >= *guard) return;
    __shared__ uint32_t lds[CL_BLOCK / 64];
    const uint64_t base = (uint64_t)blockIdx.x * CL_SCAN_TILE + (uint64_t)threadIdx.x * CL_SCAN_PER_THREAD;
    uint32_t v[CL_SCAN_PER_THREAD], s = 0;
#pragma unroll
    for (int k = 0; k < CL_SCAN_PER_THREAD; ++k) {
        v[k] = base + k < L ? a[base + k] : 0u;
        s += v[k];
    }
    uint32_t tot;
    uint32_t run = sums[blockIdx.x] + block_exclusive_scan(s, lds, &tot);
#pragma unroll
    for (int k = 0; k < CL_SCAN_PER_THREAD; ++k) {
        if (base + k < L) a[base + k] = run;
        run += v[k];
    }
}

uint32_t scan_tiles(uint64_t L) { return (uint32_t)((L + CL_SCAN_TILE - 1) / CL_SCAN_TILE); }

void enqueue_scan(uint32_t* a, uint32_t L, uint32_t* sums, uint32_t* total, const int32_t* guard, int pass, hipStream_t st) {
    const uint32_t nt = scan_tiles(L);
    if (nt == 0) return;
    hipLaunchKernelGGL(scan_tile_sums, dim3(nt), dim3(CL_BLOCK), 0, st, a, L, sums, guard, pass);
    hipLaunchKernelGGL(scan_block_sums, dim3(1), dim3(CL_BLOCK), 0, st, sums, nt, total, guard, pass);
    hipLaunchKernelGGL(scan_tile_apply, dim3(nt), dim3(CL_BLOCK), 0, st, a, L, sums, guard, pass);
}

// ------------------------------------------------------------------------------------------------ bound and parameters
__global__ __launch_bounds__(CL_BLOCK) void bound_partial(const double* __restrict__ pts, const int32_t* n_dev, uint32_t n_cap,
                                                          double* __restrict__ part, CloudParams* p) {
    __shared__ double red[6][CL_BLOCK / 64];
    const uint32_t n = live_count(n_dev, n_cap);
    double m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    unsigned long long bad = 0;
    for (uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x; i < n; i += gridDim.x * CL_BLOCK) {
        const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        if (!finite3(x, y, z)) { ++bad; continue; }
        m[0] = fmin(m[0], x); m[1] = fmin(m[1], y); m[2] = fmin(m[2], z);
        m[3] = fmax(m[3], x); m[4] = fmax(m[4], y); m[5] = fmax(m[5], z);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double t = __shfl_xor(m[k], o, 64);
            m[k] = k < 3 ? fmin(m[k], t) : fmax(m[k], t);
        }
        bad += __shfl_xor(bad, o, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) red[k][w] = m[k];
        if (bad) atomicAdd(&p->nonfinite, bad);
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        double r = red[k][0];
        for (int q = 1; q < CL_BLOCK / 64; ++q) r = k < 3 ? fmin(r, red[k][q]) : fmax(r, red[k][q]);
        part[6 * (size_t)blockIdx.x + k] = r;
    }
}

__device__ inline uint32_t bit_length(int64_t v) { return v <= 0 ? 0u : 64u - (uint32_t)__clzll((unsigned long long)v); }

// one workgroup: folds the partial bounds, sets the call's parameters.  Voxel mode (open3d's VoxelDownSample): origin = min - 0.5 v,
// the too-small test on max + 0.5 v.  Grid mode: origin = min, edge = the caller's or the default, doubled until the key fits 63 bits.
__global__ __launch_bounds__(CL_BLOCK) void cloud_params(const double* __restrict__ part, int n_part, const int32_t* n_dev, uint32_t n_cap,
                                                         int mode, double edge_in, CloudParams* p) {
    __shared__ double red[6][CL_BLOCK];
    double m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < n_part; b += CL_BLOCK)
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] = k < 3 ? fmin(m[k], part[6 * b + k]) : fmax(m[k], part[6 * b + k]);
#pragma unroll
    for (int k = 0; k < 6; ++k) red[k][threadIdx.x] = m[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int t = 1; t < CL_BLOCK; ++t)
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] = k < 3 ? fmin(m[k], red[k][t]) : fmax(m[k], red[k][t]);
    const uint32_t n = live_count(n_dev, n_cap);
    uint32_t status = p->nonfinite ? (uint32_t)CL_ST_NONFINITE : 0u;
    for (int a = 0; a < 3; ++a) { p->lo[a] = m[a]; p->hi[a] = m[3 + a]; p->dims[a] = 0; p->shift[a] = 0; }
    p->bits = 0;
    p->npasses = 0;
    p->n_seg = 0;
    p->edge = edge_in;
    if (n == 0 || status) {
        p->status = status;
        p->n = 0;
        return;
    }
    double edge = edge_in;
    if (mode == CL_MODE_VOXEL) {
        const double half = edge * 0.5;
        double ext = 0.0;
        for (int a = 0; a < 3; ++a) {
            p->origin[a] = m[a] - half;
            ext = fmax(ext, (m[3 + a] + half) - p->origin[a]);
        }
        if (edge * (double)2147483647 < ext) status |= CL_ST_TOO_SMALL;
    } else {
        for (int a = 0; a < 3; ++a) p->origin[a] = m[a];
        if (!(edge > 0.0)) {            // the default edge: cbrt of the bounding box's volume per point, every extent raised to at least
            double e[3], emax = 0.0;    // 2^-10 of the largest (a flat or linear cloud), 1 when all points coincide
            for (int a = 0; a < 3; ++a) { e[a] = m[3 + a] - m[a]; emax = fmax(emax, e[a]); }
            if (emax > 0.0) {
                for (int a = 0; a < 3; ++a) e[a] = fmax(e[a], emax * 0x1p-10);
                edge = cbrt(((e[0] * e[1]) * e[2]) / (double)n);
            } else {
                edge = 1.0;
            }
        }
    }
    if (!status) {
        for (;;) {
            uint32_t bits = 0;
            bool fits = true;
            for (int a = 0; a < 3; ++a) {
                const double f = floor((m[3 + a] - p->origin[a]) / edge);
                if (!(f < 0x1p62)) { fits = false; break; }
                p->dims[a] = (int64_t)f + 1;
                bits += bit_length((int64_t)f);
            }
            if (fits && bits <= (mode == CL_MODE_VOXEL ? 64u : 63u)) {
                p->bits = bits;
                break;
            }
            if (mode == CL_MODE_VOXEL) { status |= CL_ST_TOO_WIDE; p->bits = fits ? bits : 0u; break; }
            edge *= 2.0;
        }
    }
    p->edge = edge;
    p->status = status;
    if (status) {
        p->n = 0;
        return;
    }
    const uint32_t bz = bit_length(p->dims[2] - 1), by = bit_length(p->dims[1] - 1);
    p->shift[2] = 0;
    p->shift[1] = bz;
    p->shift[0] = bz + by;
    p->npasses = (int32_t)((p->bits + 7) / 8);
    p->n = n;
}

__global__ __launch_bounds__(CL_BLOCK) void cloud_keys(const double* __restrict__ pts, const CloudParams* __restrict__ p,
                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= p->n) return;
    const double e = p->edge;
    uint64_t key = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c = floor((pts[3 * (size_t)i + a] - p->origin[a]) / e);
        key |= (uint64_t)(int64_t)c << p->shift[a];
    }
    keys[i] = key;
    idx[i] = i;
}

// ------------------------------------------------------------------------------------------------ stable LSD radix sort
__global__ __launch_bounds__(CL_BLOCK) void radix_count(const uint64_t* __restrict__ keys, const CloudParams* __restrict__ p, int pass,
                                                        uint32_t* __restrict__ counts, uint32_t n_blocks) {
    if (pass >= p->npasses) return;
    __shared__ uint32_t h[CL_RADIX];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n = p->n, shift = 8 * pass;
    const uint64_t base = (uint64_t)blockIdx.x * CL_SORT_TILE;
    for (int k = 0; k < CL_SORT_TILE / CL_BLOCK; ++k) {
        const uint64_t i = base + (uint64_t)k * CL_BLOCK + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & (CL_RADIX - 1)], 1u);
    }
    __syncthreads();
    counts[(size_t)threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(CL_BLOCK) void radix_scatter(const uint64_t* __restrict__ keys_in, const uint32_t* __restrict__ idx_in,
                                                          uint64_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out,
                                                          const CloudParams* __restrict__ p, int pass,
                                                          const uint32_t* __restrict__ offsets, uint32_t n_blocks) {
    if (pass >= p->npasses) return;
    __shared__ uint32_t run[CL_RADIX];
    __shared__ uint32_t wc[CL_BLOCK / 64][CL_RADIX];
    const uint32_t n = p->n, shift = 8 * pass;
    const uint64_t base = (uint64_t)blockIdx.x * CL_SORT_TILE;
    if (base >= n) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    run[threadIdx.x] = offsets[(size_t)threadIdx.x * n_blocks + blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < CL_SORT_TILE / CL_BLOCK; ++k) {
#pragma unroll
        for (int q = 0; q < CL_BLOCK / 64; ++q) wc[q][threadIdx.x] = 0;
        __syncthreads();
        const uint64_t i = base + (uint64_t)k * CL_BLOCK + threadIdx.x;
        const bool valid = i < n;
        const uint64_t key = valid ? keys_in[i] : 0ull;
        const uint32_t id = valid ? idx_in[i] : 0u;
        const uint32_t d = (uint32_t)(key >> shift) & (CL_RADIX - 1);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool on = (d >> b) & 1u;
            const unsigned long long v = __ballot(on);
            same &= on ? v : ~v;
        }
        const uint32_t rank = (uint32_t)__popcll(same & below);
        if (valid && rank == 0) wc[w][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + rank;
            for (int q = 0; q < w; ++q) pos += wc[q][d];
            keys_out[pos] = key;
            idx_out[pos] = id;
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int q = 0; q < CL_BLOCK / 64; ++q) add += wc[q][threadIdx.x];
        run[threadIdx.x] += add;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ segments
__device__ inline const uint64_t* sorted_keys(const CloudParams* p, const uint64_t* a, const uint64_t* b) { return (p->npasses & 1) ? b : a; }
__device__ inline const uint32_t* sorted_idx(const CloudParams* p, const uint32_t* a, const uint32_t* b) { return (p->npasses & 1) ? b : a; }

__global__ __launch_bounds__(CL_BLOCK) void segment_heads(const uint64_t* __restrict__ ka, const uint64_t* __restrict__ kb,
                                                          const CloudParams* __restrict__ p, uint32_t n_cap, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n_cap) return;
    const uint64_t* k = sorted_keys(p, ka, kb);
    flags[i] = (i < p->n && (i == 0 || k[i] != k[i - 1])) ? 1u : 0u;
}

__global__ __launch_bounds__(CL_BLOCK) void segment_starts(const uint64_t* __restrict__ ka, const uint64_t* __restrict__ kb,
                                                           const CloudParams* __restrict__ p, const uint32_t* __restrict__ seg,
                                                           uint32_t* __restrict__ starts) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= p->n) return;
    const uint64_t* k = sorted_keys(p, ka, kb);
    if (i == 0 || k[i] != k[i - 1]) starts[seg[i]] = i;
}

// one thread per occupied voxel: the fp64 sum of its points in input order, divided by the count (open3d AccumulatedPoint)
__global__ __launch_bounds__(CL_BLOCK) void voxel_average(const double* __restrict__ pts, const uint32_t* __restrict__ ia,
                                                          const uint32_t* __restrict__ ib, const CloudParams* __restrict__ p,
                                                          const uint32_t* __restrict__ starts, double* __restrict__ out) {
    const uint32_t s = blockIdx.x * CL_BLOCK + threadIdx.x;
    const uint32_t n_seg = p->n_seg;
    if (s >= n_seg) return;
    const uint32_t* idx = sorted_idx(p, ia, ib);
    const uint32_t j0 = starts[s], j1 = s + 1 < n_seg ? starts[s + 1] : p->n;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t j = j0; j < j1; ++j) {
        const size_t q = 3 * (size_t)idx[j];
        sx = sx + pts[q];
        sy = sy + pts[q + 1];
        sz = sz + pts[q + 2];
    }
    const double c = (double)(j1 - j0);
    out[3 * (size_t)s] = sx / c;
    out[3 * (size_t)s + 1] = sy / c;
    out[3 * (size_t)s + 2] = sz / c;
}

// the grid: targets in key order with their input index (ascending within a cell: the sort is stable), one (key, first target) per
// occupied cell, and the end sentinel
__global__ __launch_bounds__(CL_BLOCK) void grid_fill(const double* __restrict__ pts, const uint64_t* __restrict__ ka,
                                                      const uint64_t* __restrict__ kb, const uint32_t* __restrict__ ia,
                                                      const uint32_t* __restrict__ ib, const CloudParams* __restrict__ p,
                                                      const uint32_t* __restrict__ starts, double* __restrict__ sorted,
                                                      uint64_t* __restrict__ cell_key, uint32_t* __restrict__ cell_start,
                                                      uint32_t* __restrict__ orig) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    const uint32_t n = p->n, n_seg = p->n_seg;
    if (i < n) {
        const uint32_t o = sorted_idx(p, ia, ib)[i];
        const size_t q = 3 * (size_t)o;
        orig[i] = o;
        sorted[3 * (size_t)i] = pts[q];
        sorted[3 * (size_t)i + 1] = pts[q + 1];
        sorted[3 * (size_t)i + 2] = pts[q + 2];
    }
    if (i < n_seg) {
        cell_start[i] = starts[i];
        cell_key[i] = sorted_keys(p, ka, kb)[starts[i]];
    }
    if (i == 0) cell_start[n_seg] = n;
}

// a grid unusable for its own points (a non-finite target, or another count than the call's): counters[1] = 1
__global__ void grid_status(const CloudParams* __restrict__ p, uint32_t n, unsigned long long* __restrict__ counters) {
    if (p->status || p->n != n) counters[1] = 1ull;
}

__global__ void cloud_info(const CloudParams* __restrict__ p, int64_t* __restrict__ info) {
    info[0] = p->status;
    info[1] = p->n_seg;
    info[2] = (int64_t)p->nonfinite;
    info[3] = p->bits;
    info[4] = (int64_t)__double_as_longlong(p->edge);
    for (int a = 0; a < 3; ++a) info[5 + a] = p->dims[a];
}

// ------------------------------------------------------------------------------------------------ scan points and transform
__device__ inline bool scan_keep(float depth, float var, float scale, float var_max, float depth_max, float* depth_m) {
    const float d = depth * scale, v = var * scale;
    *depth_m = d;
    return v < var_max && d < depth_max;
}

__global__ __launch_bounds__(CL_BLOCK) void scan_flags(const float* __restrict__ depth, const float* __restrict__ var, uint32_t m,
                                                       float scale, float var_max, float depth_max, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= m) return;
    float d;
    flags[i] = scan_keep(depth[i], var[i], scale, var_max, depth_max, &d) ? 1u : 0u;
}

__global__ __launch_bounds__(CL_BLOCK) void scan_emit(const float* __restrict__ depth, const float* __restrict__ var,
                                                      const int64_t* __restrict__ ray_index, const float* __restrict__ dirs, int64_t n_dirs,
                                                      uint32_t m, float scale, float var_max, float depth_max,
                                                      const uint32_t* __restrict__ pos, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= m) return;
    float d;
    if (!scan_keep(depth[i], var[i], scale, var_max, depth_max, &d)) return;
    const int64_t r = ray_index[i];
    if (r < 0 || r >= n_dirs) return;
    const size_t o = 3 * (size_t)pos[i];
#pragma unroll
    for (int a = 0; a < 3; ++a) out[o + a] = (double)(dirs[a * n_dirs + r] * d);
}

struct Affine { double t[12]; };

__global__ __launch_bounds__(CL_BLOCK) void append_transformed(const double* src, uint32_t n, Affine T, double* dst) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double x = src[3 * (size_t)i], y = src[3 * (size_t)i + 1], z = src[3 * (size_t)i + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) dst[3 * (size_t)i + a] = ((T.t[4 * a] * x + T.t[4 * a + 1] * y) + T.t[4 * a + 2] * z) + T.t[4 * a + 3];
}

// ------------------------------------------------------------------------------------------------ nearest-neighbour distance
struct GridView {
    const CloudParams* p;
    const double* pts;
    const uint64_t* cell_key;
    const uint32_t* cell_start;
    const uint32_t* orig;           // input index of each sorted target
};

__device__ inline double sq_dist(double qx, double qy, double qz, const double* t) {
    const double dx = qx - t[0], dy = qy - t[1], dz = qz - t[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// the cells of row (x, y) with z in [z0, z1]: lower_bound on the sorted cell keys, then forward while the key is in the row
__device__ inline void visit_row(const GridView& g, uint32_t n_cells, int64_t x, int64_t y, int64_t z0, int64_t z1, double qx, double qy,
                                 double qz, double& best) {
    const CloudParams* p = g.p;
    const uint64_t k0 = ((uint64_t)x << p->shift[0]) | ((uint64_t)y << p->shift[1]) | (uint64_t)z0;
    const uint64_t k1 = ((uint64_t)x << p->shift[0]) | ((uint64_t)y << p->shift[1]) | (uint64_t)z1;
    uint32_t lo = 0, hi = n_cells;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g.cell_key[mid] < k0) lo = mid + 1; else hi = mid;
    }
    for (uint32_t c = lo; c < n_cells && g.cell_key[c] <= k1; ++c)
        for (uint32_t j = g.cell_start[c]; j < g.cell_start[c + 1]; ++j) best = fmin(best, sq_dist(qx, qy, qz, g.pts + 3 * (size_t)j));
}

__global__ __launch_bounds__(CL_BLOCK) void nn_shells(GridView g, const double* __restrict__ q, uint32_t n_q, double* __restrict__ dist,
                                                      double* __restrict__ d2_out, uint32_t* __restrict__ fallback,
                                                      unsigned long long* __restrict__ counters) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    unsigned long long shells = 0;
    if (i < n_q) {
        const CloudParams* p = g.p;
        const double qv[3] = {q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2]};
        if (!finite3(qv[0], qv[1], qv[2])) {
            atomicAdd(&counters[1], 1ull);
            dist[i] = NAN;
            if (d2_out) d2_out[i] = NAN;
        } else if (p->n == 0) {                         // no target: open3d's SearchKNN finds nothing and the distance stays 0
            dist[i] = 0.0;
            if (d2_out) d2_out[i] = 0.0;
        } else {
            const double h = p->edge;
            int64_t c[3];
            double slack[3];
            for (int a = 0; a < 3; ++a) {
                double f = floor((qv[a] - p->origin[a]) / h);
                f = fmin(fmax(f, 0.0), (double)(p->dims[a] - 1));
                c[a] = (int64_t)f;
                slack[a] = 1e-14 * ((fabs(p->origin[a]) + fabs(qv[a])) + (double)(p->dims[a] + 1) * h);
            }
            const uint32_t n_cells = p->n_seg;
            double best = INFINITY;
            bool done = false;
            for (int r = 0; r <= NN_MAX_SHELL && !done; ++r) {
                ++shells;
                const int64_t x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < p->dims[0] - 1 ? c[0] + r : p->dims[0] - 1;
                const int64_t y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < p->dims[1] - 1 ? c[1] + r : p->dims[1] - 1;
                const int64_t zl = c[2] - r, zh = c[2] + r, zmax = p->dims[2] - 1;
                for (int64_t x = x0; x <= x1; ++x)
                    for (int64_t y = y0; y <= y1; ++y) {
                        const bool ring = x == c[0] - r || x == c[0] + r || y == c[1] - r || y == c[1] + r;
                        if (ring) {
                            visit_row(g, n_cells, x, y, zl > 0 ? zl : 0, zh < zmax ? zh : zmax, qv[0], qv[1], qv[2], best);
                        } else {
                            if (zl >= 0) visit_row(g, n_cells, x, y, zl, zl, qv[0], qv[1], qv[2], best);
                            if (zh <= zmax && zh != zl) visit_row(g, n_cells, x, y, zh, zh, qv[0], qv[1], qv[2], best);
                        }
                    }
                // a lower bound on the distance to any target in a cell outside the shells visited: per axis and side, the gap to the
                // first unvisited layer of cells, less a slack that covers the rounding of both cell assignments
                double bound = INFINITY;
                for (int a = 0; a < 3; ++a) {
                    if (c[a] - r - 1 >= 0)
                        bound = fmin(bound, fmax((qv[a] - (p->origin[a] + (double)(c[a] - r) * h)) - slack[a], 0.0));
                    if (c[a] + r + 1 <= p->dims[a] - 1)
                        bound = fmin(bound, fmax(((p->origin[a] + (double)(c[a] + r + 1) * h) - qv[a]) - slack[a], 0.0));
                }
                done = bound == INFINITY || best <= (bound * bound) * (1.0 - 1e-14);
            }
            if (done) {
                dist[i] = sqrt(best);
                if (d2_out) d2_out[i] = best;
            } else {
                fallback[atomicAdd(&counters[0], 1ull)] = i;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) shells += __shfl_xor(shells, o, 64);
    if ((threadIdx.x & 63) == 0 && shells) atomicAdd(&counters[2], shells);
}

// the exact fallback: one query per thread, every target streamed through LDS in tiles
__global__ __launch_bounds__(CL_BLOCK) void nn_brute(GridView g, const double* __restrict__ q, const uint32_t* __restrict__ fallback,
                                                     const unsigned long long* __restrict__ counters, double* __restrict__ dist,
                                                     double* __restrict__ d2_out) {
    __shared__ double tile[NN_FB_TILE * 3];
    const uint32_t n_fb = (uint32_t)counters[0];
    if ((uint64_t)blockIdx.x * CL_BLOCK >= n_fb) return;
    const uint32_t k = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool active = k < n_fb;
    const uint32_t i = active ? fallback[k] : 0u;
    const double qx = active ? q[3 * (size_t)i] : 0.0, qy = active ? q[3 * (size_t)i + 1] : 0.0, qz = active ? q[3 * (size_t)i + 2] : 0.0;
    const uint32_t n = g.p->n;
    double best = INFINITY;
    for (uint32_t t0 = 0; t0 < n; t0 += NN_FB_TILE) {
        const uint32_t m = n - t0 < NN_FB_TILE ? n - t0 : NN_FB_TILE;
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < 3 * m; e += CL_BLOCK) tile[e] = g.pts[3 * (size_t)t0 + e];
        __syncthreads();
        for (uint32_t j = 0; j < m; ++j) best = fmin(best, sq_dist(qx, qy, qz, tile + 3 * j));
    }
    if (active) {
        dist[i] = sqrt(best);
        if (d2_out) d2_out[i] = best;
    }
}

// ------------------------------------------------------------------------------------------------ shells, shared by kNN and ICP
// The same walk as nn_shells: Chebyshev shells of cells around the query's (clamped) cell, and after each shell a rounding-safe lower
// bound on the squared distance of every target in a cell not yet visited.  Each cell is visited once.
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

// visit(j) for every sorted target j of the cells of row (x, y) with z in [z0, z1]
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

// the cells at Chebyshev distance r from the query's cell; returns bound^2 (1 - 1e-14) with bound the gap to the first unvisited layer
// less the slack (INFINITY when no cell is left): every target outside shells 0..r has d2 >= the value returned
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

// (d2, index) order: the lower input index wins a tie
__device__ inline bool pair_less(double ad, uint32_t ai, double bd, uint32_t bi) { return ad < bd || (ad == bd && ai < bi); }

// ------------------------------------------------------------------------------------------------ k nearest neighbours and normals
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

__device__ inline void cross3(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ inline double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

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

// covariance of the first min(k, found) entries from cumulants summed in list order, its normal, both written at the query's input index
__device__ inline void knn_finish(const GridView& g, const KnnList& L, int k, uint32_t out, double* __restrict__ normals,
                                  double* __restrict__ cov_out) {
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

// one query per thread: sorted target i (consecutive threads take neighbouring points), output at its input index
__global__ __launch_bounds__(CL_BLOCK) void knn_normals(GridView g, int k, double* __restrict__ normals, double* __restrict__ cov_out,
                                                        uint32_t* __restrict__ fallback, unsigned long long* __restrict__ counters) {
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
        if (done) knn_finish(g, L, k, g.orig[i], normals, cov_out);
        else fallback[atomicAdd(&counters[0], 1ull)] = i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) shells += __shfl_xor(shells, o, 64);
    if ((threadIdx.x & 63) == 0 && shells) atomicAdd(&counters[2], shells);
}

// the exact fallback: every target streamed through LDS, in sorted order with its input index
__global__ __launch_bounds__(CL_BLOCK) void knn_brute(GridView g, int k, const uint32_t* __restrict__ fallback,
                                                      const unsigned long long* __restrict__ counters, double* __restrict__ normals,
                                                      double* __restrict__ cov_out) {
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
    if (active) knn_finish(g, L, k, g.orig[i], normals, cov_out);
}

// ------------------------------------------------------------------------------------------------ point-to-plane ICP
// Terms of one correspondence's contribution, in this order: JTJ upper triangle row by row (21), JTr (6), d2, count.
#define ICP_TERMS 29
#define ICP_PART_STRIDE 32
#define ICP_MAX_BLOCKS 2048
enum { ICP_ST_NONFINITE_SOURCE = 1, ICP_ST_NONFINITE_TARGET = 2, ICP_ST_NONFINITE_NORMAL = 4, ICP_ST_NONFINITE_UPDATE = 8 };

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

__device__ inline double block_sum(double v, double* lds) {   // lds: CL_BLOCK / 64 doubles; the fixed-order sum, valid in thread 0
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = lds[0];
#pragma unroll
    for (int w = 1; w < CL_BLOCK / 64; ++w) t = t + lds[w];
    return t;
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
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad += __shfl_xor(bad, o, 64);
        bad_n += __shfl_xor(bad_n, o, 64);
    }
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

// the device-matrix form of append_transformed: T [12] (top three rows, row-major) in device memory; skipped when *active is 0
__global__ __launch_bounds__(CL_BLOCK) void append_transformed_dev(const double* src, uint32_t n, const double* __restrict__ T,
                                                                   const uint32_t* active, double* dst) {
    if (active && !*active) return;
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double x = src[3 * (size_t)i], y = src[3 * (size_t)i + 1], z = src[3 * (size_t)i + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) dst[3 * (size_t)i + a] = ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
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
    info[7] = 0;
}

// ------------------------------------------------------------------------------------------------ host
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct CloudLayout {
    uint32_t n_cap, sort_blocks, scan_len;
    size_t params, part, ka, kb, ia, ib, counts, flags, starts, sums, total;
};
CloudLayout cloud_layout(int64_t n) {
    CloudLayout l;
    l.n_cap = (uint32_t)n;
    l.sort_blocks = (uint32_t)((n + CL_SORT_TILE - 1) / CL_SORT_TILE);
    const uint64_t count_len = (uint64_t)CL_RADIX * l.sort_blocks;
    l.scan_len = (uint32_t)(count_len > (uint64_t)n ? count_len : (uint64_t)n);
    l.params = 0;
    l.part = align256(sizeof(CloudParams));
    l.ka = align256(l.part + 6 * sizeof(double) * CL_BOUND_BLOCKS);
    l.kb = align256(l.ka + 8 * (size_t)n);
    l.ia = align256(l.kb + 8 * (size_t)n);
    l.ib = align256(l.ia + 4 * (size_t)n);
    l.counts = align256(l.ib + 4 * (size_t)n);
    l.flags = align256(l.counts + 4 * count_len);
    l.starts = align256(l.flags + 4 * (size_t)n);
    l.sums = align256(l.starts + 4 * ((size_t)n + 1));
    l.total = align256(l.sums + 4 * ((size_t)scan_tiles(l.scan_len) + 1));
    return l;
}

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

uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + CL_BLOCK - 1) / CL_BLOCK); }

const int64_t CL_MAX_POINTS = ((int64_t)1 << 31) - CL_SORT_TILE;

// bound -> parameters -> keys -> sort -> segment starts, on `ws`; params at `p`
int sort_cloud(const char* what, const double* pts, int64_t n, const int32_t* n_dev, int mode, double edge, char* ws, const CloudLayout& l,
               CloudParams* p, hipStream_t st) {
    if (hipMemsetAsync(p, 0, sizeof(CloudParams), st) != hipSuccess) {
        lnr_set_error("%s: clearing the parameters failed", what);
        return LNR_ERR_LAUNCH;
    }
    if (n == 0) {
        hipLaunchKernelGGL(cloud_params, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)(ws + l.part), 0, n_dev, 0u, mode, edge, p);
        LNR_CHECK_LAUNCH(what);
        return LNR_OK;
    }
    const uint32_t n_cap = l.n_cap;
    const int nbr = (int)(blocks_for(n) < CL_BOUND_BLOCKS ? blocks_for(n) : CL_BOUND_BLOCKS);
    uint64_t *ka = (uint64_t*)(ws + l.ka), *kb = (uint64_t*)(ws + l.kb);
    uint32_t *ia = (uint32_t*)(ws + l.ia), *ib = (uint32_t*)(ws + l.ib);
    uint32_t* counts = (uint32_t*)(ws + l.counts);
    uint32_t* sums = (uint32_t*)(ws + l.sums);
    hipLaunchKernelGGL(bound_partial, dim3(nbr), dim3(CL_BLOCK), 0, st, pts, n_dev, n_cap, (double*)(ws + l.part), p);
    hipLaunchKernelGGL(cloud_params, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)(ws + l.part), nbr, n_dev, n_cap, mode, edge, p);
    hipLaunchKernelGGL(cloud_keys, dim3(blocks_for(n_cap)), dim3(CL_BLOCK), 0, st, pts, p, ka, ia);
    LNR_CHECK_LAUNCH(what);
    const int32_t* guard = &p->npasses;
    for (int pass = 0; pass < CL_MAX_PASSES; ++pass) {
        const uint64_t* kin = (pass & 1) ? kb : ka;
        uint64_t* kout = (pass & 1) ? ka : kb;
        const uint32_t* iin = (pass & 1) ? ib : ia;
        uint32_t* iout = (pass & 1) ? ia : ib;
        hipLaunchKernelGGL(radix_count, dim3(l.sort_blocks), dim3(CL_BLOCK), 0, st, kin, p, pass, counts, l.sort_blocks);
        enqueue_scan(counts, CL_RADIX * l.sort_blocks, sums, nullptr, guard, pass, st);
        hipLaunchKernelGGL(radix_scatter, dim3(l.sort_blocks), dim3(CL_BLOCK), 0, st, kin, iin, kout, iout, p, pass, counts, l.sort_blocks);
        LNR_CHECK_LAUNCH(what);
    }
    uint32_t* flags = (uint32_t*)(ws + l.flags);
    hipLaunchKernelGGL(segment_heads, dim3(blocks_for(n_cap)), dim3(CL_BLOCK), 0, st, ka, kb, p, n_cap, flags);
    enqueue_scan(flags, n_cap, sums, &p->n_seg, nullptr, 0, st);
    hipLaunchKernelGGL(segment_starts, dim3(blocks_for(n_cap)), dim3(CL_BLOCK), 0, st, ka, kb, p, flags, (uint32_t*)(ws + l.starts));
    LNR_CHECK_LAUNCH(what);
    return LNR_OK;
}

}  // namespace

extern "C" size_t lnr_cloud_workspace(int64_t n_points) {
    if (n_points < 0 || n_points > CL_MAX_POINTS) return 0;
    return cloud_layout(n_points).total;
}

extern "C" size_t lnr_nn_grid_bytes(int64_t n_targets) {
    if (n_targets < 0 || n_targets > CL_MAX_POINTS) return 0;
    return grid_layout(n_targets).total;
}

extern "C" int lnr_lidar_scan_points(const float* depth, const float* variance, const int64_t* ray_index, int64_t n_rays,
                                     const float* directions, int64_t n_directions, float scale, float var_max, float depth_max,
                                     void* workspace, size_t workspace_bytes, double* points, int32_t* n_points_dev, void* stream) {
    LNR_REQUIRE(n_rays >= 0 && n_rays <= CL_MAX_POINTS, "lnr_lidar_scan_points: %lld rays, the limit is %lld", (long long)n_rays,
                (long long)CL_MAX_POINTS);
    LNR_REQUIRE(n_directions >= 0 && n_directions < ((int64_t)1 << 40), "lnr_lidar_scan_points: bad direction count");
    LNR_REQUIRE(n_points_dev && (n_rays == 0 || (depth && variance && ray_index && directions && points && workspace)),
                "lnr_lidar_scan_points: null argument");
    const CloudLayout l = cloud_layout(n_rays);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_lidar_scan_points: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(n_points_dev, 0, sizeof(int32_t), st) != hipSuccess) {
        lnr_set_error("lnr_lidar_scan_points: clearing the count failed");
        return LNR_ERR_LAUNCH;
    }
    if (n_rays == 0) return LNR_OK;
    LnrProfScope prof("lidar_scan_points", st);
    char* ws = (char*)workspace;
    uint32_t* flags = (uint32_t*)(ws + l.flags);
    const uint32_t m = (uint32_t)n_rays;
    hipLaunchKernelGGL(scan_flags, dim3(blocks_for(m)), dim3(CL_BLOCK), 0, st, depth, variance, m, scale, var_max, depth_max, flags);
    enqueue_scan(flags, m, (uint32_t*)(ws + l.sums), (uint32_t*)n_points_dev, nullptr, 0, st);
    hipLaunchKernelGGL(scan_emit, dim3(blocks_for(m)), dim3(CL_BLOCK), 0, st, depth, variance, ray_index, directions, n_directions, m, scale,
                       var_max, depth_max, flags, points);
    LNR_CHECK_LAUNCH("lnr_lidar_scan_points");
    return LNR_OK;
}

extern "C" int lnr_voxel_down_sample(const double* points, int64_t n_points, const int32_t* n_points_dev, double voxel_size,
                                     void* workspace, size_t workspace_bytes, double* out, int64_t* info_dev, void* stream) {
    LNR_REQUIRE(n_points >= 0 && n_points <= CL_MAX_POINTS, "lnr_voxel_down_sample: %lld points, the limit is %lld",
                (long long)n_points, (long long)CL_MAX_POINTS);
    LNR_REQUIRE(isfinite(voxel_size) && voxel_size > 0.0, "lnr_voxel_down_sample: voxel_size must be finite and > 0, got %g", voxel_size);
    LNR_REQUIRE(info_dev && workspace && (n_points == 0 || (points && out)), "lnr_voxel_down_sample: null argument");
    const CloudLayout l = cloud_layout(n_points);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_voxel_down_sample: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("voxel_down_sample", st);
    char* ws = (char*)workspace;
    CloudParams* p = (CloudParams*)(ws + l.params);
    if (int rc = sort_cloud("lnr_voxel_down_sample", points, n_points, n_points_dev, CL_MODE_VOXEL, voxel_size, ws, l, p, st)) return rc;
    if (n_points > 0) {
        hipLaunchKernelGGL(voxel_average, dim3(blocks_for(n_points)), dim3(CL_BLOCK), 0, st, points, (const uint32_t*)(ws + l.ia),
                           (const uint32_t*)(ws + l.ib), p, (const uint32_t*)(ws + l.starts), out);
    }
    hipLaunchKernelGGL(cloud_info, dim3(1), dim3(1), 0, st, p, info_dev);
    LNR_CHECK_LAUNCH("lnr_voxel_down_sample");
    return LNR_OK;
}

extern "C" int lnr_cloud_append_transformed(const double* src, int64_t n_points, const double* transform, double* dst, void* stream) {
    LNR_REQUIRE(n_points >= 0 && n_points <= CL_MAX_POINTS, "lnr_cloud_append_transformed: %lld points, the limit is %lld",
                (long long)n_points, (long long)CL_MAX_POINTS);
    LNR_REQUIRE(transform && (n_points == 0 || (src && dst)), "lnr_cloud_append_transformed: null argument");
    Affine T;
    for (int k = 0; k < 12; ++k) {
        T.t[k] = transform[k];
        LNR_REQUIRE(isfinite(T.t[k]), "lnr_cloud_append_transformed: non-finite transform entry %d", k);
    }
    if (n_points == 0) return LNR_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(append_transformed, dim3(blocks_for(n_points)), dim3(CL_BLOCK), 0, st, src, (uint32_t)n_points, T, dst);
    LNR_CHECK_LAUNCH("lnr_cloud_append_transformed");
    return LNR_OK;
}

extern "C" int lnr_nn_grid_build(const double* targets, int64_t n_targets, double cell_edge, void* workspace, size_t workspace_bytes,
                                 void* grid, size_t grid_bytes, int64_t* info_dev, void* stream) {
    LNR_REQUIRE(n_targets >= 0 && n_targets <= CL_MAX_POINTS, "lnr_nn_grid_build: %lld targets, the limit is %lld", (long long)n_targets,
                (long long)CL_MAX_POINTS);
    LNR_REQUIRE(!(cell_edge > 0.0) || isfinite(cell_edge), "lnr_nn_grid_build: cell_edge must be finite (or <= 0 for the default)");
    LNR_REQUIRE(info_dev && workspace && grid && (n_targets == 0 || targets), "lnr_nn_grid_build: null argument");
    const CloudLayout l = cloud_layout(n_targets);
    const GridLayout g = grid_layout(n_targets);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_nn_grid_build: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    LNR_REQUIRE(grid_bytes >= g.total, "lnr_nn_grid_build: grid of %zu bytes, %zu needed", grid_bytes, g.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("nn_grid_build", st);
    char* ws = (char*)workspace;
    char* gb = (char*)grid;
    CloudParams* p = (CloudParams*)(gb + g.params);
    if (int rc = sort_cloud("lnr_nn_grid_build", targets, n_targets, nullptr, CL_MODE_GRID, cell_edge > 0.0 ? cell_edge : 0.0, ws, l, p, st))
        return rc;
    hipLaunchKernelGGL(grid_fill, dim3(blocks_for(n_targets + 1)), dim3(CL_BLOCK), 0, st, targets, (const uint64_t*)(ws + l.ka),
                       (const uint64_t*)(ws + l.kb), (const uint32_t*)(ws + l.ia), (const uint32_t*)(ws + l.ib), p,
                       (const uint32_t*)(ws + l.starts), (double*)(gb + g.pts), (uint64_t*)(gb + g.cell_key), (uint32_t*)(gb + g.cell_start),
                       (uint32_t*)(gb + g.orig));
    hipLaunchKernelGGL(cloud_info, dim3(1), dim3(1), 0, st, p, info_dev);
    LNR_CHECK_LAUNCH("lnr_nn_grid_build");
    return LNR_OK;
}

extern "C" int lnr_nn_distance(const void* grid, int64_t n_targets, const double* queries, int64_t n_queries, double* distance,
                               double* sq_distance, void* workspace, size_t workspace_bytes, int64_t* counters_dev, void* stream) {
    LNR_REQUIRE(n_targets >= 0 && n_targets <= CL_MAX_POINTS && n_queries >= 0 && n_queries <= CL_MAX_POINTS,
                "lnr_nn_distance: %lld targets, %lld queries, the limit is %lld each", (long long)n_targets, (long long)n_queries,
                (long long)CL_MAX_POINTS);
    LNR_REQUIRE(grid && counters_dev && workspace && (n_queries == 0 || (queries && distance)), "lnr_nn_distance: null argument");
    const size_t need = lnr_cloud_workspace(n_queries);
    LNR_REQUIRE(workspace_bytes >= need, "lnr_nn_distance: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counters_dev, 0, 4 * sizeof(int64_t), st) != hipSuccess) {
        lnr_set_error("lnr_nn_distance: clearing the counters failed");
        return LNR_ERR_LAUNCH;
    }
    if (n_queries == 0) return LNR_OK;
    LnrProfScope prof("nn_distance", st);
    const GridView g = grid_view(grid, n_targets);
    uint32_t* fb = (uint32_t*)workspace;
    unsigned long long* cnt = (unsigned long long*)counters_dev;
    const uint32_t nq = (uint32_t)n_queries;
    hipLaunchKernelGGL(nn_shells, dim3(blocks_for(nq)), dim3(CL_BLOCK), 0, st, g, queries, nq, distance, sq_distance, fb, cnt);
    hipLaunchKernelGGL(nn_brute, dim3(blocks_for(nq)), dim3(CL_BLOCK), 0, st, g, queries, (const uint32_t*)fb, (const unsigned long long*)cnt,
                       distance, sq_distance);
    LNR_CHECK_LAUNCH("lnr_nn_distance");
    return LNR_OK;
}

extern "C" int lnr_cloud_append_transformed_dev(const double* src, int64_t n_points, const double* transform_dev, double* dst, void* stream) {
    LNR_REQUIRE(n_points >= 0 && n_points <= CL_MAX_POINTS, "lnr_cloud_append_transformed_dev: %lld points, the limit is %lld",
                (long long)n_points, (long long)CL_MAX_POINTS);
    LNR_REQUIRE(transform_dev && (n_points == 0 || (src && dst)), "lnr_cloud_append_transformed_dev: null argument");
    if (n_points == 0) return LNR_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(append_transformed_dev, dim3(blocks_for(n_points)), dim3(CL_BLOCK), 0, st, src, (uint32_t)n_points, transform_dev,
                       (const uint32_t*)nullptr, dst);
    LNR_CHECK_LAUNCH("lnr_cloud_append_transformed_dev");
    return LNR_OK;
}

extern "C" int lnr_cloud_normals(const void* grid, int64_t n_points, int32_t knn, double* normals, double* covariances, void* workspace,
                                 size_t workspace_bytes, int64_t* counters_dev, void* stream) {
    LNR_REQUIRE(n_points >= 0 && n_points <= CL_MAX_POINTS, "lnr_cloud_normals: %lld points, the limit is %lld", (long long)n_points,
                (long long)CL_MAX_POINTS);
    LNR_REQUIRE(knn >= 1 && knn <= LNR_KNN_MAX, "lnr_cloud_normals: knn must be in [1, %d], got %d", LNR_KNN_MAX, (int)knn);
    LNR_REQUIRE(grid && counters_dev && workspace && (n_points == 0 || normals), "lnr_cloud_normals: null argument");
    const size_t need = lnr_cloud_workspace(n_points);
    LNR_REQUIRE(workspace_bytes >= need, "lnr_cloud_normals: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counters_dev, 0, 4 * sizeof(int64_t), st) != hipSuccess) {
        lnr_set_error("lnr_cloud_normals: clearing the counters failed");
        return LNR_ERR_LAUNCH;
    }
    if (n_points == 0) return LNR_OK;
    LnrProfScope prof("cloud_normals", st);
    const GridView g = grid_view(grid, n_points);
    uint32_t* fb = (uint32_t*)workspace;
    unsigned long long* cnt = (unsigned long long*)counters_dev;
    const uint32_t n = (uint32_t)n_points;
    hipLaunchKernelGGL(knn_normals, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, g, (int)knn, normals, covariances, fb, cnt);
    hipLaunchKernelGGL(knn_brute, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, g, (int)knn, (const uint32_t*)fb, (const unsigned long long*)cnt,
                       normals, covariances);
    hipLaunchKernelGGL(grid_status, dim3(1), dim3(1), 0, st, g.p, n, cnt);
    LNR_CHECK_LAUNCH("lnr_cloud_normals");
    return LNR_OK;
}

namespace {
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

extern "C" int lnr_icp_correspondences(const void* grid, int64_t n_targets, const double* queries, int64_t n_queries, double max_distance,
                                       int32_t* index, double* sq_distance, int64_t* counters_dev, void* stream) {
    LNR_REQUIRE(n_targets >= 0 && n_targets <= CL_MAX_POINTS && n_queries >= 0 && n_queries <= CL_MAX_POINTS,
                "lnr_icp_correspondences: %lld targets, %lld queries, the limit is %lld each", (long long)n_targets, (long long)n_queries,
                (long long)CL_MAX_POINTS);
    LNR_REQUIRE(isfinite(max_distance) && max_distance > 0.0, "lnr_icp_correspondences: max_distance must be finite and > 0, got %g",
                max_distance);
    LNR_REQUIRE(grid && counters_dev && (n_queries == 0 || (queries && index && sq_distance)), "lnr_icp_correspondences: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counters_dev, 0, 4 * sizeof(int64_t), st) != hipSuccess) {
        lnr_set_error("lnr_icp_correspondences: clearing the counters failed");
        return LNR_ERR_LAUNCH;
    }
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
    if (n_source < 0 || n_source > CL_MAX_POINTS) return 0;
    return icp_layout(n_source).total;
}

extern "C" int lnr_icp_point_to_plane(const void* grid, int64_t n_targets, const double* target_normals,
                                      const double* source, int64_t n_source, double max_distance, const double* init,
                                      double relative_fitness, double relative_rmse, int32_t max_iteration, void* workspace,
                                      size_t workspace_bytes, double* result_dev, int64_t* info_dev, void* stream) {
    LNR_REQUIRE(n_targets >= 0 && n_targets <= CL_MAX_POINTS && n_source >= 0 && n_source <= CL_MAX_POINTS,
                "lnr_icp_point_to_plane: %lld targets, %lld source points, the limit is %lld each", (long long)n_targets,
                (long long)n_source, (long long)CL_MAX_POINTS);
    LNR_REQUIRE(isfinite(max_distance) && max_distance > 0.0, "lnr_icp_point_to_plane: max_distance must be finite and > 0, got %g",
                max_distance);
    LNR_REQUIRE(max_iteration >= 0, "lnr_icp_point_to_plane: max_iteration must be >= 0, got %d", (int)max_iteration);
    LNR_REQUIRE(!(relative_fitness != relative_fitness) && !(relative_rmse != relative_rmse), "lnr_icp_point_to_plane: NaN criteria");
    LNR_REQUIRE(grid && init && workspace && result_dev && info_dev && (n_targets == 0 || target_normals) && (n_source == 0 || source),
                "lnr_icp_point_to_plane: null argument");
    const IcpLayout l = icp_layout(n_source);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_icp_point_to_plane: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    Affine T0;
    for (int k = 0; k < 12; ++k) {
        T0.t[k] = init[k];
        LNR_REQUIRE(isfinite(T0.t[k]), "lnr_icp_point_to_plane: non-finite init entry %d", k);
    }
    LNR_REQUIRE(init[12] == 0.0 && init[13] == 0.0 && init[14] == 0.0 && init[15] == 1.0,
                "lnr_icp_point_to_plane: init's bottom row must be [0, 0, 0, 1]");
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("icp_point_to_plane", st);
    char* ws = (char*)workspace;
    IcpState* s = (IcpState*)(ws + l.state);
    double* part = (double*)(ws + l.part);
    double* pcd = (double*)(ws + l.src);
    const GridView g = grid_view(grid, n_targets);
    const uint32_t ns = (uint32_t)n_source, nb = icp_blocks(n_source);
    hipLaunchKernelGGL(icp_begin, dim3(1), dim3(1), 0, st, s, T0, g.p, (uint32_t)n_targets);
    if (ns) hipLaunchKernelGGL(append_transformed, dim3(blocks_for(ns)), dim3(CL_BLOCK), 0, st, source, ns, T0, pcd);
    hipLaunchKernelGGL(icp_corr<true>, dim3(nb), dim3(CL_BLOCK), 0, st, g, target_normals, (const double*)pcd, ns, max_distance, s, part,
                       (int32_t*)nullptr, (double*)nullptr, (unsigned long long*)nullptr);
    hipLaunchKernelGGL(icp_fold, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)part, nb, s, ns, relative_fitness, relative_rmse, 0);
    LNR_CHECK_LAUNCH("lnr_icp_point_to_plane");
    for (int it = 1; it <= max_iteration; ++it) {
        hipLaunchKernelGGL(icp_solve, dim3(1), dim3(1), 0, st, s);
        if (ns)
            hipLaunchKernelGGL(append_transformed_dev, dim3(blocks_for(ns)), dim3(CL_BLOCK), 0, st, (const double*)pcd, ns,
                               (const double*)s->U, (const uint32_t*)&s->active, pcd);
        hipLaunchKernelGGL(icp_corr<true>, dim3(nb), dim3(CL_BLOCK), 0, st, g, target_normals, (const double*)pcd, ns, max_distance, s,
                           part, (int32_t*)nullptr, (double*)nullptr, (unsigned long long*)nullptr);
        hipLaunchKernelGGL(icp_fold, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)part, nb, s, ns, relative_fitness, relative_rmse, it);
        LNR_CHECK_LAUNCH("lnr_icp_point_to_plane");
    }
    hipLaunchKernelGGL(icp_end, dim3(1), dim3(1), 0, st, (const IcpState*)s, result_dev, info_dev);
    LNR_CHECK_LAUNCH("lnr_icp_point_to_plane");
    return LNR_OK;
}
