// The voxel key of a point set, shared by lnr_cloud.hip (voxel down-sampling, the nearest-neighbour grid) and lnr_mesh_filters.hip
// (vertex clustering): the bound of the finite points, the parameters of the call (origin, edge, bits per axis, digit passes, status)
// folded on the device, and the packed cell index per point.  Both sources are compiled with -ffp-contract=off (build.py EXACT).
// Everything is internal to its translation unit (the anonymous namespace), like the kernels that use it.
#pragma once
#include "lnr_radix_sort.h"

#define CL_BOUND_BLOCKS 1024

enum { CL_MODE_VOXEL = 0, CL_MODE_GRID = 1 };

namespace {

__device__ inline uint32_t live_count(const int32_t* n_dev, uint32_t n_cap) {
    if (!n_dev) return n_cap;
    const int32_t v = *n_dev;
    return v < 0 ? 0u : ((uint32_t)v < n_cap ? (uint32_t)v : n_cap);
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

}  // namespace
