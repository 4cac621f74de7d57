// The walk of one TSDF ray (include/loner_hip.h, "TSDF fusion") with a per-voxel visitor, for the kernels of the sparse volume
// (lnr_tsdf_sparse.hip): the grid frame, the slab clip, the traversal of Amanatides and Woo with its tie rule, and s and q of every
// visited voxel, expression for expression those of tsdf_integrate_kernel (lnr_tsdf.hip).  The dense kernel keeps its own copy: moved
// onto this header it computed the same bytes but took 62 vector registers instead of 50 and measured 3 - 15 % slower
// (docs/HISTORY.md 15), so the two are held together by tests instead - tests/test_gpu_tsdf_sparse.py compares the sparse volume
// with ops.tsdf_integrate byte for byte.  Compiled with -ffp-contract=off (build.py EXACT): every fp64 expression below rounds
// operation by operation, as the header states it and as tests/tsdf_restatement.py restates it.  What a kernel does with a written
// voxel is its own: write(i, j, k, q) runs for every visited voxel with s >= -trunc.
#pragma once
#include <cmath>

#include "lnr_common.h"

#define TSDF_BLOCK 256
#define TSDF_ONE 1048576.0          // 2^20: the fixed-point unit of a truncated distance of 1

namespace {

struct TsdfGrid {
    int32_t n[3];
    double origin[3];
    double v, trunc, front;
};

// bumps tally[0..3] = {rays that updated a node, invalid rays, rays that miss the box, node updates}: one atomic per wave and word
__device__ __forceinline__ void tsdf_tally(int cls, uint32_t updates, unsigned long long* __restrict__ tally) {
#pragma unroll
    for (int c = 0; c < 3; ++c) wave_count_add(cls == c, &tally[c]);
    unsigned long long u = updates;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) u += __shfl_xor(u, o, 64);
    if (u && (threadIdx.x & 63) == 0) atomicAdd(&tally[3], u);
}

// Walks ray `ray` -> 1: invalid, 2: misses the box, 0: walked (the caller knows from its own count whether a voxel was written).
template <class Write>
__device__ __forceinline__ int tsdf_walk(const double* __restrict__ rays, const double* __restrict__ ranges, uint32_t ray, const TsdfGrid& g,
                                         Write&& write) {
    double o[3], d[3], go[3], gd[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = rays[6 * (size_t)ray + a];
        d[a] = rays[6 * (size_t)ray + 3 + a];
        go[a] = (o[a] - g.origin[a]) / g.v + 0.5;           // grid frame: voxel i of the axis is [i, i + 1), the box [0, n]
        gd[a] = d[a] / g.v;
        ok = ok && isfinite(o[a]) && isfinite(d[a]) && isfinite(go[a]) && isfinite(gd[a]);
    }
    const double r = ranges[ray];
    ok = ok && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0) && isfinite(r) && r > 0.0;
    if (!ok) return 1;
    double t0 = fmax(0.0, r - g.front), t1 = r + g.trunc;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (gd[a] == 0.0) {
            inside = inside && go[a] >= 0.0 && go[a] < (double)g.n[a];
        } else {
            const double ta = (0.0 - go[a]) / gd[a], tb = ((double)g.n[a] - go[a]) / gd[a];
            t0 = fmax(t0, fmin(ta, tb));
            t1 = fmin(t1, fmax(ta, tb));
        }
    }
    if (!(inside && t0 < t1)) return 2;
    int32_t c[3], step[3];
    double t_max[3], t_delta[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double e = floor(go[a] + t0 * gd[a]);
        c[a] = e < 0.0 ? 0 : (e > (double)(g.n[a] - 1) ? g.n[a] - 1 : (int32_t)e);
        if (gd[a] == 0.0) {
            step[a] = 0;
            t_max[a] = INFINITY;
            t_delta[a] = INFINITY;
        } else {
            step[a] = gd[a] > 0.0 ? 1 : -1;
            t_max[a] = ((double)(c[a] + (gd[a] > 0.0 ? 1 : 0)) - go[a]) / gd[a];
            t_delta[a] = 1.0 / fabs(gd[a]);
        }
    }
    // every step moves one index one voxel towards a face of the box, so the walk ends after at most nx + ny + nz steps
    for (;;) {
        const double px = g.origin[0] + (double)c[0] * g.v, py = g.origin[1] + (double)c[1] * g.v, pz = g.origin[2] + (double)c[2] * g.v;
        const double s = r - (((px - o[0]) * d[0] + (py - o[1]) * d[1]) + (pz - o[2]) * d[2]);
        if (s >= -g.trunc) write(c[0], c[1], c[2], llrint(fmin(s / g.trunc, 1.0) * TSDF_ONE));       // (every index is in range)
        const int a = (t_max[0] <= t_max[1] && t_max[0] <= t_max[2]) ? 0 : (t_max[1] <= t_max[2] ? 1 : 2);
        // (the arrays are indexed with constants only, so that they stay in registers)
        const double t_next = a == 0 ? t_max[0] : (a == 1 ? t_max[1] : t_max[2]);
        if (!(t_next < t1)) break;
        const int32_t next = a == 0 ? c[0] + step[0] : (a == 1 ? c[1] + step[1] : c[2] + step[2]);
        if (next < 0 || next >= (a == 0 ? g.n[0] : (a == 1 ? g.n[1] : g.n[2]))) break;
        if (a == 0) { c[0] = next; t_max[0] += t_delta[0]; }
        else if (a == 1) { c[1] = next; t_max[1] += t_delta[1]; }
        else { c[2] = next; t_max[2] += t_delta[2]; }
    }
    return 0;
}

// the checks on the lattice's parameters the sparse entry points share (lnr_tsdf_integrate's, with its texts)
int tsdf_check_params(const char* fn, const double* origin, double voxel_size, double trunc, double front) {
    LNR_REQUIRE(origin != nullptr, "%s: null argument", fn);
    LNR_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), "%s: the origin is not finite", fn);
    LNR_REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0, "%s: voxel_size must be finite and > 0, got %g", fn, voxel_size);
    LNR_REQUIRE(std::isfinite(trunc) && trunc > 0.0, "%s: trunc must be finite and > 0, got %g", fn, trunc);
    LNR_REQUIRE(front >= trunc, "%s: front (%g) must be at least trunc (%g)", fn, front, trunc);
    return LNR_OK;
}

TsdfGrid tsdf_grid(int32_t nx, int32_t ny, int32_t nz, const double* origin, double voxel_size, double trunc, double front) {
    TsdfGrid g;
    g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
    for (int a = 0; a < 3; ++a) g.origin[a] = origin[a];
    g.v = voxel_size; g.trunc = trunc; g.front = front;
    return g;
}

}  // namespace
