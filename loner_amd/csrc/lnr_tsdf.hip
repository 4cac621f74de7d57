// TSDF fusion of LiDAR rays into a dense volume (gfx950): the classical map the neural one is compared against.
//
// Replaces  open3d.pipelines.integration.UniformTSDFVolume.integrate / ScalableTSDFVolume.integrate   for range rays instead of depth
// images, with a definition of our own (include/loner_hip.h, "TSDF fusion"): every ray walks the voxels of its segment
// [max(0, r - front), r + trunc] by the traversal of Amanatides and Woo (1987) in fp64 and adds its truncated projective distance, in
// fixed point, to the node of every voxel it visits.  The sums are integers and the atomics return nothing, so a volume is a function
// of the set of rays: the order of the waves, of the rays and of the calls does not change a bit of it.
//
// This file is compiled with -ffp-contract=off (build.py): every fp64 expression below rounds operation by operation, as the header
// states it and as tests/tsdf_restatement.py restates it.
//
// One lane per ray.  Neighbouring rays of a scan pattern walk neighbouring voxels, so a wave's atomics of one step fall into a few
// cache lines; the lanes of a wave run as long as its longest walk.  Measured (profiles/tsdf.txt): 7.4 - 9.8 G node updates per second
// with nine voxels per ray and with two hundred alike, so the uneven walks of carving are not what bounds the kernel.
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

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_integrate_kernel(const double* __restrict__ rays, const double* __restrict__ ranges,
                                                                     uint32_t n_rays, const TsdfGrid g, unsigned long long* __restrict__ sum,
                                                                     uint32_t* __restrict__ count, unsigned long long* __restrict__ tally) {
    const uint32_t ray = blockIdx.x * TSDF_BLOCK + threadIdx.x;
    int cls = -1;                                               // 0: updated a node, 1: invalid, 2: misses the box, 3: wrote nothing
    uint32_t updates = 0;
    if (ray < n_rays) {
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
        if (!ok) {
            cls = 1;
        } else {
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
            if (!(inside && t0 < t1)) {
                cls = 2;
            } else {
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
                    const double px = g.origin[0] + (double)c[0] * g.v, py = g.origin[1] + (double)c[1] * g.v,
                                 pz = g.origin[2] + (double)c[2] * g.v;
                    const double s = r - (((px - o[0]) * d[0] + (py - o[1]) * d[1]) + (pz - o[2]) * d[2]);
                    if (s >= -g.trunc) {
                        const long long q = llrint(fmin(s / g.trunc, 1.0) * TSDF_ONE);
                        const size_t node = ((size_t)c[0] * g.n[1] + c[1]) * g.n[2] + c[2];      // < 2^31, and every index is in range
                        atomicAdd(sum + node, (unsigned long long)q);                            // (two's complement: a signed add)
                        atomicAdd(count + node, 1u);
                        ++updates;
                    }
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
                cls = updates ? 0 : 3;
            }
        }
    }
    tsdf_tally(cls, updates, tally);
}

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_field_kernel(const long long* __restrict__ sum, const uint32_t* __restrict__ count,
                                                                 uint32_t n, uint32_t min_count, float* __restrict__ field,
                                                                 uint8_t* __restrict__ valid) {
    const uint32_t i = blockIdx.x * TSDF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = count[i];
    field[i] = c > 0 ? (float)(-(double)sum[i] / ((double)c * TSDF_ONE)) : 0.0f;
    valid[i] = c >= min_count ? 1 : 0;
}

int tsdf_check_dims(int32_t nx, int32_t ny, int32_t nz, const char* what) {
    LNR_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: every axis needs at least two nodes (%d x %d x %d)", what, nx, ny, nz);
    LNR_REQUIRE((int64_t)nx * ny * nz < ((int64_t)1 << 31), "%s: %lld nodes, the limit is 2^31 - 1", what, (long long)nx * ny * nz);
    return LNR_OK;
}

}  // namespace

extern "C" int lnr_tsdf_integrate(const double* rays, const double* ranges, int64_t n_rays, int32_t nx, int32_t ny, int32_t nz,
                                  const double* origin, double voxel_size, double trunc, double front, int64_t* sum, uint32_t* count,
                                  int64_t* info_dev, void* stream) {
    if (int rc = tsdf_check_dims(nx, ny, nz, "lnr_tsdf_integrate")) return rc;
    LNR_REQUIRE(n_rays >= 0 && n_rays < ((int64_t)1 << 32) - TSDF_BLOCK, "lnr_tsdf_integrate: %lld rays, the limit is 2^32 - %d",
                (long long)n_rays, TSDF_BLOCK + 1);
    LNR_REQUIRE(origin && sum && count && info_dev && (n_rays == 0 || (rays && ranges)), "lnr_tsdf_integrate: null argument");
    LNR_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), "lnr_tsdf_integrate: the origin is not finite");
    LNR_REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0, "lnr_tsdf_integrate: voxel_size must be finite and > 0, got %g", voxel_size);
    LNR_REQUIRE(std::isfinite(trunc) && trunc > 0.0, "lnr_tsdf_integrate: trunc must be finite and > 0, got %g", trunc);
    LNR_REQUIRE(front >= trunc, "lnr_tsdf_integrate: front (%g) must be at least trunc (%g)", front, trunc);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("tsdf_integrate", st);
    if (hipMemsetAsync(info_dev, 0, 8 * sizeof(int64_t), st) != hipSuccess) {
        lnr_set_error("lnr_tsdf_integrate: clearing the info words failed");
        return LNR_ERR_LAUNCH;
    }
    if (n_rays > 0) {
        TsdfGrid g;
        g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
        for (int a = 0; a < 3; ++a) g.origin[a] = origin[a];
        g.v = voxel_size; g.trunc = trunc; g.front = front;
        hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((uint32_t)((n_rays + TSDF_BLOCK - 1) / TSDF_BLOCK)), dim3(TSDF_BLOCK), 0, st, rays,
                           ranges, (uint32_t)n_rays, g, (unsigned long long*)sum, count, (unsigned long long*)(info_dev + 1));
    }
    LNR_CHECK_LAUNCH("lnr_tsdf_integrate");
    return LNR_OK;
}

extern "C" int lnr_tsdf_field(const int64_t* sum, const uint32_t* count, int32_t nx, int32_t ny, int32_t nz, uint32_t min_count,
                              float* field, uint8_t* valid, void* stream) {
    if (int rc = tsdf_check_dims(nx, ny, nz, "lnr_tsdf_field")) return rc;
    LNR_REQUIRE(sum && count && field && valid, "lnr_tsdf_field: null argument");
    LNR_REQUIRE(min_count >= 1, "lnr_tsdf_field: min_count must be at least 1");
    const uint32_t n = (uint32_t)nx * (uint32_t)ny * (uint32_t)nz;
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("tsdf_field", st);
    hipLaunchKernelGGL(tsdf_field_kernel, dim3((n + TSDF_BLOCK - 1) / TSDF_BLOCK), dim3(TSDF_BLOCK), 0, st, (const long long*)sum, count, n,
                       min_count, field, valid);
    LNR_CHECK_LAUNCH("lnr_tsdf_field");
    return LNR_OK;
}
