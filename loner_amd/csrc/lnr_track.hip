// The LiDAR tracker's own kernels (gfx950): the frame cloud, per-point motion compensation and the sky-ray mask.
//
// Replaces, with the definitions stated in include/loner_hip.h ("tracking"):
//   Frame.build_point_cloud            src/common/frame.py:104-145      lnr_frame_cloud
//   LidarScan.motion_compensate        src/common/sensors.py:176-232    lnr_motion_compensate
//   Tracker.compute_sky_rays           src/tracking/tracker.py:257-297  lnr_sky_rays
// This file is compiled with -ffp-contract=off (build.py EXACT): the fp32 expressions that restate the reference's torch ops (the
// frame cloud's products, the interpolation factor, the integer degrees of the sky image) round operation by operation.
//
// The sky mask works on an image of at most 181 x 360 pixels.  The passes over the scan (the degree bounds, the scatter) are grid
// launches; the closing, the ordered compaction and the directions run in ONE workgroup that keeps the image in global memory (it
// stays in L2) and separates its phases with __syncthreads().  Order is kept by walking the pixels in row-major chunks of the block
// size: a ballot per wave ranks the kept lanes, the wave totals go through LDS, and a running base carries over the chunks.
#include "lnr_common.h"

#include <limits.h>
#include <math.h>

#define TR_BLOCK 256
#define SKY_COLS 360
#define SKY_MAX_ROWS 181
#define SKY_IMG_BYTES 65536                 /* >= SKY_MAX_ROWS * SKY_COLS, a multiple of 256 */
#define SKY_HEAD_BYTES 256
#define SKY_CLOSE_BLOCK 1024
#define SKY_TOP_ROWS 3
#define SKY_HORIZON_OFFSET 10.0f
#define TR_MAX_POINTS ((int64_t)INT32_MAX - 4096)

// the device-side parameters of one lnr_sky_rays call (head of the workspace)
struct SkyHead {
    int32_t theta_min, theta_max, phi_min, phi_max;
    uint32_t nonfinite;
};

// the per-call constants of lnr_motion_compensate
struct MocompConsts {
    double aa[3];           // theta * axis of R_start^-1 R_end
    double Rs[9];           // R_start
    double ts[3], te[3];    // translations of the start and end pose
    double Ti[12];          // top three rows of T_target^-1
};

namespace {

inline uint32_t blocks_for(int64_t n) { return (uint32_t)((n + TR_BLOCK - 1) / TR_BLOCK); }

// ------------------------------------------------------------------------------------------------ frame cloud
__global__ __launch_bounds__(TR_BLOCK) void frame_cloud(const float* __restrict__ dirs, const float* __restrict__ dist, int64_t n,
                                                        int64_t start, int64_t step, uint32_t m, double* __restrict__ points) {
    const uint32_t j = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (j >= m) return;
    const int64_t i = start + (int64_t)j * step;            // start + (m - 1) step < stop <= n (checked by the host)
    const float d = dist[i];
    points[3 * (size_t)j + 0] = (double)(dirs[i] * d);
    points[3 * (size_t)j + 1] = (double)(dirs[n + i] * d);
    points[3 * (size_t)j + 2] = (double)(dirs[2 * n + i] * d);
}

// ------------------------------------------------------------------------------------------------ motion compensation
template <typename T>
__global__ __launch_bounds__(TR_BLOCK) void motion_compensate(float* __restrict__ dirs, float* __restrict__ dist,
                                                              const T* __restrict__ stamps, uint32_t n, T t0, T denom, MocompConsts c) {
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double f = (double)((stamps[i] - t0) / denom);    // formed in the timestamps' type, as the reference's tensor expression
    const double theta = sqrt((c.aa[0] * c.aa[0] + c.aa[1] * c.aa[1]) + c.aa[2] * c.aa[2]);
    double R[9];
    if (theta < 1e-9) {                                     // NUMERIC_TOLERANCE: no relative rotation
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = c.Rs[k];
    } else {
        const double ax = c.aa[0] / theta, ay = c.aa[1] / theta, az = c.aa[2] / theta;
        const double phi = f * theta;
        const double s = sin(phi), v = 1.0 - cos(phi);
        // Rodrigues: I + s K + v K^2
        const double E[9] = {1.0 - v * (ay * ay + az * az), v * ax * ay - s * az, v * ax * az + s * ay,
                             v * ax * ay + s * az, 1.0 - v * (ax * ax + az * az), v * ay * az - s * ax,
                             v * ax * az - s * ay, v * ay * az + s * ax, 1.0 - v * (ax * ax + ay * ay)};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) R[3 * a + b] = (c.Rs[3 * a] * E[b] + c.Rs[3 * a + 1] * E[3 + b]) + c.Rs[3 * a + 2] * E[6 + b];
    }
    const double d = (double)dist[i];
    const double p[3] = {(double)dirs[i] * d, (double)dirs[(size_t)n + i] * d, (double)dirs[2 * (size_t)n + i] * d};
    double w[3], q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = ((R[3 * a] * p[0] + R[3 * a + 1] * p[1]) + R[3 * a + 2] * p[2]) + (c.ts[a] + f * (c.te[a] - c.ts[a]));
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = ((c.Ti[4 * a] * w[0] + c.Ti[4 * a + 1] * w[1]) + c.Ti[4 * a + 2] * w[2]) + c.Ti[4 * a + 3];
    const double r = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    dist[i] = (float)r;
    dirs[i] = (float)(q[0] / r);
    dirs[(size_t)n + i] = (float)(q[1] / r);
    dirs[2 * (size_t)n + i] = (float)(q[2] / r);
}

// ------------------------------------------------------------------------------------------------ sky rays
#define SKY_RAD2DEG 57.29577951308232f       /* torch's rad2deg constant, rounded to fp32 */
#define SKY_DEG2RAD 0.017453292519943295f

// integer degrees of one direction as tracker.py:264-265 forms them in fp32; false for a non-finite direction
__device__ inline bool sky_degrees(const float* __restrict__ dirs, size_t n, size_t i, int* theta, int* phi) {
    const float x = dirs[i], y = dirs[n + i], z = dirs[2 * n + i];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    *theta = (int)rintf(atan2f(y, x) * SKY_RAD2DEG);                       // [-180, 180]
    *phi = (int)rintf(atan2f(sqrtf(x * x + y * y), z) * SKY_RAD2DEG);      // [0, 180]
    return true;
}

__global__ __launch_bounds__(TR_BLOCK) void sky_init(SkyHead* h, uint32_t* img_words, uint32_t n_words, int32_t* info) {
    const uint32_t t = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (t < n_words) img_words[t] = 0u;
    if (t == 0) {
        h->theta_min = INT_MAX; h->theta_max = INT_MIN; h->phi_min = INT_MAX; h->phi_max = INT_MIN; h->nonfinite = 0u;
    }
    if (t < 8) info[t] = 0;
}

__global__ __launch_bounds__(TR_BLOCK) void sky_bounds(const float* __restrict__ dirs, uint32_t n, SkyHead* h) {
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    int tmin = INT_MAX, tmax = INT_MIN, pmin = INT_MAX, pmax = INT_MIN;
    uint32_t bad = 0;
    if (i < n) {
        int th, ph;
        if (sky_degrees(dirs, n, i, &th, &ph)) { tmin = tmax = th; pmin = pmax = ph; }
        else bad = 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tmin = min(tmin, __shfl_xor(tmin, o, 64)); tmax = max(tmax, __shfl_xor(tmax, o, 64));
        pmin = min(pmin, __shfl_xor(pmin, o, 64)); pmax = max(pmax, __shfl_xor(pmax, o, 64));
        bad += __shfl_xor(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (tmin <= tmax) {
            atomicMin(&h->theta_min, tmin); atomicMax(&h->theta_max, tmax);
            atomicMin(&h->phi_min, pmin); atomicMax(&h->phi_max, pmax);
        }
        if (bad) atomicAdd(&h->nonfinite, bad);
    }
}

__global__ __launch_bounds__(TR_BLOCK) void sky_scatter(const float* __restrict__ dirs, uint32_t n, const SkyHead* __restrict__ h,
                                                        uint8_t* __restrict__ img) {
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= n) return;
    int th, ph;
    if (!sky_degrees(dirs, n, i, &th, &ph)) return;
    const int row = ph - h->phi_min;
    int col = th - h->theta_min;
    if (col == SKY_COLS) col = 0;                            // theta_img[theta_img == 360] = 0
    if (row >= 0 && row < SKY_MAX_ROWS && col >= 0 && col < SKY_COLS) img[row * SKY_COLS + col] = 1;      // every writer stores the same 1
}

// One workgroup: dilation, erosion (out-of-image neighbours ignored, no azimuth wrap), the top rows, then the zero pixels in row-major
// order -> unit vectors -> rotated -> those more than 10 degrees above the horizon, compacted in order into sky [3, stride].
__global__ __launch_bounds__(SKY_CLOSE_BLOCK) void sky_close(const SkyHead* __restrict__ h, const uint8_t* __restrict__ occ,
                                                             uint8_t* __restrict__ dil, uint8_t* __restrict__ closed, const float* rot9,
                                                             float* __restrict__ sky, uint32_t stride, int32_t* __restrict__ info) {
    __shared__ uint32_t wave_tot[SKY_CLOSE_BLOCK / 64];
    __shared__ uint32_t base_s, cand_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows = h->phi_max >= h->phi_min ? min(h->phi_max - h->phi_min + 1, SKY_MAX_ROWS) : 0;
    const int npix = rows * SKY_COLS;
    if (tid == 0) { base_s = 0u; cand_s = 0u; }
    for (int p = tid; p < npix; p += SKY_CLOSE_BLOCK) {
        const int r = p / SKY_COLS, c = p - r * SKY_COLS;
        uint8_t m = 0;
        for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
                const int rr = r + dr, cc = c + dc;
                if (rr >= 0 && rr < rows && cc >= 0 && cc < SKY_COLS) m |= occ[rr * SKY_COLS + cc];
            }
        dil[p] = m;
    }
    __syncthreads();
    for (int p = tid; p < npix; p += SKY_CLOSE_BLOCK) {
        const int r = p / SKY_COLS, c = p - r * SKY_COLS;
        uint8_t m = 1;
        for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
                const int rr = r + dr, cc = c + dc;
                if (rr >= 0 && rr < rows && cc >= 0 && cc < SKY_COLS) m &= dil[rr * SKY_COLS + cc];
            }
        closed[p] = r < SKY_TOP_ROWS ? (uint8_t)1 : m;
    }
    __syncthreads();
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rot9[k];
    const int phi_min = h->phi_min, theta_min = h->theta_min;
    uint32_t n_cand = 0;
    for (int p0 = 0; p0 < npix; p0 += SKY_CLOSE_BLOCK) {
        const int p = p0 + tid;
        bool keep = false;
        float xw = 0.f, yw = 0.f, zw = 0.f;
        if (p < npix && closed[p] == 0) {
            ++n_cand;
            const int r = p / SKY_COLS, c = p - r * SKY_COLS;
            const float phi = (float)(r + phi_min) * SKY_DEG2RAD, theta = (float)(c + theta_min) * SKY_DEG2RAD;
            const float sp = sinf(phi);
            const float x = sp * cosf(theta), y = sp * sinf(theta), z = cosf(phi);
            xw = (R[0] * x + R[1] * y) + R[2] * z;
            yw = (R[3] * x + R[4] * y) + R[5] * z;
            zw = (R[6] * x + R[7] * y) + R[8] * z;
            const float elev = 90.0f - atan2f(sqrtf(xw * xw + yw * yw), zw) * SKY_RAD2DEG;
            keep = elev > SKY_HORIZON_OFFSET;
        }
        const unsigned long long mask = __ballot(keep);
        const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t pre = base_s, tot = 0;
#pragma unroll
        for (int k = 0; k < SKY_CLOSE_BLOCK / 64; ++k) {
            const uint32_t s = wave_tot[k];
            pre += k < wave ? s : 0u;
            tot += s;
        }
        if (keep) {
            const uint32_t o = pre + rank;
            if (o < stride) { sky[o] = xw; sky[(size_t)stride + o] = yw; sky[2 * (size_t)stride + o] = zw; }
        }
        __syncthreads();
        if (tid == 0) base_s += tot;
        __syncthreads();
    }
    if (n_cand) atomicAdd(&cand_s, n_cand);
    __syncthreads();
    if (tid == 0) {
        info[0] = h->nonfinite ? 1 : 0;
        info[1] = (int32_t)base_s;
        info[2] = (int32_t)cand_s;
        info[3] = rows;
        info[4] = phi_min;
        info[5] = theta_min;
        info[6] = (int32_t)h->nonfinite;
        info[7] = 0;
    }
}

}  // namespace

extern "C" int lnr_frame_cloud(const float* ray_directions, const float* distances, int64_t n_points, int64_t start, int64_t stop,
                               int64_t step, double* points, void* stream) {
    LNR_REQUIRE(n_points >= 0 && n_points <= TR_MAX_POINTS, "lnr_frame_cloud: %lld points, the limit is %lld", (long long)n_points,
                (long long)TR_MAX_POINTS);
    LNR_REQUIRE(start >= 0 && stop <= n_points && step >= 1, "lnr_frame_cloud: bad window [%lld, %lld) step %lld of %lld points",
                (long long)start, (long long)stop, (long long)step, (long long)n_points);
    const int64_t m = stop > start ? (stop - start + step - 1) / step : 0;
    if (m == 0) return LNR_OK;
    LNR_REQUIRE(ray_directions && distances && points, "lnr_frame_cloud: null argument");
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("frame_cloud", st);
    hipLaunchKernelGGL(frame_cloud, dim3(blocks_for(m)), dim3(TR_BLOCK), 0, st, ray_directions, distances, n_points, start, step,
                       (uint32_t)m, points);
    LNR_CHECK_LAUNCH("lnr_frame_cloud");
    return LNR_OK;
}

extern "C" int lnr_motion_compensate(float* ray_directions, float* distances, const void* timestamps, int32_t timestamps_fp64,
                                     int64_t n_points, double t0, double denom, const double* consts, void* stream) {
    LNR_REQUIRE(n_points >= 0 && n_points <= TR_MAX_POINTS, "lnr_motion_compensate: %lld points, the limit is %lld", (long long)n_points,
                (long long)TR_MAX_POINTS);
    LNR_REQUIRE(consts && (n_points == 0 || (ray_directions && distances && timestamps)), "lnr_motion_compensate: null argument");
    LNR_REQUIRE(isfinite(t0) && isfinite(denom), "lnr_motion_compensate: non-finite pose times");
    MocompConsts c;
    double* flat = (double*)&c;
    for (int k = 0; k < LNR_MOCOMP_CONSTS; ++k) {
        flat[k] = consts[k];
        LNR_REQUIRE(isfinite(flat[k]), "lnr_motion_compensate: non-finite pose constant %d", k);
    }
    if (n_points == 0) return LNR_OK;
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("motion_compensate", st);
    const uint32_t n = (uint32_t)n_points;
    if (timestamps_fp64)
        hipLaunchKernelGGL(motion_compensate<double>, dim3(blocks_for(n)), dim3(TR_BLOCK), 0, st, ray_directions, distances,
                           (const double*)timestamps, n, t0, denom, c);
    else
        hipLaunchKernelGGL(motion_compensate<float>, dim3(blocks_for(n)), dim3(TR_BLOCK), 0, st, ray_directions, distances,
                           (const float*)timestamps, n, (float)t0, (float)denom, c);
    LNR_CHECK_LAUNCH("lnr_motion_compensate");
    return LNR_OK;
}

extern "C" size_t lnr_sky_rays_workspace(void) { return SKY_HEAD_BYTES + 3 * (size_t)SKY_IMG_BYTES; }

extern "C" int lnr_sky_rays(const float* ray_directions, int64_t n_points, const float* rotation, void* workspace, size_t workspace_bytes,
                            float* sky, int64_t sky_stride, int32_t* info_dev, void* stream) {
    LNR_REQUIRE(n_points >= 1 && n_points <= TR_MAX_POINTS, "lnr_sky_rays: %lld points (1 .. %lld)", (long long)n_points,
                (long long)TR_MAX_POINTS);
    LNR_REQUIRE(ray_directions && rotation && workspace && sky && info_dev, "lnr_sky_rays: null argument");
    LNR_REQUIRE(workspace_bytes >= lnr_sky_rays_workspace(), "lnr_sky_rays: workspace of %zu bytes, %zu needed", workspace_bytes,
                lnr_sky_rays_workspace());
    LNR_REQUIRE(sky_stride >= LNR_SKY_MAX_RAYS, "lnr_sky_rays: sky holds %lld rays per row, %d needed", (long long)sky_stride,
                LNR_SKY_MAX_RAYS);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("sky_rays", st);
    char* ws = (char*)workspace;
    SkyHead* h = (SkyHead*)ws;
    uint8_t* occ = (uint8_t*)(ws + SKY_HEAD_BYTES);
    uint8_t* dil = occ + SKY_IMG_BYTES;
    uint8_t* closed = dil + SKY_IMG_BYTES;
    const uint32_t n = (uint32_t)n_points, words = SKY_IMG_BYTES / 4;
    hipLaunchKernelGGL(sky_init, dim3(blocks_for(words)), dim3(TR_BLOCK), 0, st, h, (uint32_t*)occ, words, info_dev);
    hipLaunchKernelGGL(sky_bounds, dim3(blocks_for(n)), dim3(TR_BLOCK), 0, st, ray_directions, n, h);
    hipLaunchKernelGGL(sky_scatter, dim3(blocks_for(n)), dim3(TR_BLOCK), 0, st, ray_directions, n, (const SkyHead*)h, occ);
    hipLaunchKernelGGL(sky_close, dim3(1), dim3(SKY_CLOSE_BLOCK), 0, st, (const SkyHead*)h, (const uint8_t*)occ, dil, closed,
                       rotation, sky, (uint32_t)sky_stride, info_dev);
    LNR_CHECK_LAUNCH("lnr_sky_rays");
    return LNR_OK;
}
