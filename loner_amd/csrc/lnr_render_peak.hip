// Compositing with the peak (gfx950): lnr_render_forward without the [N,S] weights, plus each ray's sample of maximal weight.
//
// Replaces  the argmax / gather over weights_fine and samples_fine   analysis/renderer.py:195-198 of the reference
//
// This file is compiled without SLP vectorisation (build.py), as lnr_mesh.hip is and for its reason: the kernel composites with the
// same render_ray as lnr_render_forward (lnr_render_ray.h), and which multiply-adds contract into fmas depends on the code around
// them.  Placed beside render_forward_kernel in lnr_render.hip, with the vectoriser on, one pair of render_ray's multiplies became a
// packed v_pk_mul_f32 for every C >= 2, its add stayed separate, and depths came out an ulp away from lnr_render_forward's at 1024
// samples per ray.  Without the vectoriser the kernel has, for every C, exactly the multiplies, fmas, adds and subtracts of
// render_forward_kernel, and depth, opacity and variance are that kernel's bit for bit (tests/test_gpu_camera.py).
#include "lnr_common.h"
#include "lnr_render_ray.h"

// (weight, index) ordered as torch.argmax orders them: a NaN is maximal, the larger weight wins, and on equal terms the lower index
__device__ __forceinline__ bool peak_before(float wa, int ia, float wb, int ib) {
    const bool na = wa != wa, nb = wb != wb;
    if (na || nb) return na && (!nb || ia < ib);
    return wa > wb || (wa == wb && ia < ib);
}

// render_forward_kernel without the [N,S] weights: the ray's peak - the sample of maximal weight - is taken from the registers that
// hold them (the depth image's consistency channel reads nothing else of the weights, analysis/renderer.py:195-198 of the reference).
// Per lane the first maximum of its C samples, then a butterfly on (weight, index, z).
template <int C>
__global__ void __launch_bounds__(RENDER_BLOCK)
render_forward_peak_kernel(const float* __restrict__ sigma, const float* __restrict__ z, const float* __restrict__ rays, int n_rays,
                           const int32_t* __restrict__ n_rays_dev, int S, const float* __restrict__ noise, float noise_std,
                           uint64_t seed, float* __restrict__ depth, float* __restrict__ opacity, float* __restrict__ variance,
                           float* __restrict__ peak_z, int32_t* __restrict__ peak_index) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= lnr_live_rays(n_rays, n_rays_dev)) return;
    const float* rr = rays + (size_t)ray * LNR_RAY_STRIDE;
    RayState<C> st;
    extern __shared__ __attribute__((aligned(16))) float render_stage[];       // C >= 16: 64 (C + 4) floats per wave (the host sizes it)
    float* stage = C >= 16 ? render_stage + (threadIdx.x >> 6) * 64 * (C + 4) : nullptr;
    render_ray<C>(st, sigma, z, noise, noise_std, seed, ray, S, lane, rr, stage);
    float bw = -INFINITY, bz = 0.0f;                     // a lane without a sample (ragged C) loses against every weight
    int bi = 0x7FFFFFFF;
#pragma unroll
    for (int t = 0; t < C; ++t) {
        const int i = lane * C + t;
        if (i < S && peak_before(st.w[t], i, bw, bi)) { bw = st.w[t]; bi = i; bz = st.z[t]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ow = __shfl_xor(bw, o, 64), oz = __shfl_xor(bz, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (peak_before(ow, oi, bw, bi)) { bw = ow; bi = oi; bz = oz; }
    }
    if (lane == 0) {
        if (depth) depth[ray] = st.depth;
        if (opacity) opacity[ray] = st.opacity;
        if (variance) variance[ray] = st.variance;
        if (peak_z) peak_z[ray] = bz;
        if (peak_index) peak_index[ray] = bi;
    }
}

extern "C" int lnr_render_forward_peak(const float* sigma, const float* z, const float* rays, int32_t n_rays, const int32_t* n_rays_dev,
                                       int32_t n_samples, const float* noise, float noise_std, uint64_t seed, float* depth,
                                       float* opacity, float* variance, float* peak_z, int32_t* peak_index, void* stream) {
    LNR_REQUIRE(sigma && z && rays && n_rays >= 0 && n_samples >= 2, "lnr_render_forward_peak: bad argument");
    if (n_rays == 0) return LNR_OK;
    const dim3 grid(lnr_div_up(n_rays, RAYS_PER_BLOCK)), block(RENDER_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_C(n_samples, hipLaunchKernelGGL(render_forward_peak_kernel<C>, grid, block, C >= 16 ? RAYS_PER_BLOCK * 64 * (C + 4) * sizeof(float) : 0, st,
                                             sigma, z, rays, n_rays, n_rays_dev, n_samples, noise, noise_std, seed, depth, opacity, variance,
                                             peak_z, peak_index));
    LNR_CHECK_LAUNCH("lnr_render_forward_peak");
    return LNR_OK;
}
