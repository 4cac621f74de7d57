// Depth images to colour (gfx950).  Compile with -ffp-contract=off: every step rounds on its own, as the reference's torch ops do.
//
// Replaces  save_depth   analysis/render_utils.py:116-127 of the reference (clip, normalise, matplotlib colour map, mask, uint8)
//
// One thread per pixel: 4 bytes in, 4 bytes out, and a 768-byte table that stays in cache.
#include "lnr_common.h"

__global__ void __launch_bounds__(256)
depth_colormap_kernel(const float* __restrict__ values, int64_t n, float multiplier, float lo, float hi, float span,
                      const uint8_t* __restrict__ table, uint32_t* __restrict__ rgba) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = values[i] * multiplier;
    uint32_t px;
    if (v != v) px = 0u;                                             // matplotlib's "bad" colour: (0, 0, 0, 0)
    else if (v >= hi) px = 0xFF000000u;                              // the mask: (0, 0, 0, 255)
    else {
        const float c = fminf(fmaxf(v, lo), hi);
        const float x = fminf(fmaxf((c - lo) / span, 0.0f), 1.0f);
        int k = (int)floorf(x * 256.0f);
        k = k > 255 ? 255 : (k < 0 ? 0 : k);
        px = (uint32_t)table[3 * k] | ((uint32_t)table[3 * k + 1] << 8) | ((uint32_t)table[3 * k + 2] << 16) | 0xFF000000u;
    }
    rgba[i] = px;                                                    // little endian: bytes R, G, B, A
}

extern "C" int lnr_depth_colormap(const float* values, int64_t n, float multiplier, double min_depth, double max_depth,
                                  const uint8_t* table, uint8_t* rgba, void* stream) {
    LNR_REQUIRE(n >= 0 && (n == 0 || (values && table && rgba)), "lnr_depth_colormap: bad argument");
    LNR_REQUIRE(max_depth > min_depth, "lnr_depth_colormap: max_depth must exceed min_depth");
    LNR_REQUIRE(((uintptr_t)rgba & 3u) == 0, "lnr_depth_colormap: rgba must be 4-byte aligned");
    if (n == 0) return LNR_OK;
    hipLaunchKernelGGL(depth_colormap_kernel, dim3(lnr_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, values, n, multiplier,
                       (float)min_depth, (float)max_depth, (float)(max_depth - min_depth), table, reinterpret_cast<uint32_t*>(rgba));
    LNR_CHECK_LAUNCH("lnr_depth_colormap");
    return LNR_OK;
}
