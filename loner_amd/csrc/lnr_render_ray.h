// One ray of volume rendering held by one wave (raw2outputs, src/models/rendering_tcnn.py:71-147): shared by the kernels of
// lnr_render.hip, the mesher's fused accumulation (lnr_mesh.hip) and the compositing with the peak (lnr_render_peak.hip).  Each of
// the three includers compiles its own copy, and the three must stay bit-identical: see lnr_mesh.hip and lnr_render_peak.hip for why
// those two translation units are built without SLP vectorisation, and tests/test_gpu_mesh.py and tests/test_gpu_camera.py for the
// checks that fail when an edit here contracts differently in one of them.
#pragma once
#include "lnr_common.h"

#define RENDER_BLOCK 256
#define RAYS_PER_BLOCK (RENDER_BLOCK / 64)
static_assert(RAYS_PER_BLOCK == LNR_LOSS_RAYS_PER_BLOCK, "header constant out of date");

template <int C>
struct RayState {
    float z[C], e[C], T[C], w[C], r[C], dl[C];   // depth, exp(-delta*relu), transmittance, weight, relu(dens), delta*|d|
    bool pos[C];                                  // dens > 0
    float opacity, depth, variance, dnorm;
};

// forward volume rendering of one ray held by one wave
// A lane's C consecutive values of a ray's row through LDS: the wave loads the row in 1 KB instructions (lane l of instruction k takes
// elements 256 k + 4 l ..) and each lane reads its own chunk back.  Loaded directly, a lane's chunk of C = 32 floats starts 128 bytes
// after its neighbour's: every load instruction touches 64 cache lines for 16 bytes each, and the 8 instructions that walk a chunk
// evict each other's lines (four waves x two 8 KB rows against a 32 KB L1) - the compositing of a 2048-sample scan ran at 7 TB/s of L2
// traffic for 1 GB of input.  Rows of 32 floats are padded by 4 in LDS (lane stride 144 bytes: conflict-free ds_read_b128).
template <int C>
__device__ __forceinline__ void load_chunk_staged(const float* __restrict__ src_row, float* stage, int lane, float (&out)[C]) {
    static_assert(C % 4 == 0, "float4 pieces");
#pragma unroll
    for (int k = 0; k < C / 4; ++k) {
        const int i = 256 * k + 4 * lane;
        *reinterpret_cast<float4*>(stage + i + 4 * (i / C)) = *reinterpret_cast<const float4*>(src_row + i);
    }
    __builtin_amdgcn_wave_barrier();                            // a wave's LDS operations complete in order
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(stage + lane * (C + 4) + 4 * q);
        out[4 * q] = v.x; out[4 * q + 1] = v.y; out[4 * q + 2] = v.z; out[4 * q + 3] = v.w;
    }
    __builtin_amdgcn_wave_barrier();
}

template <int C>
__device__ __forceinline__ void render_ray(RayState<C>& st, const float* __restrict__ sigma, const float* __restrict__ z,
                                           const float* __restrict__ noise, float noise_std, uint64_t seed, int ray,
                                           int S, int lane, const float* __restrict__ rayrec, float* stage = nullptr) {
    const int base = lane * C;
    const size_t row = (size_t)ray * S;
    float dens[C];
    bool staged = false;
    if constexpr (C >= 16) {
        if (stage != nullptr && S == 64 * C) {                 // wave-uniform: whole rows
            load_chunk_staged<C>(z + row, stage, lane, st.z);
            load_chunk_staged<C>(sigma + row, stage, lane, dens);
            if (noise) {
                float nz[C];
                load_chunk_staged<C>(noise + row, stage, lane, nz);
#pragma unroll
                for (int t = 0; t < C; ++t) dens[t] += nz[t];
            } else if (noise_std > 0.0f) {
#pragma unroll
                for (int t = 0; t < C; ++t) dens[t] += lnr_rand_normal(seed, (uint64_t)ray, (uint32_t)(base + t)) * noise_std;
            }
            staged = true;
        }
    }
    if (!staged) {
#pragma unroll
    for (int t = 0; t < C; ++t) {
        const int i = base + t;
        if (i < S) {
            st.z[t] = z[row + i];
            float n = 0.0f;
            if (noise) n = noise[row + i];
            else if (noise_std > 0.0f) n = lnr_rand_normal(seed, (uint64_t)ray, (uint32_t)i) * noise_std;
            dens[t] = sigma[row + i] + n;
        } else {
            st.z[t] = 0.0f;
            dens[t] = 0.0f;
        }
    }
    }
    const float dx = rayrec[3], dy = rayrec[4], dz = rayrec[5];
    st.dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
    // z of the sample after my last one comes from the next lane
    const float z_next_lane = __shfl_down(st.z[0], 1, 64);
    float tprod = 1.0f;
#pragma unroll
    for (int t = 0; t < C; ++t) {
        const int i = base + t;
        float delta;
        if (i < S - 1) delta = ((t + 1 < C) ? st.z[(t + 1 < C) ? t + 1 : t] : z_next_lane) - st.z[t];
        else delta = 1e10f;
        delta *= st.dnorm;
        st.dl[t] = delta;
        st.pos[t] = dens[t] > 0.0f;
        st.r[t] = st.pos[t] ? dens[t] : 0.0f;
        st.e[t] = (i < S) ? expf(-delta * st.r[t]) : 1.0f;
        const float alpha = 1.0f - st.e[t];
        st.T[t] = tprod;                           // local exclusive product, fixed up below
        tprod *= (i < S) ? (1.0f - alpha + 1e-10f) : 1.0f;
    }
    const float lane_prefix = wave_excl_prod(tprod, lane);
    float o_part = 0.0f, d_part = 0.0f;
#pragma unroll
    for (int t = 0; t < C; ++t) {
        st.T[t] *= lane_prefix;
        st.w[t] = (base + t < S) ? (1.0f - st.e[t]) * st.T[t] : 0.0f;
        o_part += st.w[t];
        d_part += st.w[t] * st.z[t];
    }
    st.opacity = wave_sum(o_part);
    st.depth = wave_sum(d_part) + (1.0f - st.opacity) * rayrec[12];
    float v_part = 0.0f;
#pragma unroll
    for (int t = 0; t < C; ++t) {
        const float q = st.depth - st.z[t];
        v_part += st.w[t] * q * q;
    }
    st.variance = wave_sum(v_part);
}

// host: samples per lane for S samples per ray (one wave per ray)
static int chunk_for(int S) {
    int c = (S + 63) / 64;
    int p = 1;
    while (p < c) p <<= 1;
    return p;
}

#define DISPATCH_C(S, CALL)                                    \
    switch (chunk_for(S)) {                                    \
        case 1: { constexpr int C = 1; CALL; } break;          \
        case 2: { constexpr int C = 2; CALL; } break;          \
        case 4: { constexpr int C = 4; CALL; } break;          \
        case 8: { constexpr int C = 8; CALL; } break;          \
        case 16: { constexpr int C = 16; CALL; } break;        \
        case 32: { constexpr int C = 32; CALL; } break;        \
        default:                                               \
            lnr_set_error("n_samples=%d not supported (max 2048)", S); \
            return LNR_ERR_UNSUPPORTED;                        \
    }
