// The device-wide stable sort of (uint64 key, uint32 payload) pairs and the exclusive scan it is built on, shared by lnr_cloud.hip
// (voxel and grid keys) and lnr_scan.hip (time keys of a LiDAR scan).
//   scan       in place over uint32 words: per-tile sums, one workgroup scans the sums, per-tile apply
//   sort       LSD radix, 8-bit digits: count (per-block histograms), exclusive scan of the [digit][block] table, stable scatter
//              (rank within a 256-element chunk from eight ballots per wave).  The host enqueues all CL_MAX_PASSES passes; the number
//              of points and of passes the key needs live on the device (*n_dev, *npasses_dev), and a pass at or above *npasses_dev
//              returns at once, so the host never waits for either.  After the call the sorted pairs are in the b buffers when
//              *npasses_dev is odd, in the a buffers otherwise (sorted_keys / sorted_idx)
// Everything is internal to its translation unit (the anonymous namespace), like the kernels that use it.
#pragma once
#include "lnr_cloud_grid.h"

#define CL_SCAN_PER_THREAD 8
#define CL_SCAN_TILE (CL_BLOCK * CL_SCAN_PER_THREAD)
#define CL_RADIX 256
#define CL_MAX_PASSES 8

namespace {

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

// ------------------------------------------------------------------------------------------------ stable LSD radix sort
__global__ __launch_bounds__(CL_BLOCK) void radix_count(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ n_dev,
                                                        const int32_t* __restrict__ npasses_dev, int pass, uint32_t* __restrict__ counts,
                                                        uint32_t n_blocks) {
    if (pass >= *npasses_dev) return;
    __shared__ uint32_t h[CL_RADIX];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n = *n_dev, shift = 8 * pass;
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
                                                          const uint32_t* __restrict__ n_dev, const int32_t* __restrict__ npasses_dev,
                                                          int pass, const uint32_t* __restrict__ offsets, uint32_t n_blocks) {
    if (pass >= *npasses_dev) return;
    __shared__ uint32_t run[CL_RADIX];
    __shared__ uint32_t wc[CL_BLOCK / 64][CL_RADIX];
    const uint32_t n = *n_dev, shift = 8 * pass;
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

// the buffers of one sort over a capacity of n pairs; counts holds CL_RADIX * sort_blocks words, sums scan_tiles(that) + 1
struct RadixBuffers {
    uint64_t *ka, *kb;
    uint32_t *ia, *ib, *counts, *sums;
    uint32_t sort_blocks;
};

uint32_t radix_sort_blocks(int64_t n) { return (uint32_t)((n + CL_SORT_TILE - 1) / CL_SORT_TILE); }

// all CL_MAX_PASSES passes over (ka, ia), ping-ponging with (kb, ib); the caller checks the launches
void enqueue_radix_sort(const RadixBuffers& r, const uint32_t* n_dev, const int32_t* npasses_dev, hipStream_t st) {
    for (int pass = 0; pass < CL_MAX_PASSES; ++pass) {
        const uint64_t* kin = (pass & 1) ? r.kb : r.ka;
        uint64_t* kout = (pass & 1) ? r.ka : r.kb;
        const uint32_t* iin = (pass & 1) ? r.ib : r.ia;
        uint32_t* iout = (pass & 1) ? r.ia : r.ib;
        hipLaunchKernelGGL(radix_count, dim3(r.sort_blocks), dim3(CL_BLOCK), 0, st, kin, n_dev, npasses_dev, pass, r.counts, r.sort_blocks);
        enqueue_scan(r.counts, CL_RADIX * r.sort_blocks, r.sums, nullptr, npasses_dev, pass, st);
        hipLaunchKernelGGL(radix_scatter, dim3(r.sort_blocks), dim3(CL_BLOCK), 0, st, kin, iin, kout, iout, n_dev, npasses_dev, pass,
                           (const uint32_t*)r.counts, r.sort_blocks);
    }
}

__device__ inline const uint64_t* sorted_keys(int32_t npasses, const uint64_t* a, const uint64_t* b) { return (npasses & 1) ? b : a; }
__device__ inline const uint32_t* sorted_idx(int32_t npasses, const uint32_t* a, const uint32_t* b) { return (npasses & 1) ? b : a; }

}  // namespace
