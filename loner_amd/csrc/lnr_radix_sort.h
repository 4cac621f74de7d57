// The device-wide stable sort of (uint64 key, uint32 payload) pairs and the exclusive scan it is built on, shared by every tool that
// sorts: lnr_cloud.hip (voxel and grid keys), lnr_scan.hip (time keys of a LiDAR scan), lnr_raycast.hip (Morton codes of the BVH),
// lnr_mesh_tools.hip and lnr_mesh_filters.hip (edge, vertex, cluster and triangle keys).
//   scan       in place over uint32 words: per-tile sums, one workgroup scans the sums, per-tile apply
//   sort       LSD radix, 8-bit digits: count (per-block histograms), exclusive scan of the [digit][block] table, stable scatter
//              (rank within a 256-element chunk from eight ballots per wave).  The host enqueues all CL_MAX_PASSES passes; the number
//              of points and of passes the key needs live on the device (*n_dev, *npasses_dev), and a pass at or above *npasses_dev
//              returns at once, so the host never waits for either.  After the call the sorted pairs are in the b buffers when
//              *npasses_dev is odd, in the a buffers otherwise (SortedPairs::keys / ::idx, or sorted_keys / sorted_idx on separate pointers)
//   workspace  SortLayout places the six arrays of one sort in a caller's workspace (sort_layout), radix_buffers turns the offsets into
//              pointers, sorted_pairs is the read-only view a kernel takes to walk the result.  A caller's own layout states only what
//              it adds around them
// Everything is internal to its translation unit (the anonymous namespace), like the kernels that use it.
#pragma once
#include "lnr_cloud_grid.h"

#define CL_SCAN_PER_THREAD 8
#define CL_SCAN_TILE (CL_BLOCK * CL_SCAN_PER_THREAD)
#define CL_RADIX 256
#define CL_MAX_PASSES 8

namespace {

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

// where the buffers of one sort over a capacity of n pairs lie in a workspace, from `base` up to `end`.  sums also serves the caller's
// own scans (enqueue_scan over flags), so it is sized for the longer of the sort's count table and scan_len, the caller's longest scan
struct SortLayout {
    size_t ka, kb, ia, ib, counts, sums, end;
    uint32_t sort_blocks;
};
SortLayout sort_layout(size_t base, int64_t n, uint64_t scan_len) {
    SortLayout l;
    l.sort_blocks = radix_sort_blocks(n);
    const uint64_t count_len = (uint64_t)CL_RADIX * l.sort_blocks;
    l.ka = align256(base);
    l.kb = align256(l.ka + 8 * (size_t)n);
    l.ia = align256(l.kb + 8 * (size_t)n);
    l.ib = align256(l.ia + 4 * (size_t)n);
    l.counts = align256(l.ib + 4 * (size_t)n);
    l.sums = align256(l.counts + 4 * count_len);
    l.end = align256(l.sums + 4 * ((size_t)scan_tiles(count_len > scan_len ? count_len : scan_len) + 1));
    return l;
}

// n: the pairs this call sorts, where that is fewer than the layout's capacity (its blocks then cover n); default: the capacity
RadixBuffers radix_buffers(char* ws, const SortLayout& l, int64_t n = -1) {
    return RadixBuffers{(uint64_t*)(ws + l.ka), (uint64_t*)(ws + l.kb), (uint32_t*)(ws + l.ia), (uint32_t*)(ws + l.ib),
                        (uint32_t*)(ws + l.counts), (uint32_t*)(ws + l.sums), n < 0 ? l.sort_blocks : radix_sort_blocks(n)};
}

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

// the sorted side of a ping-pong pair, for the kernels that keep the buffers as separate pointer parameters: with the view below the
// compiler indexes the argument block by the pass count (a dependent scalar load), which cost voxel_average, bvh_nodes, ca_gather,
// va_heads and va_emit an instruction or a register (profiles/sort_plumbing_fold.txt)
__device__ inline const uint64_t* sorted_keys(int32_t npasses, const uint64_t* a, const uint64_t* b) { return (npasses & 1) ? b : a; }
__device__ inline const uint32_t* sorted_idx(int32_t npasses, const uint32_t* a, const uint32_t* b) { return (npasses & 1) ? b : a; }

// what the other kernels that walk a sort's output take: both sides of the ping-pong, and the side the pass count on the device selects
struct SortedPairs {
    const uint64_t* __restrict__ ka;
    const uint64_t* __restrict__ kb;
    const uint32_t* __restrict__ ia;
    const uint32_t* __restrict__ ib;
    __device__ inline const uint64_t* keys(int32_t npasses) const { return (npasses & 1) ? kb : ka; }
    __device__ inline const uint32_t* idx(int32_t npasses) const { return (npasses & 1) ? ib : ia; }
};
SortedPairs sorted_pairs(const RadixBuffers& r) { return SortedPairs{r.ka, r.kb, r.ia, r.ib}; }

// bits of v (0 for v <= 0): what a key component that reaches v needs; a key of b bits sorts in (b + 7) / 8 passes
__host__ __device__ inline uint32_t bit_length(int64_t v) { return v <= 0 ? 0u : 64u - (uint32_t)__builtin_clzll((unsigned long long)v); }

}  // namespace
