// TSDF fusion into a block-sparse volume (gfx950): the dense volume of lnr_tsdf.hip over a lattice of any size, of which only the
// 8 x 8 x 8 blocks a ray wrote to are stored.
//
// Replaces  open3d.pipelines.integration.ScalableTSDFVolume / open3d.t.geometry.VoxelBlockGrid   for range rays, with a definition of
// our own (include/loner_hip.h, "sparse TSDF"): the walk, s and q are the dense volume's (restated in lnr_tsdf_walk.h), the sums are
// integers, and there is no hash table.  The directory is the sorted array of the existing blocks' keys with the slot of each in the pool; a lookup
// is a binary search, a ray keeps its last (key, slot) in registers and searches only when it enters another block.  New blocks get
// their slots in key order behind the old ones, so the pool is a function of the sequence of the calls' ray sets and the volume in
// directory order a function of the set of all rays.
//
// A call is four entry points, because the host reads two counts between them (the pool is the caller's, and grows there):
//   touch      the walk without writing: per ray the number of times it enters a block it writes to that the directory does not hold
//              (count), the exclusive scan of those, and their sum for the host
//   insert     the same walk again for the rays with a count (emit), the shared radix sort of the candidates, the distinct keys and
//              their number for the host
//   merge      (old keys, old slots) and (new keys, B_old + rank) sorted as pairs into the new directory
//   integrate  the walk with the dense kernel's two atomics per written voxel
// In steady state touch finds nothing and insert and merge are not called: two walks per ray.
//
// Marching cubes over blocks: one 256-lane workgroup per block stages the 9^3 apron of field and valid (its own nodes and the lower
// faces of up to seven neighbours, found through a neighbour table built by binary search) in LDS; a node beyond the lattice or in
// a missing block is not valid.  Count, scan and emit as in lnr_mesh.hip, in directory order, with global indices in the vertex formula.
//
// This file is compiled with -ffp-contract=off (build.py EXACT).
#include "lnr_tsdf_walk.h"
#include "lnr_radix_sort.h"

#define TS_NODES 512
#define TS_NONE 0xFFFFFFFFu
#define TS_MAX_AXIS (1 << 21)
#define TS_MAX_BLOCKS (1 << 22)     // 2^31 nodes in the arrays in directory order
#define SMC_APRON 729
#define MC_W LNR_MC_TABLE_WIDTH

__constant__ int8_t c_smc_table[256 * MC_W];
__constant__ uint8_t c_smc_ntri[256];

namespace {

__device__ __forceinline__ uint64_t ts_pack(uint32_t bx, uint32_t by, uint32_t bz) { return ((uint64_t)bx << 36) | ((uint64_t)by << 18) | (uint64_t)bz; }
__device__ __forceinline__ uint64_t ts_key(int32_t i, int32_t j, int32_t k) { return ts_pack((uint32_t)i >> 3, (uint32_t)j >> 3, (uint32_t)k >> 3); }
__device__ __forceinline__ uint32_t ts_local(uint32_t i, uint32_t j, uint32_t k) { return ((i & 7u) << 6) | ((j & 7u) << 3) | (k & 7u); }

// the rank of key in keys[0, n), ascending and unique, or TS_NONE
__device__ __forceinline__ uint32_t ts_find(const uint64_t* __restrict__ keys, uint32_t n, uint64_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && keys[lo] == key ? lo : TS_NONE;
}

// ------------------------------------------------------------------------------------------------ touch and insert
// COUNT (!EMIT): per_ray[ray] = the candidates of the ray, per_ray[n_rays] = 0, *total += their sum.
// EMIT: per_ray holds the exclusive scan; the ray writes its candidates to cand[per_ray[ray] .. per_ray[ray + 1]).
// A ray has a candidate whenever it writes a voxel whose block is not the block of the voxel it wrote before and is not in the directory.
template <bool EMIT>
__global__ __launch_bounds__(TSDF_BLOCK) void ts_touch_kernel(const double* __restrict__ rays, const double* __restrict__ ranges, uint32_t n_rays,
                                                               const TsdfGrid g, const uint64_t* __restrict__ keys, uint32_t n_blocks,
                                                               uint32_t* __restrict__ per_ray, unsigned long long* __restrict__ total,
                                                               uint64_t* __restrict__ cand, uint32_t* __restrict__ cand_ray, uint32_t n_cand) {
    const uint32_t ray = blockIdx.x * TSDF_BLOCK + threadIdx.x;
    uint32_t cnt = 0;
    if (ray < n_rays) {
        uint32_t pos = 0, end = 0;
        if (EMIT) {
            pos = per_ray[ray];
            end = per_ray[ray + 1] < n_cand ? per_ray[ray + 1] : n_cand;
        }
        if (!EMIT || pos < end) {
            uint64_t last = ~0ull;                                   // (no key: a key has 54 bits)
            tsdf_walk(rays, ranges, ray, g, [&](int32_t i, int32_t j, int32_t k, long long) {
                const uint64_t key = ts_key(i, j, k);
                if (key == last) return;
                last = key;
                if (ts_find(keys, n_blocks, key) != TS_NONE) return;
                if (EMIT) {
                    if (pos < end) { cand[pos] = key; cand_ray[pos] = ray; }
                    ++pos;
                } else {
                    ++cnt;
                }
            });
        }
    }
    if (!EMIT) {
        if (ray <= n_rays) per_ray[ray] = cnt;
        unsigned long long u = cnt;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) u += __shfl_xor(u, o, 64);
        if (u && (threadIdx.x & 63) == 0) atomicAdd(total, u);
    }
}

__global__ void ts_sort_params(uint32_t* __restrict__ words, uint32_t n, int32_t npasses) {
    words[0] = n;
    words[1] = (uint32_t)npasses;
}

// flags[i] = 1 at the first of every run of equal sorted keys
__global__ __launch_bounds__(CL_BLOCK) void ts_heads(const uint64_t* __restrict__ sorted, uint32_t n, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i < n) flags[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1u : 0u;
}

// flags: the exclusive scan of the heads; the distinct keys, ascending, go to new_keys and their number to *n_new
__global__ __launch_bounds__(CL_BLOCK) void ts_compact(const uint64_t* __restrict__ sorted, uint32_t n, const uint32_t* __restrict__ flags,
                                                        const uint32_t* __restrict__ n_unique, uint64_t* __restrict__ new_keys,
                                                        unsigned long long* __restrict__ n_new) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i == 0) *n_new = *n_unique;
    if (i < n && (i == 0 || sorted[i] != sorted[i - 1]) && flags[i] < n) new_keys[flags[i]] = sorted[i];
}

// the pairs of the merge: the directory as it is, then the new keys with the slots B_old, B_old + 1, ...
__global__ __launch_bounds__(CL_BLOCK) void ts_merge_fill(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ slot, uint32_t n_old,
                                                           const uint64_t* __restrict__ new_keys, uint32_t n_new, uint64_t* __restrict__ ka,
                                                           uint32_t* __restrict__ ia) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n_old + n_new) return;
    ka[i] = i < n_old ? keys[i] : new_keys[i - n_old];
    ia[i] = i < n_old ? slot[i] : i;
}

__global__ __launch_bounds__(CL_BLOCK) void ts_merge_copy(const uint64_t* __restrict__ ks, const uint32_t* __restrict__ is, uint32_t n,
                                                           uint64_t* __restrict__ keys_out, uint32_t* __restrict__ slot_out) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    keys_out[i] = ks[i];
    slot_out[i] = is[i];
}

// ------------------------------------------------------------------------------------------------ integrate
// info: the call's eight words; [5] and [6] are the host's numbers, [1..4] the dense kernel's tally, [7] the written voxels whose block
// the directory does not hold (or holds with a slot outside the pool): they write nothing
__global__ __launch_bounds__(TSDF_BLOCK) void ts_integrate_kernel(const double* __restrict__ rays, const double* __restrict__ ranges,
                                                                   uint32_t n_rays, const TsdfGrid g, const uint64_t* __restrict__ keys,
                                                                   const uint32_t* __restrict__ slot, uint32_t n_blocks, uint32_t capacity,
                                                                   unsigned long long* __restrict__ sum, uint32_t* __restrict__ count,
                                                                   unsigned long long* __restrict__ info, uint32_t n_new) {
    const uint32_t ray = blockIdx.x * TSDF_BLOCK + threadIdx.x;
    if (ray == 0) {
        info[5] = n_new;
        info[6] = n_blocks;
    }
    int cls = -1;                                               // 0: updated a node, 1: invalid, 2: misses the box, 3: wrote nothing
    uint32_t updates = 0, lost = 0;
    if (ray < n_rays) {
        uint64_t last = ~0ull;
        uint32_t s = TS_NONE;
        cls = tsdf_walk(rays, ranges, ray, g, [&](int32_t i, int32_t j, int32_t k, long long q) {
            const uint64_t key = ts_key(i, j, k);
            if (key != last) {
                last = key;
                const uint32_t rank = ts_find(keys, n_blocks, key);
                s = rank == TS_NONE ? TS_NONE : slot[rank];
                if (s >= capacity) s = TS_NONE;
            }
            if (s == TS_NONE) {
                ++lost;
                return;
            }
            const size_t node = (size_t)s * TS_NODES + ts_local((uint32_t)i, (uint32_t)j, (uint32_t)k);
            atomicAdd(sum + node, (unsigned long long)q);                                            // (two's complement: a signed add)
            atomicAdd(count + node, 1u);
            ++updates;
        });
        if (cls == 0 && !updates) cls = 3;
    }
    tsdf_tally(cls, updates, info + 1);
    unsigned long long u = lost;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) u += __shfl_xor(u, o, 64);
    if (u && (threadIdx.x & 63) == 0) atomicAdd(&info[7], u);
}

__global__ __launch_bounds__(TSDF_BLOCK) void ts_field_kernel(const long long* __restrict__ sum, const uint32_t* __restrict__ count,
                                                               const uint32_t* __restrict__ slot, uint32_t n_blocks, uint32_t capacity,
                                                               uint32_t min_count, float* __restrict__ field, uint8_t* __restrict__ valid) {
    const size_t i = (size_t)blockIdx.x * TSDF_BLOCK + threadIdx.x;
    const uint32_t b = (uint32_t)(i / TS_NODES);
    if (b >= n_blocks) return;
    const uint32_t s = slot[b];
    uint32_t c = 0;
    long long v = 0;
    if (s < capacity) {
        const size_t src = (size_t)s * TS_NODES + (i & (TS_NODES - 1));
        c = count[src];
        v = sum[src];
    }
    field[i] = c > 0 ? (float)(-(double)v / ((double)c * TSDF_ONE)) : 0.0f;
    valid[i] = c >= min_count ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ marching cubes over blocks
struct SmcDims {
    uint32_t n[3];      // nodes per axis
    uint32_t nb[3];     // blocks per axis
};

// nbr[8 b + c]: the directory rank of the block at (bx + (c & 1), by + (c >> 1 & 1), bz + (c >> 2 & 1)), or -1
__global__ __launch_bounds__(CL_BLOCK) void smc_neighbours(const uint64_t* __restrict__ keys, uint32_t n_blocks, const SmcDims d,
                                                            int32_t* __restrict__ nbr) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= 8u * n_blocks) return;
    const uint32_t b = t >> 3, c = t & 7u;
    const uint64_t key = keys[b];
    const uint32_t x = (uint32_t)(key >> 36) + (c & 1u), y = ((uint32_t)(key >> 18) & 0x3FFFFu) + ((c >> 1) & 1u),
                   z = ((uint32_t)key & 0x3FFFFu) + ((c >> 2) & 1u);
    int32_t r = -1;
    if (x < d.nb[0] && y < d.nb[1] && z < d.nb[2]) {
        const uint32_t rank = c == 0 ? b : ts_find(keys, n_blocks, ts_pack(x, y, z));
        if (rank != TS_NONE) r = (int32_t)rank;
    }
    nbr[t] = r;
}

// the apron of block b in LDS: f and ok [9][9][9] over the block's nodes and the first layer of its upper neighbours.  A node of a
// missing block or beyond the lattice is not valid (and reads as 0)
__device__ __forceinline__ void smc_stage(uint32_t b, const uint64_t* __restrict__ keys, const int32_t* __restrict__ nbr,
                                          const float* __restrict__ field, const uint8_t* __restrict__ valid, const SmcDims& d, float* f,
                                          uint8_t* ok, int32_t* nb, uint32_t* g0) {
    if (threadIdx.x < 8) nb[threadIdx.x] = nbr[8 * (size_t)b + threadIdx.x];
    if (threadIdx.x == 8) {
        const uint64_t key = keys[b];
        g0[0] = (uint32_t)(key >> 36) << 3;
        g0[1] = ((uint32_t)(key >> 18) & 0x3FFFFu) << 3;
        g0[2] = ((uint32_t)key & 0x3FFFFu) << 3;
    }
    __syncthreads();
    for (uint32_t a = threadIdx.x; a < SMC_APRON; a += CL_BLOCK) {
        const uint32_t x = a / 81u, y = (a / 9u) % 9u, z = a % 9u;
        const int32_t r = nb[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
        bool v = r >= 0 && g0[0] + x < d.n[0] && g0[1] + y < d.n[1] && g0[2] + z < d.n[2];
        float val = 0.0f;
        if (v) {
            const size_t src = (size_t)r * TS_NODES + ts_local(x, y, z);
            v = valid[src] != 0;
            val = field[src];
        }
        f[a] = val;
        ok[a] = v ? 1 : 0;
    }
    __syncthreads();
}

__device__ __forceinline__ uint32_t smc_apron_index(uint32_t l) { return (l >> 6) * 81u + ((l >> 3) & 7u) * 9u + (l & 7u); }

// bits 0..2: the node's +x / +y / +z edge has two valid ends on different sides of the level
__device__ __forceinline__ uint32_t smc_edge_bits(const float* f, const uint8_t* ok, uint32_t a, float level) {
    if (!ok[a]) return 0;
    const bool in = f[a] > level;
    uint32_t bits = 0;
    if (ok[a + 81] && (f[a + 81] > level) != in) bits |= 1u;
    if (ok[a + 9] && (f[a + 9] > level) != in) bits |= 2u;
    if (ok[a + 1] && (f[a + 1] > level) != in) bits |= 4u;
    return bits;
}

// the case of the cell whose lower node this is; 0 for a cell with a corner that is not valid (which covers the lattice's upper faces)
__device__ __forceinline__ uint32_t smc_case(const float* f, const uint8_t* ok, uint32_t a, float level) {
    uint32_t cas = 0;
    bool all = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t n = a + ((c & 1) ? 81u : 0u) + ((c & 2) ? 9u : 0u) + ((c & 4) ? 1u : 0u);
        cas |= (f[n] > level ? 1u : 0u) << c;
        all = all && ok[n];
    }
    return all ? cas : 0;
}

#define SMC_SHARED                              \
    __shared__ float f[SMC_APRON];              \
    __shared__ uint8_t ok[SMC_APRON + 3];       \
    __shared__ int32_t nb[8];                   \
    __shared__ uint32_t g0[4];                  \
    __shared__ uint32_t lds[CL_BLOCK / 64]

// one workgroup per block, two consecutive nodes per lane
__global__ __launch_bounds__(CL_BLOCK) void smc_count_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ nbr,
                                                              const float* __restrict__ field, const uint8_t* __restrict__ valid,
                                                              const SmcDims d, float level, uint32_t* __restrict__ block_counts) {
    SMC_SHARED;
    const uint32_t b = blockIdx.x;
    smc_stage(b, keys, nbr, field, valid, d, f, ok, nb, g0);
    uint32_t nv = 0, nt = 0;
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
        const uint32_t a = smc_apron_index(2 * threadIdx.x + h);
        nv += __popc(smc_edge_bits(f, ok, a, level));
        nt += c_smc_ntri[smc_case(f, ok, a, level)];
    }
    uint32_t tv, tt;
    block_exclusive_scan(nv, lds, &tv);
    block_exclusive_scan(nt, lds, &tt);
    if (threadIdx.x == 0) {
        block_counts[2 * (size_t)b] = tv;
        block_counts[2 * (size_t)b + 1] = tt;
    }
}

// exclusive scan of the block counts (two interleaved columns) in one workgroup, chunk after chunk with a running carry
__global__ __launch_bounds__(CL_BLOCK) void smc_scan_kernel(const uint32_t* __restrict__ block_counts, uint32_t n_blocks,
                                                             uint64_t* __restrict__ block_offsets, unsigned long long* __restrict__ totals) {
    __shared__ uint32_t lds[CL_BLOCK / 64];
    uint64_t carry0 = 0, carry1 = 0;
    for (uint32_t c0 = 0; c0 < n_blocks; c0 += CL_BLOCK) {
        const uint32_t b = c0 + threadIdx.x;
        const uint32_t v0 = b < n_blocks ? block_counts[2 * (size_t)b] : 0u, v1 = b < n_blocks ? block_counts[2 * (size_t)b + 1] : 0u;
        uint32_t t0, t1;
        const uint32_t e0 = block_exclusive_scan(v0, lds, &t0);
        const uint32_t e1 = block_exclusive_scan(v1, lds, &t1);
        if (b < n_blocks) {
            block_offsets[2 * (size_t)b] = carry0 + e0;
            block_offsets[2 * (size_t)b + 1] = carry1 + e1;
        }
        carry0 += t0;
        carry1 += t1;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry0;
        totals[1] = carry1;
    }
}

// packed [B][512]: the first vertex id of the node in bits 2.., its x- and y-edge bits in bits 0 and 1 (as lnr_mesh.hip packs them)
__global__ __launch_bounds__(CL_BLOCK) void smc_vertex_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ nbr,
                                                               const float* __restrict__ field, const uint8_t* __restrict__ valid,
                                                               const SmcDims d, float level, const uint64_t* __restrict__ block_offsets,
                                                               float sx, float sy, float sz, float ox, float oy, float oz,
                                                               uint32_t* __restrict__ packed, float* __restrict__ verts, uint64_t n_verts) {
    SMC_SHARED;
    const uint32_t b = blockIdx.x;
    smc_stage(b, keys, nbr, field, valid, d, f, ok, nb, g0);
    uint32_t bits[2];
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) bits[h] = smc_edge_bits(f, ok, smc_apron_index(2 * threadIdx.x + h), level);
    uint32_t total;
    const uint32_t pre = block_exclusive_scan(__popc(bits[0]) + __popc(bits[1]), lds, &total);
    uint64_t id = block_offsets[2 * (size_t)b] + pre;
    const float sp[3] = {sx, sy, sz}, org[3] = {ox, oy, oz};
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
        const uint32_t l = 2 * threadIdx.x + h, a = smc_apron_index(l);
        if (bits[h] && id + __popc(bits[h]) <= n_verts) {                 // (always: the count pass saw the same bits)
            packed[(size_t)b * TS_NODES + l] = ((uint32_t)id << 2) | (bits[h] & 3u);
            const uint32_t ijk[3] = {g0[0] + (l >> 6), g0[1] + ((l >> 3) & 7u), g0[2] + (l & 7u)};
            const uint32_t stride[3] = {81u, 9u, 1u};
            const float va = f[a];
            uint64_t vid = id;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (!((bits[h] >> ax) & 1u)) continue;
                const float vb = f[a + stride[ax]];
                const float tt = __fdiv_rn(level - va, vb - va);
                float* o = verts + 3 * (size_t)vid;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float c = q == ax ? lnr_add_rn((float)ijk[q], tt) : (float)ijk[q];
                    o[q] = lnr_add_rn(lnr_mul_rn(c, sp[q]), org[q]);
                }
                ++vid;
            }
        }
        id += __popc(bits[h]);
    }
}

__global__ __launch_bounds__(CL_BLOCK) void smc_triangle_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ nbr,
                                                                 const float* __restrict__ field, const uint8_t* __restrict__ valid,
                                                                 const SmcDims d, float level, const uint64_t* __restrict__ block_offsets,
                                                                 const uint32_t* __restrict__ packed, int32_t* __restrict__ tris,
                                                                 uint64_t n_tris) {
    SMC_SHARED;
    const uint32_t b = blockIdx.x;
    smc_stage(b, keys, nbr, field, valid, d, f, ok, nb, g0);
    uint32_t cas[2];
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) cas[h] = smc_case(f, ok, smc_apron_index(2 * threadIdx.x + h), level);
    uint32_t total;
    const uint32_t pre = block_exclusive_scan((uint32_t)c_smc_ntri[cas[0]] + c_smc_ntri[cas[1]], lds, &total);
    uint64_t slot = block_offsets[2 * (size_t)b + 1] + pre;
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
        const uint32_t l = 2 * threadIdx.x + h;
        const uint32_t lx = l >> 6, ly = (l >> 3) & 7u, lz = l & 7u;
        const uint32_t nt = c_smc_ntri[cas[h]];
        for (uint32_t q = 0; q < nt && slot + q < n_tris; ++q) {          // (always: the count pass saw the same cases)
            int32_t* o = tris + 3 * (size_t)(slot + q);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int e = c_smc_table[cas[h] * MC_W + 3 * q + m];
                const int ax = e >> 2, qq = e & 3;
                const int o0 = ax == 0 ? 1 : 0, o1 = ax == 2 ? 1 : 2;
                const int c = ((qq & 1) << o0) | (((qq >> 1) & 1) << o1);
                // the edge's owner: the corner c of the cell, a node of this block or of a neighbour (which exists: the corner is valid)
                const uint32_t x = lx + (c & 1), y = ly + ((c >> 1) & 1), z = lz + ((c >> 2) & 1);
                const int32_t r = nb[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
                const uint32_t w = r >= 0 ? packed[(size_t)r * TS_NODES + ts_local(x, y, z)] : 0u;
                o[m] = (int32_t)((w >> 2) + (ax >= 1 ? (w & 1u) : 0u) + (ax == 2 ? ((w >> 1) & 1u) : 0u));
            }
        }
        slot += nt;
    }
}

// ------------------------------------------------------------------------------------------------ host
int ts_check_dims(int32_t nx, int32_t ny, int32_t nz, const char* fn) {
    LNR_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: every axis needs at least two nodes (%d x %d x %d)", fn, nx, ny, nz);
    LNR_REQUIRE(nx <= TS_MAX_AXIS && ny <= TS_MAX_AXIS && nz <= TS_MAX_AXIS, "%s: %d x %d x %d nodes, the limit is 2^21 per axis", fn, nx, ny, nz);
    return LNR_OK;
}

// digit passes that sort the keys of a lattice: 18 bits per axis below the highest axis with more than one block
int32_t ts_npasses(int32_t nx, int32_t ny, int32_t nz) {
    const uint32_t bx = bit_length((nx - 1) >> 3), by = bit_length((ny - 1) >> 3), bz = bit_length((nz - 1) >> 3);
    const uint32_t bits = bx ? 36 + bx : (by ? 18 + by : bz);
    return (int32_t)((bits + 7) / 8 > 0 ? (bits + 7) / 8 : 1);
}

// touch: the scan's tile sums.  insert and merge: the flags, the distinct keys, three words {n, passes, distinct} and the sort
struct TsLayout {
    size_t flags, new_keys, words, total;
    SortLayout sort;
};
TsLayout ts_layout(int64_t n_sort) {
    TsLayout l;
    l.flags = 0;
    l.new_keys = align256(4 * (size_t)n_sort);
    l.words = align256(l.new_keys + 8 * (size_t)n_sort);
    l.sort = sort_layout(l.words + 256, n_sort, (uint64_t)n_sort);
    l.total = l.sort.end;
    return l;
}
size_t ts_touch_bytes(int64_t n_rays) { return align256(4 * ((size_t)scan_tiles((uint64_t)n_rays + 1) + 1)); }

bool ts_rays_ok(int64_t n_rays) { return n_rays >= 0 && n_rays < ((int64_t)1 << 32) - TSDF_BLOCK; }

uint32_t ts_ray_blocks(int64_t n) { return (uint32_t)((n + TSDF_BLOCK - 1) / TSDF_BLOCK); }

struct SmcTable {
    int8_t t[256 * MC_W];
    uint8_t ntri[256];
    bool ok;
    SmcTable() {
        ok = lnr_mc_case_table(t) == LNR_OK;
        for (int c = 0; c < 256; ++c) {
            int n = 0;
            while (ok && n < MC_W && t[c * MC_W + n] >= 0) ++n;
            ntri[c] = (uint8_t)(n / 3);
        }
    }
};
const SmcTable& smc_table() {
    static const SmcTable tab;
    return tab;
}

struct SmcLayout {
    size_t nbr, counts, offsets, packed, total;
};
SmcLayout smc_layout(int64_t n_blocks) {
    SmcLayout l;
    l.nbr = 0;
    l.counts = align256(4 * 8 * (size_t)n_blocks);
    l.offsets = align256(l.counts + 2 * sizeof(uint32_t) * (size_t)n_blocks);
    l.packed = align256(l.offsets + 2 * sizeof(uint64_t) * (size_t)n_blocks);
    l.total = align256(l.packed + sizeof(uint32_t) * TS_NODES * (size_t)n_blocks);
    return l;
}
SmcDims smc_dims(int32_t nx, int32_t ny, int32_t nz) {
    SmcDims d;
    d.n[0] = (uint32_t)nx; d.n[1] = (uint32_t)ny; d.n[2] = (uint32_t)nz;
    for (int a = 0; a < 3; ++a) d.nb[a] = (d.n[a] + 7u) >> 3;
    return d;
}
int smc_check(const char* fn, const void* keys, int64_t n_blocks, const void* field, const void* valid, int32_t nx, int32_t ny, int32_t nz,
              const void* workspace, size_t workspace_bytes) {
    if (int rc = ts_check_dims(nx, ny, nz, fn)) return rc;
    LNR_REQUIRE(n_blocks >= 1 && n_blocks < TS_MAX_BLOCKS, "%s: %lld blocks, 1 to 2^22 - 1 can be meshed", fn, (long long)n_blocks);
    LNR_REQUIRE(keys && field && valid && workspace, "%s: null argument", fn);
    LNR_REQUIRE(workspace_bytes >= smc_layout(n_blocks).total, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes,
                smc_layout(n_blocks).total);
    return LNR_OK;
}

}  // namespace

extern "C" size_t lnr_tsdf_sparse_workspace(int64_t n_rays, int64_t n_sort) {
    if (!ts_rays_ok(n_rays) || !count_ok(n_sort)) return 0;
    const size_t touch = ts_touch_bytes(n_rays), sort = n_sort > 0 ? ts_layout(n_sort).total : 0;
    return touch > sort ? touch : sort;
}

extern "C" int lnr_tsdf_sparse_touch(const double* rays, const double* ranges, int64_t n_rays, int32_t nx, int32_t ny, int32_t nz,
                                     const double* origin, double voxel_size, double trunc, double front, const uint64_t* keys,
                                     int64_t n_blocks, uint32_t* ray_offsets, void* workspace, size_t workspace_bytes, int64_t* counts_dev,
                                     void* stream) {
    const char* fn = "lnr_tsdf_sparse_touch";
    if (int rc = ts_check_dims(nx, ny, nz, fn)) return rc;
    LNR_REQUIRE(ts_rays_ok(n_rays), "%s: %lld rays, the limit is 2^32 - %d", fn, (long long)n_rays, TSDF_BLOCK + 1);
    CL_REQUIRE_COUNT("lnr_tsdf_sparse_touch", n_blocks, "blocks");
    LNR_REQUIRE(ray_offsets && workspace && counts_dev && (n_rays == 0 || (rays && ranges)) && (n_blocks == 0 || keys), "%s: null argument", fn);
    if (int rc = tsdf_check_params(fn, origin, voxel_size, trunc, front)) return rc;
    LNR_REQUIRE(workspace_bytes >= ts_touch_bytes(n_rays), "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, ts_touch_bytes(n_rays));
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("tsdf_sparse_touch", st);
    if (int rc = clear_words(counts_dev, 2 * sizeof(int64_t), st, fn, "counts")) return rc;
    const TsdfGrid g = tsdf_grid(nx, ny, nz, origin, voxel_size, trunc, front);
    hipLaunchKernelGGL(ts_touch_kernel<false>, dim3(ts_ray_blocks(n_rays + 1)), dim3(TSDF_BLOCK), 0, st, rays, ranges, (uint32_t)n_rays, g, keys,
                       (uint32_t)n_blocks, ray_offsets, (unsigned long long*)counts_dev, (uint64_t*)nullptr, (uint32_t*)nullptr, 0u);
    enqueue_scan(ray_offsets, (uint32_t)(n_rays + 1), (uint32_t*)workspace, nullptr, nullptr, 0, st);
    LNR_CHECK_LAUNCH(fn);
    return LNR_OK;
}

extern "C" int lnr_tsdf_sparse_insert(const double* rays, const double* ranges, int64_t n_rays, int32_t nx, int32_t ny, int32_t nz,
                                      const double* origin, double voxel_size, double trunc, double front, const uint64_t* keys,
                                      int64_t n_blocks, const uint32_t* ray_offsets, int64_t n_candidates, void* workspace,
                                      size_t workspace_bytes, int64_t* counts_dev, void* stream) {
    const char* fn = "lnr_tsdf_sparse_insert";
    if (int rc = ts_check_dims(nx, ny, nz, fn)) return rc;
    LNR_REQUIRE(ts_rays_ok(n_rays) && n_rays > 0, "%s: %lld rays, 1 to 2^32 - %d", fn, (long long)n_rays, TSDF_BLOCK + 1);
    CL_REQUIRE_COUNT("lnr_tsdf_sparse_insert", n_blocks, "blocks");
    CL_REQUIRE_COUNT("lnr_tsdf_sparse_insert", n_blocks + n_candidates, "blocks and candidates");
    LNR_REQUIRE(n_candidates >= 1, "%s: %lld candidates, at least one", fn, (long long)n_candidates);
    LNR_REQUIRE(rays && ranges && ray_offsets && workspace && counts_dev && (n_blocks == 0 || keys), "%s: null argument", fn);
    if (int rc = tsdf_check_params(fn, origin, voxel_size, trunc, front)) return rc;
    const int64_t n_sort = n_blocks + n_candidates;
    const TsLayout l = ts_layout(n_sort);
    LNR_REQUIRE(workspace_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("tsdf_sparse_insert", st);
    char* ws = (char*)workspace;
    uint32_t* words = (uint32_t*)(ws + l.words);
    uint32_t* flags = (uint32_t*)(ws + l.flags);
    const RadixBuffers r = radix_buffers(ws, l.sort, n_candidates);
    const int32_t npasses = ts_npasses(nx, ny, nz);
    const uint32_t n = (uint32_t)n_candidates;
    hipLaunchKernelGGL(ts_sort_params, dim3(1), dim3(1), 0, st, words, n, npasses);
    const TsdfGrid g = tsdf_grid(nx, ny, nz, origin, voxel_size, trunc, front);
    hipLaunchKernelGGL(ts_touch_kernel<true>, dim3(ts_ray_blocks(n_rays)), dim3(TSDF_BLOCK), 0, st, rays, ranges, (uint32_t)n_rays, g, keys,
                       (uint32_t)n_blocks, (uint32_t*)ray_offsets, (unsigned long long*)nullptr, r.ka, r.ia, n);
    enqueue_radix_sort(r, words, (const int32_t*)(words + 1), st);
    const uint64_t* sorted = (npasses & 1) ? r.kb : r.ka;
    hipLaunchKernelGGL(ts_heads, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, sorted, n, flags);
    enqueue_scan(flags, n, r.sums, words + 2, nullptr, 0, st);
    hipLaunchKernelGGL(ts_compact, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, sorted, n, (const uint32_t*)flags, (const uint32_t*)(words + 2),
                       (uint64_t*)(ws + l.new_keys), (unsigned long long*)(counts_dev + 1));
    LNR_CHECK_LAUNCH(fn);
    return LNR_OK;
}

extern "C" int lnr_tsdf_sparse_merge(const uint64_t* keys, const uint32_t* slot, int64_t n_blocks, int64_t n_new, int64_t n_candidates,
                                     int32_t nx, int32_t ny, int32_t nz, void* workspace, size_t workspace_bytes, uint64_t* keys_out,
                                     uint32_t* slot_out, void* stream) {
    const char* fn = "lnr_tsdf_sparse_merge";
    if (int rc = ts_check_dims(nx, ny, nz, fn)) return rc;
    CL_REQUIRE_COUNT("lnr_tsdf_sparse_merge", n_blocks, "blocks");
    CL_REQUIRE_COUNT("lnr_tsdf_sparse_merge", n_blocks + n_candidates, "blocks and candidates");
    LNR_REQUIRE(n_new >= 1 && n_new <= n_candidates, "%s: %lld new blocks of %lld candidates", fn, (long long)n_new, (long long)n_candidates);
    LNR_REQUIRE(workspace && keys_out && slot_out && (n_blocks == 0 || (keys && slot)), "%s: null argument", fn);
    const TsLayout l = ts_layout(n_blocks + n_candidates);
    LNR_REQUIRE(workspace_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("tsdf_sparse_merge", st);
    char* ws = (char*)workspace;
    uint32_t* words = (uint32_t*)(ws + l.words);
    const uint32_t n = (uint32_t)(n_blocks + n_new);
    const RadixBuffers r = radix_buffers(ws, l.sort, n);
    const int32_t npasses = ts_npasses(nx, ny, nz);
    hipLaunchKernelGGL(ts_sort_params, dim3(1), dim3(1), 0, st, words, n, npasses);
    hipLaunchKernelGGL(ts_merge_fill, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, keys, slot, (uint32_t)n_blocks,
                       (const uint64_t*)(ws + l.new_keys), (uint32_t)n_new, r.ka, r.ia);
    enqueue_radix_sort(r, words, (const int32_t*)(words + 1), st);
    hipLaunchKernelGGL(ts_merge_copy, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, (const uint64_t*)((npasses & 1) ? r.kb : r.ka),
                       (const uint32_t*)((npasses & 1) ? r.ib : r.ia), n, keys_out, slot_out);
    LNR_CHECK_LAUNCH(fn);
    return LNR_OK;
}

extern "C" int lnr_tsdf_sparse_integrate(const double* rays, const double* ranges, int64_t n_rays, int32_t nx, int32_t ny, int32_t nz,
                                         const double* origin, double voxel_size, double trunc, double front, const uint64_t* keys,
                                         const uint32_t* slot, int64_t n_blocks, int64_t n_new, int64_t capacity, int64_t* sum, uint32_t* count,
                                         int64_t* info_dev, void* stream) {
    const char* fn = "lnr_tsdf_sparse_integrate";
    if (int rc = ts_check_dims(nx, ny, nz, fn)) return rc;
    LNR_REQUIRE(ts_rays_ok(n_rays), "%s: %lld rays, the limit is 2^32 - %d", fn, (long long)n_rays, TSDF_BLOCK + 1);
    CL_REQUIRE_COUNT("lnr_tsdf_sparse_integrate", n_blocks, "blocks");
    LNR_REQUIRE(n_new >= 0 && n_new <= n_blocks && n_blocks <= capacity && capacity < ((int64_t)1 << 32) - 1,
                "%s: %lld new of %lld blocks in a pool of %lld", fn, (long long)n_new, (long long)n_blocks, (long long)capacity);
    LNR_REQUIRE(info_dev && (n_rays == 0 || (rays && ranges)) && (n_blocks == 0 || (keys && slot && sum && count)), "%s: null argument", fn);
    if (int rc = tsdf_check_params(fn, origin, voxel_size, trunc, front)) return rc;
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("tsdf_sparse_integrate", st);
    if (int rc = clear_words(info_dev, 8 * sizeof(int64_t), st, fn, "info words")) return rc;
    const TsdfGrid g = tsdf_grid(nx, ny, nz, origin, voxel_size, trunc, front);
    hipLaunchKernelGGL(ts_integrate_kernel, dim3(ts_ray_blocks(n_rays > 0 ? n_rays : 1)), dim3(TSDF_BLOCK), 0, st, rays, ranges, (uint32_t)n_rays,
                       g, keys, slot, (uint32_t)n_blocks, (uint32_t)capacity, (unsigned long long*)sum, count, (unsigned long long*)info_dev,
                       (uint32_t)n_new);
    LNR_CHECK_LAUNCH(fn);
    return LNR_OK;
}

extern "C" int lnr_tsdf_sparse_field(const int64_t* sum, const uint32_t* count, const uint32_t* slot, int64_t n_blocks, int64_t capacity,
                                     uint32_t min_count, float* field, uint8_t* valid, void* stream) {
    const char* fn = "lnr_tsdf_sparse_field";
    LNR_REQUIRE(n_blocks >= 1 && n_blocks < TS_MAX_BLOCKS && n_blocks <= capacity && capacity < ((int64_t)1 << 32) - 1,
                "%s: %lld blocks in a pool of %lld; 1 to 2^22 - 1 blocks can be read", fn, (long long)n_blocks, (long long)capacity);
    LNR_REQUIRE(sum && count && slot && field && valid, "%s: null argument", fn);
    LNR_REQUIRE(min_count >= 1, "%s: min_count must be at least 1", fn);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("tsdf_sparse_field", st);
    hipLaunchKernelGGL(ts_field_kernel, dim3((uint32_t)(n_blocks * (TS_NODES / TSDF_BLOCK))), dim3(TSDF_BLOCK), 0, st, (const long long*)sum, count,
                       slot, (uint32_t)n_blocks, (uint32_t)capacity, min_count, field, valid);
    LNR_CHECK_LAUNCH(fn);
    return LNR_OK;
}

extern "C" size_t lnr_mc_sparse_workspace(int64_t n_blocks) {
    if (n_blocks < 1 || n_blocks >= TS_MAX_BLOCKS) return 0;
    return smc_layout(n_blocks).total;
}

extern "C" int lnr_mc_sparse_count(const uint64_t* keys, int64_t n_blocks, const float* field, const uint8_t* valid, int32_t nx, int32_t ny,
                                   int32_t nz, float level, void* workspace, size_t workspace_bytes, uint64_t* totals_dev, void* stream) {
    const char* fn = "lnr_mc_sparse_count";
    if (int rc = smc_check(fn, keys, n_blocks, field, valid, nx, ny, nz, workspace, workspace_bytes)) return rc;
    LNR_REQUIRE(totals_dev != nullptr, "%s: null argument", fn);
    const SmcTable& tab = smc_table();
    LNR_REQUIRE(tab.ok, "%s: no case table", fn);
    hipStream_t st = (hipStream_t)stream;
    // the table goes to constant memory of the current device with every call, as in lnr_mc_count
    if (hipMemcpyToSymbolAsync(HIP_SYMBOL(c_smc_table), tab.t, sizeof(tab.t), 0, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyToSymbolAsync(HIP_SYMBOL(c_smc_ntri), tab.ntri, sizeof(tab.ntri), 0, hipMemcpyHostToDevice, st) != hipSuccess) {
        lnr_set_error("%s: upload of the case table failed", fn);
        return LNR_ERR_LAUNCH;
    }
    const SmcLayout l = smc_layout(n_blocks);
    char* ws = (char*)workspace;
    const SmcDims d = smc_dims(nx, ny, nz);
    const uint32_t B = (uint32_t)n_blocks;
    LnrProfScope prof("mc_sparse_count", st);
    hipLaunchKernelGGL(smc_neighbours, dim3(blocks_for(8ull * B)), dim3(CL_BLOCK), 0, st, keys, B, d, (int32_t*)(ws + l.nbr));
    hipLaunchKernelGGL(smc_count_kernel, dim3(B), dim3(CL_BLOCK), 0, st, keys, (const int32_t*)(ws + l.nbr), field, valid, d, level,
                       (uint32_t*)(ws + l.counts));
    hipLaunchKernelGGL(smc_scan_kernel, dim3(1), dim3(CL_BLOCK), 0, st, (const uint32_t*)(ws + l.counts), B, (uint64_t*)(ws + l.offsets),
                       (unsigned long long*)totals_dev);
    LNR_CHECK_LAUNCH(fn);
    return LNR_OK;
}

extern "C" int lnr_mc_sparse_emit(const uint64_t* keys, int64_t n_blocks, const float* field, const uint8_t* valid, int32_t nx, int32_t ny,
                                  int32_t nz, float level, const float* spacing, const float* origin, void* workspace, size_t workspace_bytes,
                                  int64_t n_verts, int64_t n_tris, float* verts, int32_t* tris, void* stream) {
    const char* fn = "lnr_mc_sparse_emit";
    if (int rc = smc_check(fn, keys, n_blocks, field, valid, nx, ny, nz, workspace, workspace_bytes)) return rc;
    LNR_REQUIRE(spacing && origin, "%s: null argument", fn);
    LNR_REQUIRE(n_verts >= 0 && n_verts < ((int64_t)1 << 30), "%s: %lld vertices, the limit is 2^30 - 1", fn, (long long)n_verts);
    LNR_REQUIRE(n_tris >= 0 && (n_verts == 0 || (verts && (tris || n_tris == 0))), "%s: bad outputs", fn);
    if (n_verts == 0) return LNR_OK;
    hipStream_t st = (hipStream_t)stream;
    const SmcLayout l = smc_layout(n_blocks);
    char* ws = (char*)workspace;
    const SmcDims d = smc_dims(nx, ny, nz);
    const uint32_t B = (uint32_t)n_blocks;
    LnrProfScope prof("mc_sparse_emit", st);
    hipLaunchKernelGGL(smc_vertex_kernel, dim3(B), dim3(CL_BLOCK), 0, st, keys, (const int32_t*)(ws + l.nbr), field, valid, d, level,
                       (const uint64_t*)(ws + l.offsets), spacing[0], spacing[1], spacing[2], origin[0], origin[1], origin[2],
                       (uint32_t*)(ws + l.packed), verts, (uint64_t)n_verts);
    if (n_tris > 0)
        hipLaunchKernelGGL(smc_triangle_kernel, dim3(B), dim3(CL_BLOCK), 0, st, keys, (const int32_t*)(ws + l.nbr), field, valid, d, level,
                           (const uint64_t*)(ws + l.offsets), (const uint32_t*)(ws + l.packed), tris, (uint64_t)n_tris);
    LNR_CHECK_LAUNCH(fn);
    return LNR_OK;
}
