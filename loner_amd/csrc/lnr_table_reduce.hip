// The end of the density backward: the table-gradient reduce (per-owner LDS reduction of the records and overflow sums the encode
// backward left behind a TableGradSink, lnr_density_api.h) and the fold of the MLP backward's weight-gradient slabs, with their launchers.
#include "lnr_density_api.h"
#include <cstdlib>

// grad[i] += sum over workgroup slabs.  A 64 x 16 workgroup: 64 consecutive parameters, the slabs split over 16 thread rows
// (a thousand threads share the reads instead of one per parameter), rows combined through LDS in a fixed order: no
// atomics, bit-reproducible.
#define LNR_SLAB_GROUPS 16
// the fold of 64 consecutive parameters by one 1024-thread workgroup (`block` = which 64): reduce_slabs_kernel, and the extra workgroups
// at the end of table_grad_reduce2_kernel's grid (one launch fewer per backward: ~4.5 us of a one-keyframe rank's 0.34 ms iteration)
__device__ __forceinline__ void slab_fold_block(const float* __restrict__ slabs, int n_slabs, int n_mlp, float* __restrict__ grad, int overwrite, int block) {
    __shared__ float part[LNR_SLAB_GROUPS][64];
    const int px = threadIdx.x & 63, gy = threadIdx.x >> 6;
    const int i = block * 64 + px;
    const int per = (n_slabs + LNR_SLAB_GROUPS - 1) / LNR_SLAB_GROUPS;
    int b = gy * per;
    const int b_end = min(n_slabs, b + per);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if (i < n_mlp) {
        for (; b + 3 < b_end; b += 4) {
            s0 += slabs[(size_t)b * n_mlp + i]; s1 += slabs[(size_t)(b + 1) * n_mlp + i];
            s2 += slabs[(size_t)(b + 2) * n_mlp + i]; s3 += slabs[(size_t)(b + 3) * n_mlp + i];
        }
        for (; b < b_end; ++b) s0 += slabs[(size_t)b * n_mlp + i];
    }
    part[gy][px] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (gy == 0 && i < n_mlp) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < LNR_SLAB_GROUPS; ++k) s += part[k][px];
        grad[i] = overwrite ? s : grad[i] + s;
    }
}
__global__ void __launch_bounds__(64 * LNR_SLAB_GROUPS)
reduce_slabs_kernel(const float* __restrict__ slabs, int n_slabs, int n_mlp, float* __restrict__ grad, int overwrite) {
    slab_fold_block(slabs, n_slabs, n_mlp, grad, overwrite, (int)blockIdx.x);
}

// Workgroup `o` owns floats [o << shift, (o+1) << shift) of the table gradient.  The encode-backward workgroups of
// level l (bpg of them) wrote the records addressed to it into regions [l][o - first_owner(l)][chunk];
// it streams them, sums them in LDS in 64-bit fixed point (LDS float atomics run at < 1 lane/clk/CU on CDNA4, integer
// ones ~16x faster; 2^-42 resolution, exact and order-independent) and adds the slice to grad_table with coalesced
// read-modify-writes (it is the only writer of that slice).  PAIR: packed pair records (n_features >= 2) or {idx, v}
// records - see lnr_density_api.h.
//
// The kernel is bound by instruction issue and latency, not by bytes (ablations in docs/HISTORY.md 4.3): a region holds ~30-60 records,
// so every wave instruction serves one short region.  Hence the shape of the loop: a wave takes a contiguous run of its owner's
// regions, lane r holds region r's record count, and everything that depends only on the region - its count (v_readlane), its
// address (scalar arithmetic), the trip count - stays on the scalar unit; the first piece (64 x-pair records or 128 8-byte
// records, one load per lane) of RED_U regions is in flight while the previous RED_U are summed; the rare longer regions are
// finished by a second loop.  64 VGPRs, so that two workgroups (2 x 64 KB of accumulators) share a CU.
template <int PAIR>
__device__ __forceinline__ void reduce_one(long long* acc, uint2 r, uint32_t base) {
    if (PAIR) {
        uint32_t pi; float v0, v1;
        lnr_unpack_pair(r, pi, v0, v1);
        // no test for zero: a record exists because one of its values is non-zero, and a branch per value costs more than adding 0
        unsigned long long* a = reinterpret_cast<unsigned long long*>(acc) + 2 * pi;
        if (__builtin_expect(__builtin_fmaxf(__builtin_fabsf(v0), __builtin_fabsf(v1)) < 256.0f, 1)) {
            atomicAdd(a, (unsigned long long)lnr_to_fix_small(v0));
            atomicAdd(a + 1, (unsigned long long)lnr_to_fix_small(v1));
        } else {
            atomicAdd(a, (unsigned long long)lnr_to_fix(v0));
            atomicAdd(a + 1, (unsigned long long)lnr_to_fix(v1));
        }
    } else {
        const float v = __uint_as_float(r.y);
        if (v != 0.0f) atomicAdd(reinterpret_cast<unsigned long long*>(&acc[r.x - base]), (unsigned long long)lnr_to_fix(v));
    }
}
__device__ __forceinline__ void reduce_xpair(long long* acc, const LnrXRec& r) {
    uint32_t pi, t; float a0, a1, fx;
    lnr_unpack_xpair(r, pi, t, a0, a1, fx);
    const uint32_t pj = pi ^ ((2u << t) - 1u);                        // the (x+1) corner's entry: e ^ (2^(t+1) - 1)
    long long q[4];
    lnr_xpair_fix(a0, a1, fx, q);
    unsigned long long* a = reinterpret_cast<unsigned long long*>(acc);
    atomicAdd(a + 2 * pi, (unsigned long long)q[0]);
    atomicAdd(a + 2 * pi + 1, (unsigned long long)q[1]);
    atomicAdd(a + 2 * pj, (unsigned long long)q[2]);
    atomicAdd(a + 2 * pj + 1, (unsigned long long)q[3]);
}

#ifdef LNR_PHASE_TIMING
__device__ unsigned long long lnr_reduce_phase_cycles[LNR_N_PHASES];
#endif
#define RED_SLICE (1 << LNR_SLICE_SHIFT)

// records are read once: streaming (nt) loads
typedef uint32_t red_u32x3 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t red_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ LnrXRec load_xrec_stream(const char* p) {
    const red_u32x3 v = __builtin_nontemporal_load(reinterpret_cast<const red_u32x3*>(p));
    LnrXRec r; r.a = v.x; r.b = v.y; r.c = v.z;
    return r;
}
__device__ __forceinline__ uint4 load_rec2_stream(const uint4* p) {
    const red_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const red_u32x4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// One wave sums the records of n_regions consecutive regions (of one level and owner) into the workgroup's LDS accumulators.
template <int PAIR, int RED_U>
__device__ __forceinline__ void reduce_regions(long long* acc, const int* __restrict__ wave_counts, const char* __restrict__ wave_regions, int n_regions,
                                               uint32_t region_bytes, bool xp, uint32_t base, int lane) {
    for (int r0 = 0; r0 < n_regions; r0 += 64) {
        const int nq = min(64, n_regions - r0);                                                      // regions of this round (wave-uniform)
        const int my_n = lane < nq ? wave_counts[r0 + lane] : 0;
        const char* round_regions = wave_regions + (size_t)r0 * region_bytes;
        if (xp) {
            // x-pair levels (lnr_density_api.h): 12-byte records, a piece = 64 records = one 12-byte load per lane; the first two pieces
            // of a region go through the pipelined loop (an encode-backward workgroup leaves ~65 records per region)
            LnrXRec cur[RED_U][2], nxt[RED_U][2];
            auto loadx = [&](int q0, LnrXRec out[RED_U][2]) {
#pragma unroll
                for (int u = 0; u < RED_U; ++u) {
                    const int q = q0 + u < nq ? q0 + u : nq - 1;                                     // clamp: unconditional loads
                    const int n = __builtin_amdgcn_readlane(my_n, q);
                    const char* rg = round_regions + (size_t)q * region_bytes;
                    out[u][0] = load_xrec_stream(rg + (lane < n ? lane : 0) * 12);
                    out[u][1] = load_xrec_stream(rg + (lane + 64 < n ? lane + 64 : 0) * 12);
                }
            };
            loadx(0, nxt);
            for (int q0 = 0; q0 < nq; q0 += RED_U) {
#pragma unroll
                for (int u = 0; u < RED_U; ++u) { cur[u][0] = nxt[u][0]; cur[u][1] = nxt[u][1]; }
                if (q0 + RED_U < nq) loadx(q0 + RED_U, nxt);
#pragma unroll
                for (int u = 0; u < RED_U; ++u) {
                    const int n = q0 + u < nq ? __builtin_amdgcn_readlane(my_n, q0 + u < 64 ? q0 + u : 63) : 0;
                    if (lane < n) reduce_xpair(acc, cur[u][0]);
                    if (lane + 64 < n) reduce_xpair(acc, cur[u][1]);
                }
            }
            unsigned long long more = __ballot(my_n > 128);                                          // regions with further pieces: rare
            while (more) {
                const int q = __builtin_ctzll(more);
                more &= more - 1ull;
                const int n = __builtin_amdgcn_readlane(my_n, q);
                const char* rg = round_regions + (size_t)q * region_bytes;
                for (int off = 128; off < n; off += 64 * 4) {                                        // four pieces in flight
                    LnrXRec r[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { const int k = off + 64 * u + lane; r[u] = load_xrec_stream(rg + (size_t)(k < n ? k : n - 1) * 12); }
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (off + 64 * u + lane < n) reduce_xpair(acc, r[u]);
                }
            }
            continue;
        }
        // 8-byte records: a piece = 128 records = one 16-byte load (two records) per lane
        uint4 cur[RED_U], nxt[RED_U];
        auto load4 = [&](int q0, uint4 out[RED_U]) {
#pragma unroll
            for (int u = 0; u < RED_U; ++u) {
                const int q = q0 + u < nq ? q0 + u : nq - 1;
                const int n = __builtin_amdgcn_readlane(my_n, q);
                out[u] = load_rec2_stream(reinterpret_cast<const uint4*>(round_regions + (size_t)q * region_bytes) + (2 * lane < n ? lane : 0));   // regions are 16-byte aligned
            }
        };
        load4(0, nxt);
        for (int q0 = 0; q0 < nq; q0 += RED_U) {
#pragma unroll
            for (int u = 0; u < RED_U; ++u) cur[u] = nxt[u];
            if (q0 + RED_U < nq) load4(q0 + RED_U, nxt);
#pragma unroll
            for (int u = 0; u < RED_U; ++u) {
                const int n = q0 + u < nq ? __builtin_amdgcn_readlane(my_n, q0 + u < 64 ? q0 + u : 63) : 0;
                if (2 * lane < n) reduce_one<PAIR>(acc, make_uint2(cur[u].x, cur[u].y), base);
                if (2 * lane + 1 < n) reduce_one<PAIR>(acc, make_uint2(cur[u].z, cur[u].w), base);
            }
        }
        unsigned long long more = __ballot(my_n > 128);
        while (more) {
            const int q = __builtin_ctzll(more);
            more &= more - 1ull;
            const int n = __builtin_amdgcn_readlane(my_n, q);
            const uint2* rg = reinterpret_cast<const uint2*>(round_regions + (size_t)q * region_bytes);
            for (int off = 128; off < n; off += 128 * 4) {                                           // four pieces (of 128 records) in flight
                uint4 r[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int k = off + 128 * u + 2 * lane; r[u] = load_rec2_stream(reinterpret_cast<const uint4*>(rg) + (k < n ? k : 0) / 2); }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = off + 128 * u + 2 * lane;
                    if (k < n) reduce_one<PAIR>(acc, make_uint2(r[u].x, r[u].y), base);
                    if (k + 1 < n) reduce_one<PAIR>(acc, make_uint2(r[u].z, r[u].w), base);
                }
            }
        }
    }
}

// float range of level l, its record-level bookkeeping (shared by the two reduce kernels)
struct RedLevel { uint64_t lo, hi; };
__device__ __forceinline__ RedLevel red_level(const LnrNetSpec& spec, int l) {
    RedLevel r;
    r.lo = (uint64_t)spec.level_offset[l] * spec.n_features;
    r.hi = r.lo + (uint64_t)spec.level_size[l] * spec.n_features;
    return r;
}

// Spatially coherent levels (RegionPlan::split > 1: dense-indexed ones, where an owner slice is a slab of cells and a scan pours most of
// the level's records into two or three of them): `split` workgroups share an owner, each sums a run of the owner's regions in LDS and
// adds its non-zero sums to the level's 64-bit overflow accumulators (integer atomics: exact, order-independent), which the owner's
// workgroup of table_grad_reduce2_kernel folds in afterwards.  Without it those few owners were the whole kernel's critical path
// (0.8 ms for level 1 of the default network against 0.2 ms for everything else).
template <int PAIR, int RED_U, int MINW>
__global__ void __launch_bounds__(1024, MINW)
table_grad_reduce_split_kernel(const LnrNetSpec spec, const void* __restrict__ regions_v, const RegionPlan plan, const int* __restrict__ counts, int bpg,
                               int maxo, long long* __restrict__ ovf) {
    extern __shared__ long long acc[];
    constexpr int slice = RED_SLICE, shift = LNR_SLICE_SHIFT;
    int b = blockIdx.x, l = 0, span = 0;
    int64_t my_ovf = 0;
    RedLevel lv;
    for (;; ++l) {                                                          // the host launched exactly sum(span * split) workgroups
        lv = red_level(spec, l);
        span = (int)(((lv.hi - 1) >> shift) - (lv.lo >> shift)) + 1;
        const int n = plan.split[l] > 1 ? span * plan.split[l] : 0;
        if (b < n) break;
        b -= n;
        my_ovf += (int64_t)(lv.hi - lv.lo);
    }
    const int parts = plan.split[l], local = b / parts, part = b % parts;
    const uint32_t base = ((uint32_t)(lv.lo >> shift) + (uint32_t)local) << shift;
    const uint32_t region_bytes = plan.bytes[l];
    if (region_bytes == 0u) return;
#pragma unroll
    for (int i = threadIdx.x; i < slice; i += 1024) acc[i] = 0ll;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int per_part = (bpg + parts - 1) / parts, part_first = part * per_part, part_n = min(per_part, bpg - part_first);
    const int per_wave = (part_n + 15) / 16, first = part_first + wave * per_wave, n_regions = min(per_wave, part_first + part_n - first);
    if (n_regions > 0)
        reduce_regions<PAIR, RED_U>(acc, counts + ((size_t)l * maxo + local) * bpg + first,
                                    reinterpret_cast<const char*>(regions_v) + plan.off[l] + ((size_t)local * bpg + first) * (size_t)region_bytes, n_regions,
                                    region_bytes, PAIR && plan.xp[l] != 0, base, lane);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < slice / 1024; ++k) {
        const int i = threadIdx.x + k * 1024;
        const uint64_t gi = (uint64_t)base + i;
        const long long q = acc[i];
        if (q != 0ll && gi >= lv.lo && gi < lv.hi) atomicAdd(reinterpret_cast<unsigned long long*>(ovf + my_ovf + (int64_t)(gi - lv.lo)), (unsigned long long)q);
    }
}

template <int PAIR, int RED_U, int MINW>
__global__ void __launch_bounds__(1024, MINW)   // HIP: (max threads, min waves per SIMD)
table_grad_reduce2_kernel(const LnrNetSpec spec, const void* __restrict__ regions_v, const RegionPlan plan, const int* __restrict__ counts, int bpg,
                          int maxo, long long* __restrict__ ovf, const int* __restrict__ ovf_flag, int epoch, float* __restrict__ grad_table,
                          int64_t n_table_floats, int overwrite, const float* __restrict__ slabs, int n_slabs, int n_mlp, float* __restrict__ grad_mlp) {
    extern __shared__ long long acc[];
    // slabs != NULL: the last ceil(n_mlp / 64) workgroups of the grid fold the MLP backward's weight-gradient slabs (slab_fold_block)
    const int slab_blocks = slabs != nullptr ? (n_mlp + 63) / 64 : 0;
    const int owner_blocks = (int)gridDim.x - slab_blocks;
    if ((int)blockIdx.x >= owner_blocks) {                                   // (workgroup-uniform)
        slab_fold_block(slabs, n_slabs, n_mlp, grad_mlp, overwrite, (int)blockIdx.x - owner_blocks);
        return;
    }
    // Owners in DESCENDING table order: the hardware starts workgroups in blockIdx order, the chip holds 512 of the ~900 at a time, and
    // the owners of the fine (x-pair) levels - the heaviest, and with the default network exactly 512 of them - sit at the END of the
    // table: started last they were the kernel's tail behind a half-empty chip; started first they fill it, and the lighter owners of
    // the coarse levels follow.
    const int o = owner_blocks - 1 - (int)blockIdx.x;
    constexpr int slice = RED_SLICE, shift = LNR_SLICE_SHIFT;
    const uint32_t base = (uint32_t)o << shift;
    PHASE_INIT();
#pragma unroll
    for (int i = threadIdx.x; i < slice; i += 1024) acc[i] = 0ll;
    __syncthreads();
    PHASE(0);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int nwaves = 16;
    int64_t ovf_off = 0;                                                   // running offset of the record levels' overflow accumulators
    for (int l = 0; l < spec.n_levels; ++l) {
        const RedLevel lv = red_level(spec, l);
        const uint64_t lo = lv.lo, hi = lv.hi;
        const int64_t my_ovf = ovf_off;
        ovf_off += (int64_t)(hi - lo);                                      // every level has overflow accumulators
        if (hi <= base || lo >= (uint64_t)base + slice) continue;
        // records that did not fit their region were summed into 64-bit accumulators by the encode kernel (and, on split levels, all
        // records by the split kernel): same fixed point, so region records + overflow add up exactly, whatever the (arrival-order
        // dependent) split between the two was.  [r4] The accumulators are ALL ZERO between calls: a kernel that adds to a level's
        // stores the call's epoch in the level's status word, only then are they read here - and put back to zero by this, their only,
        // reader (no 59 MB memset per call, no 59 MB of reads for levels nothing overflowed on; split levels always carry sums)
        if (plan.split[l] > 1 || ovf_flag[l] == epoch) {               // workgroup-uniform
            long long v[slice / 1024];
#pragma unroll
            for (int k = 0; k < slice / 1024; ++k) {
                const uint64_t gi = (uint64_t)base + threadIdx.x + k * 1024;
                v[k] = (gi >= lo && gi < hi) ? ovf[my_ovf + (int64_t)(gi - lo)] : 0ll;
            }
#pragma unroll
            for (int k = 0; k < slice / 1024; ++k) {
                if (v[k] != 0ll) {
                    acc[threadIdx.x + k * 1024] += v[k];
                    ovf[my_ovf + (int64_t)((uint64_t)base + threadIdx.x + k * 1024 - lo)] = 0ll;
                }
            }
            __syncthreads();
            PHASE(1);
        }
        const int local = o - (int)(lo >> shift);
        if (local < 0 || local >= maxo) continue;
        const uint32_t region_bytes = plan.bytes[l];
        if (region_bytes == 0u || plan.split[l] > 1) continue;              // every record of this level overflowed / went through the split kernel
        const int per_wave = (bpg + nwaves - 1) / nwaves;
        const int first = wave * per_wave;
        const int n_regions = min(per_wave, bpg - first);
        if (n_regions > 0)
            reduce_regions<PAIR, RED_U>(acc, counts + ((size_t)l * maxo + local) * bpg + first,
                                        reinterpret_cast<const char*>(regions_v) + plan.off[l] + ((size_t)local * bpg + first) * (size_t)region_bytes, n_regions,
                                        region_bytes, PAIR && plan.xp[l] != 0, base, lane);
        PHASE(3);
    }
    __syncthreads();
    PHASE(5);
    {
        // LNR_BWD_OVERWRITE_GRAD (workgroup-uniform): the slice IS this call's gradient - every float is stored, none is read
        float g[slice / 1024];
#pragma unroll
        for (int k = 0; k < slice / 1024; ++k) {
            const int64_t gi = (int64_t)base + threadIdx.x + k * 1024;
            g[k] = (!overwrite && gi < n_table_floats) ? grad_table[gi] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < slice / 1024; ++k) {
            const int64_t gi = (int64_t)base + threadIdx.x + k * 1024;
            const long long q = acc[threadIdx.x + k * 1024];
            if (gi < n_table_floats && (overwrite || q != 0ll)) grad_table[gi] = g[k] + (float)((double)q * (1.0 / (double)LNR_FIX_SCALE));
        }
    }
    PHASE(6);
    PHASE_FLUSH(lnr_reduce_phase_cycles, 0);
}

// (the callers check the launches: LNR_CHECK_LAUNCH)
void lnr_launch_slab_fold(const SlabFold& f, int overwrite, hipStream_t st) {
    LnrProfScope prof("reduce_slabs", st);
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(lnr_div_up(f.n_mlp, 64)), dim3(64 * LNR_SLAB_GROUPS), 0, st, f.slabs, f.n_slabs, f.n_mlp, f.grad, overwrite);
}

template <int PAIR, int U, int W>
static int launch_reduce_variant(const LnrNetSpec* spec, const TableGradSink& c, int n_owners, int n_split, const SlabFold& f, int overwrite, hipStream_t st) {
    const size_t lds = (size_t)RED_SLICE * sizeof(long long);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(table_grad_reduce2_kernel<PAIR, U, W>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(table_grad_reduce_split_kernel<PAIR, U, W>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        lnr_set_error("lnr_density_backward: hipFuncSetAttribute failed"); return LNR_ERR_LAUNCH;
    }
    if (n_split > 0) {
        LnrProfScope prof("table_grad_reduce_split", st);
        hipLaunchKernelGGL((table_grad_reduce_split_kernel<PAIR, U, W>), dim3(n_split), dim3(1024), lds, st, *spec, c.regions, c.plan, c.counts, c.bpg, c.maxo, c.ovf);
    }
    LnrProfScope prof("table_grad_reduce", st);
    const int slab_blocks = f.slabs != nullptr ? (f.n_mlp + 63) / 64 : 0;
    hipLaunchKernelGGL((table_grad_reduce2_kernel<PAIR, U, W>), dim3(n_owners + slab_blocks), dim3(1024), lds, st, *spec, c.regions, c.plan, c.counts, c.bpg, c.maxo,
                       c.ovf, c.ovf_flag, c.epoch, c.grad_table, spec->n_params - spec->n_mlp_params, overwrite, f.slabs, f.n_slabs, f.n_mlp, f.grad);
    return LNR_OK;
}
// 2 regions in flight per wave at 8 waves per SIMD (two workgroups per CU) measured best: 0.35 ms against 0.37 (4 in flight, 8 waves),
// 0.40 (4, 4 waves) and 0.43 (8, 4 waves) on the bench workload
#ifndef LNR_RED_U
#define LNR_RED_U 2
#endif
#ifndef LNR_RED_W
#define LNR_RED_W 8
#endif
int lnr_launch_table_reduce(const LnrNetSpec* spec, const TableGradSink& sink, int n_owners, int n_split, const SlabFold& fold, int overwrite, hipStream_t st) {
    if (spec->n_features < 2) return launch_reduce_variant<0, LNR_RED_U, LNR_RED_W>(spec, sink, n_owners, n_split, fold, overwrite, st);
    return launch_reduce_variant<1, LNR_RED_U, LNR_RED_W>(spec, sink, n_owners, n_split, fold, overwrite, st);
}

#ifdef LNR_PHASE_TIMING
void lnr_table_reduce_print_phases(hipStream_t st) {
    static const char* names[LNR_N_PHASES] = {"zero LDS", "overflow fold", "-", "records", "-", "final barrier", "write-out"};
    unsigned long long h[LNR_N_PHASES];
    if (getenv("LNR_PHASE_TIMING") && lnr_phase_fetch(HIP_SYMBOL(lnr_reduce_phase_cycles), h, LNR_N_PHASES, st)) lnr_phase_print("table_grad_reduce", names, h);
}
#endif
