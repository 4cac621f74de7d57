// Scan ingestion (gfx950): a raw point array becomes the time-ordered LidarScan the tracker and the mapper take.
//
// Replaces the host passes of examples/run_loner.py:59-157 (build_scan_from_msg: FOV mask, range filter, norms, the timestamp
// heuristics, the sort) with the definition stated in include/loner_hip.h ("scan ingestion").  This file is compiled with
// -ffp-contract=off (build.py EXACT): every fp32 expression below rounds operation by operation as torch's CPU ops do, the one fused
// operation is the explicit fmaf of the norm, and the divide and the square root are IEEE (no fast-math).
//
// One stream, no host wait:
//   flag       per point: FOV and range tests -> keep word; over the kept points the first and last index, max |t| and a count of
//              non-finite times (one atomic per wave and quantity)
//   scan       exclusive scan of the keep words (lnr_radix_sort.h): the rank of every kept point, and M
//   params     one thread: the branches of the timestamp heuristics from t[first], t[last] and max |t|, the flag bits, and the number of
//              digit passes the key needs (0 when every time is the stamp)
//   keys       per kept point: key = image(t) << 8 d | rank, d = the 8-bit digits of M - 1; image is the order-preserving 32-bit
//              picture of the fp32 time.  This orders exactly as (image << 32 | rank) does and leaves no dead digit between the
//              halves, so the sort's pass guard (a pass count) skips every digit the key does not use.  The payload is the ORIGINAL index
//   sort       the stable LSD radix sort of lnr_radix_sort.h, shared with lnr_cloud.hip
//   gather     per output point: coordinates and time re-read through the original index; direction = xyz / dist, the final time, the
//              index as int64; a count of adjacent output pairs out of order (0 by construction: the caller's sortedness check)
//   info       the status words for the one host read
#include "lnr_radix_sort.h"

namespace {

struct FovSegments {
    int32_t enabled, n;
    float lo[LNR_SCAN_MAX_FOV_SEGMENTS], hi[LNR_SCAN_MAX_FOV_SEGMENTS];
};

// the call's parameters, on the device.  Cleared by the call; first_inv holds max(~i) so that 0 is its neutral element
struct ScanParams {
    uint32_t m;                     // kept points (the scan's total)
    int32_t npasses;                // digit passes of the sort
    uint32_t first_inv, last;       // ~(first kept index), last kept index
    uint32_t maxabs_bits;           // bits of max |t| over the kept points with a finite time
    uint32_t flags;                 // LNR_SCAN_*
    uint32_t nonfinite, unsorted;
    uint32_t key_shift;             // 8 * digits of m - 1
    float sub_neg, sub_global;      // t[first] at the negative-start and at the global-time subtraction
};

__device__ inline float raw_time(int mode, const float* __restrict__ tin, uint32_t i) {
    if (mode == LNR_SCAN_TIME_GIVEN) return tin[i];
    return (float)(i & 2047u) / 2048.0f * 0.1f;          // LNR_SCAN_TIME_RECOMPUTE; unused for LNR_SCAN_TIME_NONE
}

// steps 3 of the contract on one element, the branches as ScanParams holds them
__device__ inline float final_time(uint32_t flags, float sub_neg, float sub_global, float stamp, float v) {
    if (flags & LNR_SCAN_CONSTANT) return stamp;
    if (flags & LNR_SCAN_NANOSECONDS) v = v * 1e-9f;
    if (flags & LNR_SCAN_NEGATIVE_START) v = v - sub_neg;
    return (flags & LNR_SCAN_LOCAL) ? v + stamp : (v - sub_global) + stamp;
}

__device__ inline float point_range(float x, float y, float z) { return sqrtf(__fmaf_rn(z, z, __fmaf_rn(y, y, x * x))); }

__device__ inline uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = __shfl_xor(v, o, 64);
        v = v > t ? v : t;
    }
    return v;
}

__global__ __launch_bounds__(CL_BLOCK) void ingest_flag(const float* __restrict__ xyz, const float* __restrict__ tin, uint32_t n, int mode,
                                                        FovSegments fov, float min_range, uint32_t* __restrict__ keep_out,
                                                        ScanParams* __restrict__ p) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool valid = i < n;
    bool keep = false;
    if (valid) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        bool in_fov = true;
        if (fov.enabled) {
            float theta = atan2f(y, x) * 57.29577951308232f;
            if (theta < 0.0f) theta = theta + 360.0f;
            in_fov = false;
            for (int s = 0; s < fov.n; ++s) in_fov = in_fov || (theta >= fov.lo[s] && theta <= fov.hi[s]);
        }
        keep = in_fov && point_range(x, y, z) > min_range;
        keep_out[i] = keep ? 1u : 0u;
    }
    uint32_t absbits = 0, bad = 0;
    if (keep && mode != LNR_SCAN_TIME_NONE) {
        const float t = raw_time(mode, tin, i);
        if (isfinite(t)) absbits = __float_as_uint(fabsf(t)); else bad = 1;
    }
    const unsigned long long kept = __ballot(keep);
    if (kept == 0ull) return;                                           // wave-uniform
    absbits = wave_max_u32(absbits);
    const unsigned long long bad_lanes = __ballot(bad != 0);
    const int lane = threadIdx.x & 63;
    const uint32_t wave_base = i - (uint32_t)lane;
    if (lane == 0) {
        const uint32_t first = wave_base + (uint32_t)__ffsll((long long)kept) - 1u;
        const uint32_t last = wave_base + 63u - (uint32_t)__clzll((long long)kept);
        atomicMax(&p->first_inv, ~first);
        atomicMax(&p->last, last);
        if (absbits) atomicMax(&p->maxabs_bits, absbits);
        if (bad_lanes) atomicAdd(&p->nonfinite, (uint32_t)__popcll(bad_lanes));
    }
}

__global__ void ingest_params(const float* __restrict__ tin, int mode, float stamp, ScanParams* __restrict__ p) {
    const uint32_t m = p->m;
    p->npasses = 0;
    p->key_shift = 0;
    p->sub_neg = 0.0f;
    p->sub_global = 0.0f;
    if (m == 0) { p->flags = 0; return; }
    uint32_t flags = 0;
    if (mode == LNR_SCAN_TIME_NONE) {
        flags = LNR_SCAN_NO_TIMES | LNR_SCAN_CONSTANT;
    } else {
        float v0 = raw_time(mode, tin, ~p->first_inv), v1 = raw_time(mode, tin, p->last);
        if (__uint_as_float(p->maxabs_bits) > 1e7f) {
            flags |= LNR_SCAN_NANOSECONDS;
            v0 = v0 * 1e-9f;
            v1 = v1 * 1e-9f;
        }
        if (v0 < -0.001f) {
            flags |= LNR_SCAN_NEGATIVE_START;
            p->sub_neg = v0;
            v1 = v1 - v0;
            v0 = v0 - v0;
        }
        if (v0 < 1e-2f) {
            flags |= LNR_SCAN_LOCAL;
            v0 = v0 + stamp;
            v1 = v1 + stamp;
        } else {
            flags |= LNR_SCAN_GLOBAL;
            p->sub_global = v0;
            v1 = (v1 - v0) + stamp;
            v0 = (v0 - v0) + stamp;
        }
        if (v1 - v0 < 1e-3f) flags |= LNR_SCAN_CONSTANT;
    }
    p->flags = flags;
    if (!(flags & LNR_SCAN_CONSTANT)) {
        uint32_t digits = 1;
        while (digits < 4 && ((m - 1) >> (8 * digits)) != 0) ++digits;
        p->key_shift = 8 * digits;
        p->npasses = (int32_t)digits + 4;
    }
}

__global__ __launch_bounds__(CL_BLOCK) void ingest_keys(const float* __restrict__ tin, const uint32_t* __restrict__ rank, uint32_t n, int mode,
                                                        float stamp, const ScanParams* __restrict__ p, uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t pos = rank[i], next = i + 1 < n ? rank[i + 1] : p->m;
    if (next == pos) return;                                            // dropped
    idx[pos] = i;
    if (p->npasses == 0) return;
    float t = final_time(p->flags, p->sub_neg, p->sub_global, stamp, raw_time(mode, tin, i));
    if (t == 0.0f) t = 0.0f;                                            // -0 and +0 tie
    const uint32_t bits = __float_as_uint(t);
    const uint32_t image = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    keys[pos] = ((uint64_t)image << p->key_shift) | (uint64_t)pos;
}

__global__ __launch_bounds__(CL_BLOCK) void ingest_gather(const float* __restrict__ xyz, const float* __restrict__ tin, int mode, float stamp,
                                                          ScanParams* __restrict__ p, SortedPairs sp, float* __restrict__ dirs,
                                                          float* __restrict__ dist_out, float* __restrict__ times,
                                                          int64_t* __restrict__ order) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    const uint32_t m = p->m;
    if (j >= m) return;
    const uint32_t* idx = sp.idx(p->npasses);
    const uint32_t i = idx[j];
    const uint32_t flags = p->flags;
    const float sn = p->sub_neg, sg = p->sub_global;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    const float d = point_range(x, y, z);
    const float t = final_time(flags, sn, sg, stamp, (flags & LNR_SCAN_CONSTANT) ? 0.0f : raw_time(mode, tin, i));
    dirs[j] = x / d;
    dirs[(size_t)m + j] = y / d;
    dirs[2 * (size_t)m + j] = z / d;
    dist_out[j] = d;
    times[j] = t;
    order[j] = (int64_t)i;
    if (j > 0 && !(flags & LNR_SCAN_CONSTANT)) {
        const float t_prev = final_time(flags, sn, sg, stamp, raw_time(mode, tin, idx[j - 1]));
        if (t < t_prev) atomicAdd(&p->unsorted, 1u);
    }
}

__global__ void ingest_info(const ScanParams* __restrict__ p, int64_t* __restrict__ info) {
    info[0] = p->m;
    info[1] = p->flags;
    info[2] = p->nonfinite;
    info[3] = p->unsorted;
    info[4] = p->npasses;
    info[5] = p->m ? (int64_t)(~p->first_inv) : -1;
    info[6] = p->m ? (int64_t)p->last : -1;
    info[7] = 0;
}

// the parameters, the n keep words, and the sort over n pairs (its sums also scan the keep words)
struct ScanLayout {
    size_t params, keep, total;
    SortLayout sort;
};
ScanLayout scan_layout(int64_t n) {
    ScanLayout l;
    l.params = 0;
    l.keep = align256(sizeof(ScanParams));
    l.sort = sort_layout(l.keep + 4 * (size_t)n, n, (uint64_t)n);
    l.total = l.sort.end;
    return l;
}

}  // namespace

extern "C" size_t lnr_scan_from_points_workspace(int64_t n_points) {
    if (!count_ok(n_points)) return 0;
    return scan_layout(n_points).total;
}

extern "C" int lnr_scan_from_points(const float* xyz, const float* point_times, int64_t n_points, int32_t time_mode, float stamp,
                                    int32_t fov_enabled, const float* fov_segments, int32_t n_fov_segments, float min_range,
                                    void* workspace, size_t workspace_bytes, float* ray_directions, float* distances, float* timestamps,
                                    int64_t* order, int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_scan_from_points", n_points, "points");
    LNR_REQUIRE(time_mode == LNR_SCAN_TIME_NONE || time_mode == LNR_SCAN_TIME_GIVEN || time_mode == LNR_SCAN_TIME_RECOMPUTE,
                "lnr_scan_from_points: time_mode %d is none of LNR_SCAN_TIME_*", time_mode);
    LNR_REQUIRE(n_fov_segments >= 0 && n_fov_segments <= LNR_SCAN_MAX_FOV_SEGMENTS, "lnr_scan_from_points: %d FOV segments, at most %d",
                n_fov_segments, LNR_SCAN_MAX_FOV_SEGMENTS);
    LNR_REQUIRE(isfinite(stamp) && !isnan(min_range), "lnr_scan_from_points: stamp must be finite and min_range a number");
    LNR_REQUIRE(info_dev && workspace && (n_fov_segments == 0 || fov_segments) &&
                    (n_points == 0 || (xyz && ray_directions && distances && timestamps && order)) &&
                    (n_points == 0 || time_mode != LNR_SCAN_TIME_GIVEN || point_times),
                "lnr_scan_from_points: null argument");
    const ScanLayout l = scan_layout(n_points);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_scan_from_points: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    FovSegments fov;
    fov.enabled = fov_enabled ? 1 : 0;
    fov.n = n_fov_segments;
    for (int s = 0; s < LNR_SCAN_MAX_FOV_SEGMENTS; ++s) {
        fov.lo[s] = s < n_fov_segments ? fov_segments[2 * s] : 0.0f;
        fov.hi[s] = s < n_fov_segments ? fov_segments[2 * s + 1] : 0.0f;
    }
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("scan_from_points", st);
    char* ws = (char*)workspace;
    ScanParams* p = (ScanParams*)(ws + l.params);
    if (int rc = clear_words(p, sizeof(ScanParams), st, "lnr_scan_from_points", "parameters")) return rc;
    if (n_points > 0) {
        const uint32_t n = (uint32_t)n_points;
        uint32_t* keep = (uint32_t*)(ws + l.keep);
        const RadixBuffers r = radix_buffers(ws, l.sort);
        hipLaunchKernelGGL(ingest_flag, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, xyz, point_times, n, (int)time_mode, fov, min_range, keep, p);
        enqueue_scan(keep, n, r.sums, &p->m, nullptr, 0, st);
        hipLaunchKernelGGL(ingest_params, dim3(1), dim3(1), 0, st, point_times, (int)time_mode, stamp, p);
        hipLaunchKernelGGL(ingest_keys, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, point_times, (const uint32_t*)keep, n, (int)time_mode, stamp,
                           (const ScanParams*)p, r.ka, r.ia);
        LNR_CHECK_LAUNCH("lnr_scan_from_points");
        enqueue_radix_sort(r, &p->m, &p->npasses, st);
        hipLaunchKernelGGL(ingest_gather, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, xyz, point_times, (int)time_mode, stamp, p,
                           sorted_pairs(r), ray_directions, distances, timestamps, order);
    }
    hipLaunchKernelGGL(ingest_info, dim3(1), dim3(1), 0, st, (const ScanParams*)p, info_dev);
    LNR_CHECK_LAUNCH("lnr_scan_from_points");
    return LNR_OK;
}
