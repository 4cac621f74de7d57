// Mesh sampling, the statistical outlier filter and the trajectory-compensated transform of a scan (gfx950): the three per-point tools
// the reference's map evaluation takes from open3d and scipy around the clouds of lnr_cloud.hip and lnr_icp.hip.
//   analysis/compute_metrics/maps/mesh_to_pcd.py        TriangleMesh::SamplePointsUniformly           lnr_mesh_sample_points
//   examples/fusion_portable/create_lidar_map.py:134    PointCloud::RemoveStatisticalOutliers         lnr_cloud_knn_mean_distance,
//                                                                                                     lnr_cloud_outlier_threshold
//   examples/fusion_portable/create_lidar_map.py:57-111 scipy Slerp and interp1d, T @ xyz             lnr_cloud_trajectory_transform
// with the definitions stated in include/loner_hip.h ("mesh sampling, outlier filter, trajectory transform").  This file is compiled
// with -ffp-contract=off (build.py EXACT): every fp64 expression below rounds operation by operation, as the numpy restatement
// (tests/cloud_tools_restatement.py) does.  No float atomics anywhere: two runs give the same bits.
//   sampling   areas, then their prefix sum as a 64-ary tree: one thread sums a chunk of 64 left to right, the chunk totals are summed
//              the same way level by level, and on the way down C_t = (prefix of the totals before the chunk) + (sum within the chunk);
//              the bounds n_t = round(C_t / S n) go through the same tree with max, since C_t may step down by an ulp where two chunks
//              meet; a block of 256 consecutive points searches the bounds twice (its first and last point, a wave each, 64 probes per
//              step) and each point then only between those two, which is no memory access at all when the block lies inside one
//              triangle
//   outlier    lnr_cloud_knn.h's search with the mean of the neighbours' distances as its Finish; the mean and the deviation as the ICP
//              sums are taken: per thread in index order, per block, then one workgroup's fold
//   trajectory a count per block of kept points, one workgroup's scan of the counts, and the emit that recomputes the (cheap) keep test
//              and ranks its points within the block by ballots: input order is kept without a sort
#include "lnr_cloud_knn.h"
#include "lnr_traj.h"

namespace {

// ------------------------------------------------------------------------------------------------ the 64-ary tree
#define TREE_ARITY 64
#define TREE_MAX_LEVELS 6               /* 64^6 > 2^31 */

struct SumF64 {
    __device__ inline double operator()(double a, double b) const { return a + b; }
};
struct MaxI64 {
    __device__ inline int64_t operator()(int64_t a, int64_t b) const { return a > b ? a : b; }
};

// tot[c] = ((a[64 c] op a[64 c + 1]) op ...) over the chunk's elements below n
template <class T, class Op>
__global__ __launch_bounds__(CL_BLOCK) void tree_totals(const T* __restrict__ a, uint32_t n, T* __restrict__ tot, uint32_t n_chunks) {
    const uint32_t c = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (c >= n_chunks) return;
    const size_t base = (size_t)TREE_ARITY * c;
    const uint32_t m = n - base < TREE_ARITY ? (uint32_t)(n - base) : (uint32_t)TREE_ARITY;
    const Op op{};
    T r = a[base];
    for (uint32_t j = 1; j < m; ++j) r = op(r, a[base + j]);
    tot[c] = r;
}

// in place: a[t] = up[c - 1] op (the chunk's elements up to t, left to right), without the first term in chunk 0.  up: the inclusive
// prefix of the chunk totals (unused at the top level, which is one chunk)
template <class T, class Op>
__global__ __launch_bounds__(CL_BLOCK) void tree_prefix(T* __restrict__ a, uint32_t n, const T* __restrict__ up, uint32_t n_chunks) {
    const uint32_t c = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (c >= n_chunks) return;
    const size_t base = (size_t)TREE_ARITY * c;
    const uint32_t m = n - base < TREE_ARITY ? (uint32_t)(n - base) : (uint32_t)TREE_ARITY;
    const Op op{};
    T r = a[base];
    if (c == 0) {
        for (uint32_t j = 1; j < m; ++j) { r = op(r, a[base + j]); a[base + j] = r; }
    } else {
        const T before = up[c - 1];
        a[base] = op(before, r);
        for (uint32_t j = 1; j < m; ++j) { r = op(r, a[base + j]); a[base + j] = op(before, r); }
    }
}

struct TreeLevels {
    int levels;                         // level 0 is the array itself
    uint32_t n[TREE_MAX_LEVELS];
    size_t off[TREE_MAX_LEVELS];        // element offset of level l >= 1 within the tree space
    size_t total;                       // elements of levels 1..
};
TreeLevels tree_levels(uint32_t n) {
    TreeLevels t;
    t.levels = 1;
    t.n[0] = n;
    t.off[0] = 0;
    t.total = 0;
    while (t.n[t.levels - 1] > TREE_ARITY) {
        t.n[t.levels] = (t.n[t.levels - 1] + TREE_ARITY - 1) / TREE_ARITY;
        t.off[t.levels] = t.total;
        t.total += t.n[t.levels];
        ++t.levels;
    }
    return t;
}

// the inclusive prefix of a[0, n) under op, in place; space: t.total elements
template <class T, class Op>
void enqueue_tree_prefix(T* a, const TreeLevels& t, T* space, hipStream_t st) {
    T* lv[TREE_MAX_LEVELS];
    lv[0] = a;
    for (int l = 1; l < t.levels; ++l) lv[l] = space + t.off[l];
    for (int l = 0; l + 1 < t.levels; ++l)
        hipLaunchKernelGGL((tree_totals<T, Op>), dim3(blocks_for(t.n[l + 1])), dim3(CL_BLOCK), 0, st, (const T*)lv[l], t.n[l], lv[l + 1],
                           t.n[l + 1]);
    for (int l = t.levels - 1; l >= 0; --l) {
        const uint32_t chunks = (t.n[l] + TREE_ARITY - 1) / TREE_ARITY;
        hipLaunchKernelGGL((tree_prefix<T, Op>), dim3(blocks_for(chunks)), dim3(CL_BLOCK), 0, st, lv[l], t.n[l],
                           (const T*)(l + 1 < t.levels ? lv[l + 1] : nullptr), chunks);
    }
}

// ------------------------------------------------------------------------------------------------ mesh sampling
enum { MS_ST_NONFINITE = 1, MS_ST_BAD_INDEX = 2, MS_ST_AREA = 4 };

struct MeshHead {
    double total;                       // S
    uint32_t status;
    unsigned long long bad;             // triangles with a non-finite vertex or an index out of range
};

__global__ __launch_bounds__(CL_BLOCK) void mesh_areas(const double* __restrict__ v, int64_t n_verts, const int32_t* __restrict__ tri,
                                                       uint32_t n_tris, double* __restrict__ area, MeshHead* h) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    const int64_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    double a = 0.0;
    uint32_t st = 0;
    if (i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) {      // (own test: lnr_mesh_args.h's cost 2 VGPRs)
        st = MS_ST_BAD_INDEX;
    } else {
        const double *p0 = v + 3 * (size_t)i0, *p1 = v + 3 * (size_t)i1, *p2 = v + 3 * (size_t)i2;
        if (!(finite3(p0[0], p0[1], p0[2]) && finite3(p1[0], p1[1], p1[2]) && finite3(p2[0], p2[1], p2[2]))) {
            st = MS_ST_NONFINITE;
        } else {
            const double ux = p0[0] - p1[0], uy = p0[1] - p1[1], uz = p0[2] - p1[2];
            const double wx = p0[0] - p2[0], wy = p0[1] - p2[1], wz = p0[2] - p2[2];
            const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
            a = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
        }
    }
    area[t] = a;
    if (st) {
        atomicOr(&h->status, st);
        atomicAdd(&h->bad, 1ull);
    }
}

// one thread, after the prefix sum: S and the outcome
__global__ void mesh_total(const double* __restrict__ cdf, uint32_t n_tris, int64_t n_points, MeshHead* h, int64_t* __restrict__ info) {
    const double S = n_tris ? cdf[n_tris - 1] : 0.0;
    if (!isfinite(S)) h->status |= MS_ST_AREA;
    h->total = S;
    info[0] = h->status;
    info[1] = h->status == 0 && S > 0.0 ? n_points : 0;
    info[2] = (int64_t)h->bad;
    info[3] = (int64_t)__double_as_longlong(S);
    info[4] = 0; info[5] = 0; info[6] = 0; info[7] = 0;
}

// n_t before the running max: round((C_t / S) n), half away from zero, within [0, n]
__global__ __launch_bounds__(CL_BLOCK) void mesh_bounds(const double* __restrict__ cdf, uint32_t n_tris, int64_t n_points,
                                                        const MeshHead* __restrict__ h, int64_t* __restrict__ bound) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    int64_t b = 0;
    if (h->status == 0 && h->total > 0.0) {
        const double x = round((cdf[t] / h->total) * (double)n_points);
        b = x >= (double)n_points ? n_points : (x > 0.0 ? (int64_t)x : 0);
    }
    bound[t] = b;
}

// the first t in [lo, hi] with bound[t] > i (bound[hi] > i is the caller's)
__device__ inline uint32_t mesh_owner(const int64_t* __restrict__ bound, uint32_t lo, uint32_t hi, int64_t i) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bound[mid] > i) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the same for one wave at a time (uniform arguments, all 64 lanes active): 64 probes per step instead of one, so the 20 dependent
// loads of a binary search over 10^6 bounds become 4
__device__ inline uint32_t mesh_owner_wave(const int64_t* __restrict__ bound, uint32_t lo, uint32_t hi, int64_t i) {
    const uint32_t lane = threadIdx.x & 63;
    while (hi - lo >= 64) {
        const uint32_t step = (hi - lo) / 64 + 1;               // lane l probes the end of the l-th piece; the last pieces reach hi
        const uint64_t want = (uint64_t)lo + (uint64_t)(lane + 1) * step - 1;
        const uint32_t at = want < hi ? (uint32_t)want : hi;
        const unsigned long long above = __ballot(bound[at] > i);          // monotone in the lane; lane 63 probes hi: never empty
        const uint32_t f = (uint32_t)__ffsll((long long)above) - 1;
        const uint64_t end = (uint64_t)lo + (uint64_t)(f + 1) * step - 1;
        const uint32_t new_lo = f ? lo + f * step : lo;
        hi = end < hi ? (uint32_t)end : hi;
        lo = new_lo;
    }
    const uint32_t at = lo + lane < hi ? lo + lane : hi;
    const unsigned long long above = __ballot(bound[at] > i);
    return lo + (uint32_t)__ffsll((long long)above) - 1;
}

__device__ inline double u53(uint32_t hi, uint32_t lo) { return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1p-53; }

__global__ __launch_bounds__(CL_BLOCK) void mesh_points(const double* __restrict__ v, const int32_t* __restrict__ tri,
                                                        const int64_t* __restrict__ bound, uint32_t n_tris, int64_t n_points, uint64_t seed,
                                                        const MeshHead* __restrict__ h, double* __restrict__ points,
                                                        int32_t* __restrict__ tri_out) {
    if (h->status || !(h->total > 0.0)) return;
    __shared__ uint32_t span[2];
    const int64_t first = (int64_t)blockIdx.x * CL_BLOCK;
    const int64_t last = first + CL_BLOCK - 1 < n_points - 1 ? first + CL_BLOCK - 1 : n_points - 1;
    if (threadIdx.x < 128) {                                    // wave 0: the first point's triangle; wave 1: the last point's
        const uint32_t t = mesh_owner_wave(bound, 0, n_tris - 1, threadIdx.x < 64 ? first : last);
        if ((threadIdx.x & 63) == 0) span[threadIdx.x >> 6] = t;
    }
    __syncthreads();
    const int64_t i = first + threadIdx.x;
    if (i <= last) {
        const uint32_t t = mesh_owner(bound, span[0], span[1], i);
        const double *p0 = v + 3 * (size_t)tri[3 * (size_t)t], *p1 = v + 3 * (size_t)tri[3 * (size_t)t + 1],
                     *p2 = v + 3 * (size_t)tri[3 * (size_t)t + 2];
        const Philox4 r = philox4x32_10((uint64_t)i, LNR_STREAM_MESH, seed);
        const double r1 = u53(r.x, r.y), r2 = u53(r.z, r.w);
        const double s = sqrt(r1);
        const double a = 1.0 - s, b = s * (1.0 - r2), c = s * r2;
#pragma unroll
        for (int e = 0; e < 3; ++e) points[3 * (size_t)i + e] = (a * p0[e] + b * p1[e]) + c * p2[e];
        if (tri_out) tri_out[i] = (int32_t)t;
    }
}

struct MeshLayout { size_t head, cdf, bound, tree, total; };
MeshLayout mesh_layout(int64_t n_tris) {
    MeshLayout l;
    l.head = 0;
    l.cdf = align256(sizeof(MeshHead));
    l.bound = align256(l.cdf + 8 * (size_t)n_tris);
    l.tree = align256(l.bound + 8 * (size_t)n_tris);
    l.total = align256(l.tree + 8 * tree_levels((uint32_t)n_tris).total);
    return l;
}

// ------------------------------------------------------------------------------------------------ outlier filter
// lnr_cloud_knn.h's Finish: the mean of the first min(k, found) distances, summed in list order
struct MeanDistanceFinish {
    double* __restrict__ avg;

    __device__ inline void operator()(const GridView&, const KnnList& L, int k, uint32_t out) const {
        const uint32_t m = L.found < (uint32_t)k ? L.found : (uint32_t)k;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < LNR_KNN_MAX; ++j)
            if ((uint32_t)j < m) s = s + sqrt(L.d[j]);
        avg[out] = s / (double)m;
    }
};

#define OT_MAX_BLOCKS 2048

uint32_t outlier_blocks(int64_t n) {
    const uint32_t b = blocks_for(n);
    return b < 1 ? 1u : (b < OT_MAX_BLOCKS ? b : (uint32_t)OT_MAX_BLOCKS);
}

// PASS 0: the sum of avg_i > 0; PASS 1: of (avg_i - mean)^2 over the same.  Thread by thread in index order (i = thread, thread +
// stride, ...), then the block's fixed-order sum
template <int PASS>
__global__ __launch_bounds__(CL_BLOCK) void outlier_part(const double* __restrict__ avg, uint32_t n, const double* __restrict__ res,
                                                         double* __restrict__ part) {
    __shared__ double lds[CL_BLOCK / 64];
    const double mean = PASS ? res[0] : 0.0;
    double acc = 0.0;
    for (uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x; i < n; i += gridDim.x * CL_BLOCK) {
        const double a = avg[i];
        if (a > 0.0) {
            const double d = a - mean;
            acc = PASS ? acc + d * d : acc + a;
        }
    }
    const double t = block_sum(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// one workgroup: the partials as icp_fold sums them (thread t: blocks t, t + 256, ... in turn, then the block sum); res {mean, std,
// threshold, valid}
template <int PASS>
__global__ __launch_bounds__(CL_BLOCK) void outlier_fold(const double* __restrict__ part, uint32_t n_part, const CloudParams* __restrict__ p,
                                                         uint32_t n, double std_ratio, double* __restrict__ res) {
    __shared__ double lds[CL_BLOCK / 64];
    double a = 0.0;
    for (uint32_t b = threadIdx.x; b < n_part; b += CL_BLOCK) a = a + part[b];
    const double t = block_sum(a, lds);
    if (threadIdx.x != 0) return;
    const double valid = p->status == 0 && p->n == n ? (double)n : 0.0;
    if (PASS == 0) {
        res[0] = t / valid;
        res[3] = valid;
    } else {
        const double sd = sqrt(t / (valid - 1.0));
        res[1] = sd;
        res[2] = res[0] + std_ratio * sd;
    }
}

// ------------------------------------------------------------------------------------------------ trajectory transform
enum { TJ_KEEP = 0, TJ_NONFINITE = 1, TJ_BELOW = 2, TJ_OUTSIDE = 3 };

__device__ inline int traj_class(const double* __restrict__ pts, const double* __restrict__ stamps, uint32_t i, const TrajView& tv,
                                 double min_range) {
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2], tau = stamps[i];
    if (!(finite3(x, y, z) && isfinite(tau))) return TJ_NONFINITE;
    if (!(sqrt((x * x + y * y) + z * z) > min_range)) return TJ_BELOW;
    if (tau < tv.T[0] || tau > tv.T[tv.K - 1]) return TJ_OUTSIDE;
    return TJ_KEEP;
}

// tally [4]: points per class; count[b]: the kept points of block b
__global__ __launch_bounds__(CL_BLOCK) void traj_count(const double* __restrict__ pts, const double* __restrict__ stamps, uint32_t n,
                                                       TrajView tv, double min_range, uint32_t* __restrict__ count,
                                                       unsigned long long* __restrict__ tally) {
    __shared__ uint32_t wave_kept[CL_BLOCK / 64];
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    const int cls = i < n ? traj_class(pts, stamps, i, tv, min_range) : -1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned long long k = (unsigned long long)__popcll(__ballot(cls == c));
        if ((threadIdx.x & 63) == 0) {
            if (k) atomicAdd(&tally[c], k);
            if (c == TJ_KEEP) wave_kept[threadIdx.x >> 6] = (uint32_t)k;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < CL_BLOCK / 64; ++w) t += wave_kept[w];
        count[blockIdx.x] = t;
    }
}

// one workgroup: count becomes its exclusive prefix, 256 blocks at a time with a running carry; then the outcome
__global__ __launch_bounds__(CL_BLOCK) void traj_scan(uint32_t* __restrict__ count, uint32_t n_blocks, const unsigned long long* __restrict__ tally,
                                                      int64_t* __restrict__ info) {
    __shared__ uint32_t lds[CL_BLOCK / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += CL_BLOCK) {
        const uint32_t b = base + threadIdx.x;
        uint32_t all;
        const uint32_t before = block_exclusive_scan(b < n_blocks ? count[b] : 0u, lds, &all);
        if (b < n_blocks) count[b] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) {
        info[0] = tally[TJ_NONFINITE] ? 1 : 0;
        info[1] = (int64_t)tally[TJ_KEEP];
        info[2] = (int64_t)tally[TJ_BELOW];
        info[3] = (int64_t)tally[TJ_OUTSIDE];
        info[4] = (int64_t)tally[TJ_NONFINITE];
        info[5] = 0; info[6] = 0; info[7] = 0;
    }
}

__device__ inline void libm_sincos(double theta, double* s, double* c) {
    *s = sin(theta);
    *c = cos(theta);
}

// the pose at tau (lnr_traj.h, with the library's sine) applied to one point
__device__ inline void traj_apply(const TrajView& tv, double x, double y, double z, double tau, double* __restrict__ out) {
    double R[9], trans[3];
    traj_pose<libm_sincos>(tv, tau, R, trans);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = ((R[3 * a] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z) + trans[a];
}

// kept point i of block b goes to out[count[b] + (kept points of the block before i)]
__global__ __launch_bounds__(CL_BLOCK) void traj_emit(const double* __restrict__ pts, const double* __restrict__ stamps, uint32_t n,
                                                      TrajView tv, double min_range, const uint32_t* __restrict__ count,
                                                      double* __restrict__ out) {
    __shared__ uint32_t wave_kept[CL_BLOCK / 64];
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool keep = i < n && traj_class(pts, stamps, i, tv, min_range) == TJ_KEEP;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_kept[w] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (!keep) return;
    uint32_t rank = count[blockIdx.x] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    for (uint32_t u = 0; u < w; ++u) rank += wave_kept[u];
    traj_apply(tv, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], stamps[i], out + 3 * (size_t)rank);
}

// ------------------------------------------------------------------------------------------------ host
// one workspace for the three cloud entries: the partials or the tallies, then n words (the exact pass's list, or the block counts)
struct CloudToolsLayout { size_t part, words, total; };
CloudToolsLayout cloud_tools_layout(int64_t n) {
    CloudToolsLayout l;
    l.part = 0;
    l.words = align256(sizeof(double) * OT_MAX_BLOCKS);
    l.total = align256(l.words + 4 * ((size_t)n + 1));
    return l;
}

}  // namespace

extern "C" size_t lnr_mesh_sample_workspace(int64_t n_triangles) {
    if (!count_ok(n_triangles)) return 0;
    return mesh_layout(n_triangles).total;
}

extern "C" int lnr_mesh_sample_points(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                      int64_t n_points, uint64_t seed, void* workspace, size_t workspace_bytes, double* points,
                                      int32_t* triangle_index, int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNTS("lnr_mesh_sample_points", n_triangles, "triangles", n_points, "points");
    LNR_REQUIRE(n_vertices >= 0 && n_vertices <= INT32_MAX, "lnr_mesh_sample_points: %lld vertices, the limit is %d", (long long)n_vertices,
                INT32_MAX);
    LNR_REQUIRE(info_dev && workspace && (n_triangles == 0 || triangles) && (n_vertices == 0 || vertices) &&
                    (n_points == 0 || n_triangles == 0 || points),
                "lnr_mesh_sample_points: null argument");
    const MeshLayout l = mesh_layout(n_triangles);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_mesh_sample_points: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    MeshHead* h = (MeshHead*)(ws + l.head);
    double* cdf = (double*)(ws + l.cdf);
    int64_t* bound = (int64_t*)(ws + l.bound);
    if (int rc = clear_words(h, sizeof(MeshHead), st, "lnr_mesh_sample_points", "head")) return rc;
    LnrProfScope prof("mesh_sample_points", st);
    const uint32_t F = (uint32_t)n_triangles;
    const TreeLevels t = tree_levels(F);
    if (F) {
        hipLaunchKernelGGL(mesh_areas, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, vertices, n_vertices, triangles, F, cdf, h);
        enqueue_tree_prefix<double, SumF64>(cdf, t, (double*)(ws + l.tree), st);
    }
    hipLaunchKernelGGL(mesh_total, dim3(1), dim3(1), 0, st, (const double*)cdf, F, n_points, h, info_dev);
    LNR_CHECK_LAUNCH("lnr_mesh_sample_points");
    if (F == 0 || n_points == 0) return LNR_OK;
    hipLaunchKernelGGL(mesh_bounds, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, (const double*)cdf, F, n_points, (const MeshHead*)h, bound);
    enqueue_tree_prefix<int64_t, MaxI64>(bound, t, (int64_t*)(ws + l.tree), st);
    hipLaunchKernelGGL(mesh_points, dim3(blocks_for(n_points)), dim3(CL_BLOCK), 0, st, vertices, triangles, (const int64_t*)bound, F,
                       n_points, seed, (const MeshHead*)h, points, triangle_index);
    LNR_CHECK_LAUNCH("lnr_mesh_sample_points");
    return LNR_OK;
}

extern "C" size_t lnr_cloud_tools_workspace(int64_t n_points) {
    if (!count_ok(n_points)) return 0;
    return cloud_tools_layout(n_points).total;
}

extern "C" int lnr_cloud_knn_mean_distance(const void* grid, int64_t n_points, int32_t nb_neighbors, double* mean_distance,
                                           void* workspace, size_t workspace_bytes, int64_t* counters_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_knn_mean_distance", n_points, "points");
    LNR_REQUIRE(nb_neighbors >= 1 && nb_neighbors <= LNR_KNN_MAX, "lnr_cloud_knn_mean_distance: nb_neighbors must be in [1, %d], got %d",
                LNR_KNN_MAX, (int)nb_neighbors);
    LNR_REQUIRE(grid && counters_dev && workspace && (n_points == 0 || mean_distance), "lnr_cloud_knn_mean_distance: null argument");
    const CloudToolsLayout l = cloud_tools_layout(n_points);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_cloud_knn_mean_distance: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = clear_words(counters_dev, 4 * sizeof(int64_t), st, "lnr_cloud_knn_mean_distance", "counters")) return rc;
    if (n_points == 0) return LNR_OK;
    LnrProfScope prof("cloud_knn_mean_distance", st);
    enqueue_knn(grid_view(grid, n_points), (uint32_t)n_points, (int)nb_neighbors, MeanDistanceFinish{mean_distance},
                (uint32_t*)((char*)workspace + l.words), (unsigned long long*)counters_dev, st);
    LNR_CHECK_LAUNCH("lnr_cloud_knn_mean_distance");
    return LNR_OK;
}

extern "C" int lnr_cloud_outlier_threshold(const void* grid, const double* mean_distance, int64_t n_points, double std_ratio,
                                           void* workspace, size_t workspace_bytes, double* result_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_outlier_threshold", n_points, "points");
    LNR_REQUIRE(isfinite(std_ratio), "lnr_cloud_outlier_threshold: std_ratio must be finite, got %g", std_ratio);
    LNR_REQUIRE(grid && workspace && result_dev && (n_points == 0 || mean_distance), "lnr_cloud_outlier_threshold: null argument");
    const CloudToolsLayout l = cloud_tools_layout(n_points);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_cloud_outlier_threshold: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("cloud_outlier_threshold", st);
    const CloudParams* p = grid_view(grid, n_points).p;
    double* part = (double*)((char*)workspace + l.part);
    const uint32_t n = (uint32_t)n_points, nb = outlier_blocks(n_points);
    hipLaunchKernelGGL(outlier_part<0>, dim3(nb), dim3(CL_BLOCK), 0, st, mean_distance, n, (const double*)result_dev, part);
    hipLaunchKernelGGL(outlier_fold<0>, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)part, nb, p, n, std_ratio, result_dev);
    hipLaunchKernelGGL(outlier_part<1>, dim3(nb), dim3(CL_BLOCK), 0, st, mean_distance, n, (const double*)result_dev, part);
    hipLaunchKernelGGL(outlier_fold<1>, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)part, nb, p, n, std_ratio, result_dev);
    LNR_CHECK_LAUNCH("lnr_cloud_outlier_threshold");
    return LNR_OK;
}

extern "C" int lnr_cloud_trajectory_transform(const double* points, const double* timestamps, int64_t n_points, const double* traj_times,
                                              const double* traj_positions, const double* traj_rotations, const double* traj_rotvecs,
                                              int64_t n_poses, double min_range, void* workspace, size_t workspace_bytes, double* out,
                                              int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_trajectory_transform", n_points, "points");
    LNR_REQUIRE(n_poses >= 2 && n_poses <= INT32_MAX, "lnr_cloud_trajectory_transform: %lld poses, at least 2 are needed",
                (long long)n_poses);
    LNR_REQUIRE(!(min_range != min_range), "lnr_cloud_trajectory_transform: min_range is NaN");
    LNR_REQUIRE(traj_times && traj_positions && traj_rotations && traj_rotvecs && workspace && info_dev &&
                    (n_points == 0 || (points && timestamps && out)),
                "lnr_cloud_trajectory_transform: null argument");
    const CloudToolsLayout l = cloud_tools_layout(n_points);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_cloud_trajectory_transform: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned long long* tally = (unsigned long long*)(ws + l.part);
    uint32_t* count = (uint32_t*)(ws + l.words);
    if (int rc = clear_words(tally, 4 * sizeof(unsigned long long), st, "lnr_cloud_trajectory_transform", "tallies")) return rc;
    LnrProfScope prof("cloud_trajectory_transform", st);
    const TrajView tv{traj_times, traj_positions, traj_rotations, traj_rotvecs, (uint32_t)n_poses};
    const uint32_t n = (uint32_t)n_points, nb = blocks_for(n_points);
    if (n) hipLaunchKernelGGL(traj_count, dim3(nb), dim3(CL_BLOCK), 0, st, points, timestamps, n, tv, min_range, count, tally);
    hipLaunchKernelGGL(traj_scan, dim3(1), dim3(CL_BLOCK), 0, st, count, nb, (const unsigned long long*)tally, info_dev);
    if (n) hipLaunchKernelGGL(traj_emit, dim3(nb), dim3(CL_BLOCK), 0, st, points, timestamps, n, tv, min_range, (const uint32_t*)count, out);
    LNR_CHECK_LAUNCH("lnr_cloud_trajectory_transform");
    return LNR_OK;
}
