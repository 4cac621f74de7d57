// Point clouds of a rendered map (gfx950): scan points, voxel down-sampling, the rigid transform of a merged scan, and exact
// nearest-neighbour distances between two clouds.
//
// Replaces the open3d calls of analysis/renderer_lidar.py:71-91, :296-349 and analysis/evaluate_lidar_map.py:16-98:
//   PointCloud.voxel_down_sample, PointCloud.transform, PointCloud.compute_point_cloud_distance
// with the definitions stated in include/loner_hip.h ("point clouds").  This file is compiled with -ffp-contract=off (build.py EXACT):
// every fp64 expression below rounds operation by operation, as the numpy restatement (tests/cloud_restatement.py) does; the divides
// and square roots are IEEE (no fast-math).
//
// Everything is built from one device-wide stable sort of (uint64 key, uint32 index) pairs:
//   bound      per-block min / max of the finite points and a count of the others, then one workgroup folds them into the
//              parameters of the call (origin, edge, bits per axis, digit passes, status) in device memory
//   key        per point: the packed cell index (x highest, z lowest), only as many bits as the bound needs
//   sort       LSD radix, 8-bit digits: count (per-block histograms), exclusive scan of the [digit][block] table, stable scatter
//              (rank within a 256-element chunk from eight ballots per wave).  All 8 passes are enqueued; those the key does not
//              need return at once (the pass count is on the device, the host never waits for it)
//   segments   heads (key differs from its predecessor), their exclusive scan and the start of each run
//   voxel      one thread per occupied voxel sums its points in input order (the sort is stable) and divides by the count
//   grid       the targets gathered in key order, one (key, start) per occupied cell
// The nearest-neighbour query walks Chebyshev shells of cells around the query's cell and stops when its best squared distance is
// below a rounding-safe lower bound on every unvisited cell; queries still open after NN_MAX_SHELL shells stream every target
// through LDS.  The walk and that exact pass are lnr_cloud_grid.h's, shared with the kNN normals and the ICP of lnr_icp.hip.
// The scan, the sort and its workspace layout are lnr_radix_sort.h's, shared with every tool that sorts.  The bound, the parameters and the key
// are lnr_cloud_keys.h's, shared with the vertex clustering of lnr_mesh_filters.hip.
#include "lnr_cloud_keys.h"

namespace {

// ------------------------------------------------------------------------------------------------ segments
__global__ __launch_bounds__(CL_BLOCK) void segment_heads(SortedPairs sp, const CloudParams* __restrict__ p, uint32_t n_cap,
                                                          uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n_cap) return;
    const uint64_t* k = sp.keys(p->npasses);
    flags[i] = (i < p->n && (i == 0 || k[i] != k[i - 1])) ? 1u : 0u;
}

__global__ __launch_bounds__(CL_BLOCK) void segment_starts(SortedPairs sp, const CloudParams* __restrict__ p,
                                                           const uint32_t* __restrict__ seg, uint32_t* __restrict__ starts) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= p->n) return;
    const uint64_t* k = sp.keys(p->npasses);
    if (i == 0 || k[i] != k[i - 1]) starts[seg[i]] = i;
}

// one thread per occupied voxel: the fp64 sum of its points in input order, divided by the count (open3d AccumulatedPoint)
__global__ __launch_bounds__(CL_BLOCK) void voxel_average(const double* __restrict__ pts, const uint32_t* __restrict__ ia,
                                                          const uint32_t* __restrict__ ib, const CloudParams* __restrict__ p,
                                                          const uint32_t* __restrict__ starts, double* __restrict__ out) {
    const uint32_t s = blockIdx.x * CL_BLOCK + threadIdx.x;
    const uint32_t n_seg = p->n_seg;
    if (s >= n_seg) return;
    const uint32_t* idx = sorted_idx(p->npasses, ia, ib);
    const uint32_t j0 = starts[s], j1 = s + 1 < n_seg ? starts[s + 1] : p->n;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t j = j0; j < j1; ++j) {
        const size_t q = 3 * (size_t)idx[j];
        sx = sx + pts[q];
        sy = sy + pts[q + 1];
        sz = sz + pts[q + 2];
    }
    const double c = (double)(j1 - j0);
    out[3 * (size_t)s] = sx / c;
    out[3 * (size_t)s + 1] = sy / c;
    out[3 * (size_t)s + 2] = sz / c;
}

// the grid: targets in key order with their input index (ascending within a cell: the sort is stable), one (key, first target) per
// occupied cell, and the end sentinel
__global__ __launch_bounds__(CL_BLOCK) void grid_fill(const double* __restrict__ pts, SortedPairs sp, const CloudParams* __restrict__ p,
                                                      const uint32_t* __restrict__ starts, double* __restrict__ sorted,
                                                      uint64_t* __restrict__ cell_key, uint32_t* __restrict__ cell_start,
                                                      uint32_t* __restrict__ orig) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    const uint32_t n = p->n, n_seg = p->n_seg;
    if (i < n) {
        const uint32_t o = sp.idx(p->npasses)[i];
        const size_t q = 3 * (size_t)o;
        orig[i] = o;
        sorted[3 * (size_t)i] = pts[q];
        sorted[3 * (size_t)i + 1] = pts[q + 1];
        sorted[3 * (size_t)i + 2] = pts[q + 2];
    }
    if (i < n_seg) {
        cell_start[i] = starts[i];
        cell_key[i] = sp.keys(p->npasses)[starts[i]];
    }
    if (i == 0) cell_start[n_seg] = n;
}

__global__ void cloud_info(const CloudParams* __restrict__ p, int64_t* __restrict__ info) {
    info[0] = p->status;
    info[1] = p->n_seg;
    info[2] = (int64_t)p->nonfinite;
    info[3] = p->bits;
    info[4] = (int64_t)__double_as_longlong(p->edge);
    for (int a = 0; a < 3; ++a) info[5 + a] = p->dims[a];
}

// ------------------------------------------------------------------------------------------------ scan points and transform
__device__ inline bool scan_keep(float depth, float var, float scale, float var_max, float depth_max, float* depth_m) {
    const float d = depth * scale, v = var * scale;
    *depth_m = d;
    return v < var_max && d < depth_max;
}

__global__ __launch_bounds__(CL_BLOCK) void scan_flags(const float* __restrict__ depth, const float* __restrict__ var, uint32_t m,
                                                       float scale, float var_max, float depth_max, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= m) return;
    float d;
    flags[i] = scan_keep(depth[i], var[i], scale, var_max, depth_max, &d) ? 1u : 0u;
}

__global__ __launch_bounds__(CL_BLOCK) void scan_emit(const float* __restrict__ depth, const float* __restrict__ var,
                                                      const int64_t* __restrict__ ray_index, const float* __restrict__ dirs, int64_t n_dirs,
                                                      uint32_t m, float scale, float var_max, float depth_max,
                                                      const uint32_t* __restrict__ pos, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= m) return;
    float d;
    if (!scan_keep(depth[i], var[i], scale, var_max, depth_max, &d)) return;
    const int64_t r = ray_index[i];
    if (r < 0 || r >= n_dirs) return;
    const size_t o = 3 * (size_t)pos[i];
#pragma unroll
    for (int a = 0; a < 3; ++a) out[o + a] = (double)(dirs[a * n_dirs + r] * d);
}

__global__ __launch_bounds__(CL_BLOCK) void append_transformed(const double* src, uint32_t n, Affine T, double* dst) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i < n) transform_point(src, T.t, dst, i);
}

// ------------------------------------------------------------------------------------------------ nearest-neighbour distance
__global__ __launch_bounds__(CL_BLOCK) void nn_shells(GridView g, const double* __restrict__ q, uint32_t n_q, double* __restrict__ dist,
                                                      double* __restrict__ d2_out, uint32_t* __restrict__ fallback,
                                                      unsigned long long* __restrict__ counters) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    unsigned long long shells = 0;
    if (i < n_q) {
        const CloudParams* p = g.p;
        const double qv[3] = {q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2]};
        if (!finite3(qv[0], qv[1], qv[2])) {
            atomicAdd(&counters[1], 1ull);
            dist[i] = NAN;
            if (d2_out) d2_out[i] = NAN;
        } else if (p->n == 0) {                         // no target: open3d's SearchKNN finds nothing and the distance stays 0
            dist[i] = 0.0;
            if (d2_out) d2_out[i] = 0.0;
        } else {
            const ShellQuery s = shell_query(p, qv[0], qv[1], qv[2]);
            double best = INFINITY;
            auto visit = [&](uint32_t j) { best = fmin(best, sq_dist(s.q[0], s.q[1], s.q[2], g.pts + 3 * (size_t)j)); };
            bool done = false;
            for (int r = 0; r <= NN_MAX_SHELL && !done; ++r) {
                ++shells;
                const double lb = shell_visit(g, s, r, visit);
                done = lb == INFINITY || best <= lb;
            }
            if (done) {
                dist[i] = sqrt(best);
                if (d2_out) d2_out[i] = best;
            } else {
                fallback[atomicAdd(&counters[0], 1ull)] = i;
            }
        }
    }
    shells = wave_sum(shells);
    if ((threadIdx.x & 63) == 0 && shells) atomicAdd(&counters[2], shells);
}

// the exact fallback: one query per thread, every target streamed through LDS in tiles
__global__ __launch_bounds__(CL_BLOCK) void nn_brute(GridView g, const double* __restrict__ q, const uint32_t* __restrict__ fallback,
                                                     const unsigned long long* __restrict__ counters, double* __restrict__ dist,
                                                     double* __restrict__ d2_out) {
    __shared__ double tile[NN_FB_TILE * 3];
    const uint32_t n_fb = (uint32_t)counters[0];
    if ((uint64_t)blockIdx.x * CL_BLOCK >= n_fb) return;
    const uint32_t k = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool active = k < n_fb;
    const uint32_t i = active ? fallback[k] : 0u;
    const double qx = active ? q[3 * (size_t)i] : 0.0, qy = active ? q[3 * (size_t)i + 1] : 0.0, qz = active ? q[3 * (size_t)i + 2] : 0.0;
    const uint32_t n = g.p->n;
    double best = INFINITY;
    for (uint32_t t0 = 0; t0 < n; t0 += NN_FB_TILE) {
        const uint32_t m = n - t0 < NN_FB_TILE ? n - t0 : NN_FB_TILE;
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < 3 * m; e += CL_BLOCK) tile[e] = g.pts[3 * (size_t)t0 + e];
        __syncthreads();
        for (uint32_t j = 0; j < m; ++j) best = fmin(best, sq_dist(qx, qy, qz, tile + 3 * j));
    }
    if (active) {
        dist[i] = sqrt(best);
        if (d2_out) d2_out[i] = best;
    }
}

// ------------------------------------------------------------------------------------------------ host
// the parameters, the bound partials, the sort over n pairs (its sums also scan the n segment flags), the flags and the run starts
struct CloudLayout {
    uint32_t n_cap;
    size_t params, part, flags, starts, total;
    SortLayout sort;
};
CloudLayout cloud_layout(int64_t n) {
    CloudLayout l;
    l.n_cap = (uint32_t)n;
    l.params = 0;
    l.part = align256(sizeof(CloudParams));
    l.sort = sort_layout(l.part + 6 * sizeof(double) * CL_BOUND_BLOCKS, n, (uint64_t)n);
    l.flags = l.sort.end;
    l.starts = align256(l.flags + 4 * (size_t)n);
    l.total = align256(l.starts + 4 * ((size_t)n + 1));
    return l;
}

// bound -> parameters -> keys -> sort -> segment starts, on `ws`; params at `p`
int sort_cloud(const char* what, const double* pts, int64_t n, const int32_t* n_dev, int mode, double edge, char* ws, const CloudLayout& l,
               CloudParams* p, hipStream_t st) {
    if (int rc = clear_words(p, sizeof(CloudParams), st, what, "parameters")) return rc;
    if (n == 0) {
        hipLaunchKernelGGL(cloud_params, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)(ws + l.part), 0, n_dev, 0u, mode, edge, p);
        LNR_CHECK_LAUNCH(what);
        return LNR_OK;
    }
    const uint32_t n_cap = l.n_cap;
    const int nbr = (int)(blocks_for(n) < CL_BOUND_BLOCKS ? blocks_for(n) : CL_BOUND_BLOCKS);
    const RadixBuffers r = radix_buffers(ws, l.sort);
    hipLaunchKernelGGL(bound_partial, dim3(nbr), dim3(CL_BLOCK), 0, st, pts, n_dev, n_cap, (double*)(ws + l.part), p);
    hipLaunchKernelGGL(cloud_params, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)(ws + l.part), nbr, n_dev, n_cap, mode, edge, p);
    hipLaunchKernelGGL(cloud_keys, dim3(blocks_for(n_cap)), dim3(CL_BLOCK), 0, st, pts, p, r.ka, r.ia);
    LNR_CHECK_LAUNCH(what);
    enqueue_radix_sort(r, &p->n, &p->npasses, st);
    LNR_CHECK_LAUNCH(what);
    uint32_t* flags = (uint32_t*)(ws + l.flags);
    hipLaunchKernelGGL(segment_heads, dim3(blocks_for(n_cap)), dim3(CL_BLOCK), 0, st, sorted_pairs(r), p, n_cap, flags);
    enqueue_scan(flags, n_cap, r.sums, &p->n_seg, nullptr, 0, st);
    hipLaunchKernelGGL(segment_starts, dim3(blocks_for(n_cap)), dim3(CL_BLOCK), 0, st, sorted_pairs(r), p, flags,
                       (uint32_t*)(ws + l.starts));
    LNR_CHECK_LAUNCH(what);
    return LNR_OK;
}

}  // namespace

extern "C" size_t lnr_cloud_workspace(int64_t n_points) {
    if (!count_ok(n_points)) return 0;
    return cloud_layout(n_points).total;
}

extern "C" size_t lnr_nn_grid_bytes(int64_t n_targets) {
    if (!count_ok(n_targets)) return 0;
    return grid_layout(n_targets).total;
}

extern "C" int lnr_lidar_scan_points(const float* depth, const float* variance, const int64_t* ray_index, int64_t n_rays,
                                     const float* directions, int64_t n_directions, float scale, float var_max, float depth_max,
                                     void* workspace, size_t workspace_bytes, double* points, int32_t* n_points_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_lidar_scan_points", n_rays, "rays");
    LNR_REQUIRE(n_directions >= 0 && n_directions < ((int64_t)1 << 40), "lnr_lidar_scan_points: bad direction count");
    LNR_REQUIRE(n_points_dev && (n_rays == 0 || (depth && variance && ray_index && directions && points && workspace)),
                "lnr_lidar_scan_points: null argument");
    const CloudLayout l = cloud_layout(n_rays);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_lidar_scan_points: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = clear_words(n_points_dev, sizeof(int32_t), st, "lnr_lidar_scan_points", "count")) return rc;
    if (n_rays == 0) return LNR_OK;
    LnrProfScope prof("lidar_scan_points", st);
    char* ws = (char*)workspace;
    uint32_t* flags = (uint32_t*)(ws + l.flags);
    const uint32_t m = (uint32_t)n_rays;
    hipLaunchKernelGGL(scan_flags, dim3(blocks_for(m)), dim3(CL_BLOCK), 0, st, depth, variance, m, scale, var_max, depth_max, flags);
    enqueue_scan(flags, m, (uint32_t*)(ws + l.sort.sums), (uint32_t*)n_points_dev, nullptr, 0, st);
    hipLaunchKernelGGL(scan_emit, dim3(blocks_for(m)), dim3(CL_BLOCK), 0, st, depth, variance, ray_index, directions, n_directions, m, scale,
                       var_max, depth_max, flags, points);
    LNR_CHECK_LAUNCH("lnr_lidar_scan_points");
    return LNR_OK;
}

extern "C" int lnr_voxel_down_sample(const double* points, int64_t n_points, const int32_t* n_points_dev, double voxel_size,
                                     void* workspace, size_t workspace_bytes, double* out, int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_voxel_down_sample", n_points, "points");
    LNR_REQUIRE(isfinite(voxel_size) && voxel_size > 0.0, "lnr_voxel_down_sample: voxel_size must be finite and > 0, got %g", voxel_size);
    LNR_REQUIRE(info_dev && workspace && (n_points == 0 || (points && out)), "lnr_voxel_down_sample: null argument");
    const CloudLayout l = cloud_layout(n_points);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_voxel_down_sample: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("voxel_down_sample", st);
    char* ws = (char*)workspace;
    CloudParams* p = (CloudParams*)(ws + l.params);
    if (int rc = sort_cloud("lnr_voxel_down_sample", points, n_points, n_points_dev, CL_MODE_VOXEL, voxel_size, ws, l, p, st)) return rc;
    if (n_points > 0) {
        hipLaunchKernelGGL(voxel_average, dim3(blocks_for(n_points)), dim3(CL_BLOCK), 0, st, points, (const uint32_t*)(ws + l.sort.ia),
                           (const uint32_t*)(ws + l.sort.ib), p, (const uint32_t*)(ws + l.starts), out);
    }
    hipLaunchKernelGGL(cloud_info, dim3(1), dim3(1), 0, st, p, info_dev);
    LNR_CHECK_LAUNCH("lnr_voxel_down_sample");
    return LNR_OK;
}

extern "C" int lnr_cloud_append_transformed(const double* src, int64_t n_points, const double* transform, double* dst, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_append_transformed", n_points, "points");
    LNR_REQUIRE(transform && (n_points == 0 || (src && dst)), "lnr_cloud_append_transformed: null argument");
    Affine T;
    const int bad = affine_from_host(transform, &T);
    LNR_REQUIRE(bad < 0, "lnr_cloud_append_transformed: non-finite transform entry %d", bad);
    if (n_points == 0) return LNR_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(append_transformed, dim3(blocks_for(n_points)), dim3(CL_BLOCK), 0, st, src, (uint32_t)n_points, T, dst);
    LNR_CHECK_LAUNCH("lnr_cloud_append_transformed");
    return LNR_OK;
}

extern "C" int lnr_nn_grid_build(const double* targets, int64_t n_targets, double cell_edge, void* workspace, size_t workspace_bytes,
                                 void* grid, size_t grid_bytes, int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_nn_grid_build", n_targets, "targets");
    LNR_REQUIRE(!(cell_edge > 0.0) || isfinite(cell_edge), "lnr_nn_grid_build: cell_edge must be finite (or <= 0 for the default)");
    LNR_REQUIRE(info_dev && workspace && grid && (n_targets == 0 || targets), "lnr_nn_grid_build: null argument");
    const CloudLayout l = cloud_layout(n_targets);
    const GridLayout g = grid_layout(n_targets);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_nn_grid_build: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    LNR_REQUIRE(grid_bytes >= g.total, "lnr_nn_grid_build: grid of %zu bytes, %zu needed", grid_bytes, g.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("nn_grid_build", st);
    char* ws = (char*)workspace;
    char* gb = (char*)grid;
    CloudParams* p = (CloudParams*)(gb + g.params);
    if (int rc = sort_cloud("lnr_nn_grid_build", targets, n_targets, nullptr, CL_MODE_GRID, cell_edge > 0.0 ? cell_edge : 0.0, ws, l, p, st))
        return rc;
    hipLaunchKernelGGL(grid_fill, dim3(blocks_for(n_targets + 1)), dim3(CL_BLOCK), 0, st, targets, sorted_pairs(radix_buffers(ws, l.sort)), p,
                       (const uint32_t*)(ws + l.starts), (double*)(gb + g.pts), (uint64_t*)(gb + g.cell_key), (uint32_t*)(gb + g.cell_start),
                       (uint32_t*)(gb + g.orig));
    hipLaunchKernelGGL(cloud_info, dim3(1), dim3(1), 0, st, p, info_dev);
    LNR_CHECK_LAUNCH("lnr_nn_grid_build");
    return LNR_OK;
}

extern "C" int lnr_nn_distance(const void* grid, int64_t n_targets, const double* queries, int64_t n_queries, double* distance,
                               double* sq_distance, void* workspace, size_t workspace_bytes, int64_t* counters_dev, void* stream) {
    CL_REQUIRE_COUNTS("lnr_nn_distance", n_targets, "targets", n_queries, "queries");
    LNR_REQUIRE(grid && counters_dev && workspace && (n_queries == 0 || (queries && distance)), "lnr_nn_distance: null argument");
    const size_t need = lnr_cloud_workspace(n_queries);
    LNR_REQUIRE(workspace_bytes >= need, "lnr_nn_distance: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = clear_words(counters_dev, 4 * sizeof(int64_t), st, "lnr_nn_distance", "counters")) return rc;
    if (n_queries == 0) return LNR_OK;
    LnrProfScope prof("nn_distance", st);
    const GridView g = grid_view(grid, n_targets);
    uint32_t* fb = (uint32_t*)workspace;
    unsigned long long* cnt = (unsigned long long*)counters_dev;
    const uint32_t nq = (uint32_t)n_queries;
    hipLaunchKernelGGL(nn_shells, dim3(blocks_for(nq)), dim3(CL_BLOCK), 0, st, g, queries, nq, distance, sq_distance, fb, cnt);
    hipLaunchKernelGGL(nn_brute, dim3(blocks_for(nq)), dim3(CL_BLOCK), 0, st, g, queries, (const uint32_t*)fb, (const unsigned long long*)cnt,
                       distance, sq_distance);
    LNR_CHECK_LAUNCH("lnr_nn_distance");
    return LNR_OK;
}
