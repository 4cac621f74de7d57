// Mesh clean-up (gfx950): connected components over shared edges, per-cluster area, the compaction behind every filter, and vertex
// normals: what a user of open3d's TriangleMesh calls between extracting a mesh and scoring or viewing it.
//   TriangleMesh::ClusterConnectedTriangles                          lnr_mesh_connected_triangles, lnr_mesh_cluster_area
//   RemoveTrianglesByMask, RemoveVerticesByMask,
//   RemoveUnreferencedVertices, RemoveDegenerateTriangles, Crop      lnr_mesh_select
//   ComputeVertexNormals (as TriangleMesh.compute_vertex_normals)    lnr_mesh_vertex_normals
// with the definitions stated in include/loner_hip.h ("mesh tools").  This file is compiled with -ffp-contract=off (build.py EXACT):
// every fp64 expression below rounds operation by operation, as the numpy restatement (tests/mesh_tools_restatement.py) does.  Float
// results take no atomics: their order is a function of the mesh.  The integer atomics (union-find, histogram, status) commute.
//   components keys (lo << b | hi, b the bit length of V - 1) of the 3 F edges with the triangle as payload, the stable sort of
//              lnr_radix_sort.h, then a union-find over triangles: equal neighbouring keys are united, the larger root hooked under the
//              smaller by compare-and-swap; a failed swap means another lane hooked that root, and the loop goes on from what it found
//              there (no lane waits for another).  A root is therefore its component's smallest triangle, and the exclusive scan of
//              the root flags numbers the clusters by first triangle
//   area       the triangles sorted by cluster (stable: ascending index within one), the areas gathered in that order, and per run a
//              64-ary tree in place: level l sums 64 partials 64^l apart, left to right
//   select     keep flags per triangle and vertex, their exclusive scans, and the emit through the vertex scan
//   normals    keys (vertex << 2 | corner) with the triangle as payload, sorted; the thread at the head of a vertex's run walks it
#include "lnr_mesh_head.h"
#include "lnr_union_find.h"

namespace {

// the head's words here: status MT_ST_*, n_a a scan's total (clusters, or surviving vertices), n_b the surviving triangles
enum { MT_ST_BAD_INDEX = 1, MT_ST_BAD_CLUSTER = 2 };

#define MT_ARITY 64
#define MT_NONE 0xFFFFFFFFu

// ------------------------------------------------------------------------------------------------ connected components
__global__ __launch_bounds__(CL_BLOCK) void cc_keys(const int32_t* __restrict__ tri, uint32_t n_tris, int64_t n_verts, uint32_t shift,
                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ idx, uint32_t* __restrict__ parent,
                                                    MeshSortHead* h) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    int64_t i[3];
    const bool ok = load_corners(tri, t, n_verts, i);
    parent[t] = t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t a = (uint64_t)i[k], b = (uint64_t)i[(k + 1) % 3];
        keys[3 * (size_t)t + k] = ok ? ((a < b ? a : b) << shift) | (a < b ? b : a) : 0ull;
        idx[3 * (size_t)t + k] = t;
    }
    if (!ok) atomicOr(&h->status, (uint32_t)MT_ST_BAD_INDEX);
}

__global__ __launch_bounds__(CL_BLOCK) void cc_link(SortedPairs sp, uint32_t* __restrict__ parent, const MeshSortHead* __restrict__ h) {
    const uint64_t j = (uint64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (j == 0 || j >= h->n || h->status) return;
    const uint64_t* keys = sp.keys(h->npasses);
    if (keys[j] != keys[j - 1]) return;
    const uint32_t* idx = sp.idx(h->npasses);
    uf_unite(parent, idx[j], idx[j - 1]);
}

// root[t] and flag[t] = (t is a root); no hook runs beside this kernel, so a root found is final
__global__ __launch_bounds__(CL_BLOCK) void cc_flatten(uint32_t* __restrict__ parent, uint32_t n_tris, uint32_t* __restrict__ root,
                                                       uint32_t* __restrict__ flag) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    const uint32_t r = uf_find(parent, t);
    root[t] = r;
    flag[t] = r == t ? 1u : 0u;
}

// cluster[t] = rank of t's root among the roots; sizes += 1, one atomic per wave and distinct cluster
__global__ __launch_bounds__(CL_BLOCK) void cc_labels(const uint32_t* __restrict__ root, const uint32_t* __restrict__ rank, uint32_t n_tris,
                                                      int32_t* __restrict__ cluster, int32_t* __restrict__ sizes) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool active = t < n_tris;
    const uint32_t c = active ? rank[root[t]] : MT_NONE;
    if (active) cluster[t] = (int32_t)c;
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    while (todo) {                                                      // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t cl = __shfl(c, leader, 64);
        const unsigned long long same = __ballot(active && c == cl);
        if (lane == leader) atomicAdd(&sizes[cl], (int32_t)__popcll(same));
        todo &= ~same;
    }
}

// ------------------------------------------------------------------------------------------------ cluster area
__device__ inline double triangle_area(const double* __restrict__ v, const int64_t* i) {
    const double *p0 = v + 3 * (size_t)i[0], *p1 = v + 3 * (size_t)i[1], *p2 = v + 3 * (size_t)i[2];
    const double ux = p0[0] - p1[0], uy = p0[1] - p1[1], uz = p0[2] - p1[2];
    const double wx = p0[0] - p2[0], wy = p0[1] - p2[1], wz = p0[2] - p2[2];
    const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

__global__ __launch_bounds__(CL_BLOCK) void ca_keys(const int32_t* __restrict__ tri, uint32_t n_tris, int64_t n_verts,
                                                    const int32_t* __restrict__ cluster, int64_t n_clusters, uint64_t* __restrict__ keys,
                                                    uint32_t* __restrict__ idx, MeshSortHead* h) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    int64_t i[3];
    const bool ok = load_corners(tri, t, n_verts, i);
    const int64_t c = cluster[t];
    const bool c_ok = c >= 0 && c < n_clusters;
    keys[t] = c_ok ? (uint64_t)c : 0ull;
    idx[t] = t;
    if (!ok || !c_ok) atomicOr(&h->status, (uint32_t)((ok ? 0 : MT_ST_BAD_INDEX) | (c_ok ? 0 : MT_ST_BAD_CLUSTER)));
}

// part[j] = area of the j-th triangle in (cluster, index) order; start[c] = the first j of cluster c
__global__ __launch_bounds__(CL_BLOCK) void ca_gather(const double* __restrict__ v, int64_t n_verts, const int32_t* __restrict__ tri,
                                                      const uint64_t* __restrict__ ka, const uint64_t* __restrict__ kb,
                                                      const uint32_t* __restrict__ ia, const uint32_t* __restrict__ ib,
                                                      const MeshSortHead* __restrict__ h, double* __restrict__ part,
                                                      uint32_t* __restrict__ start) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (j >= h->n || h->status) return;
    const uint64_t* keys = sorted_keys(h->npasses, ka, kb);
    const uint32_t t = sorted_idx(h->npasses, ia, ib)[j];
    int64_t i[3];
    load_corners(tri, t, n_verts, i);                                   // in range: the status is clear
    part[j] = triangle_area(v, i);
    if (j == 0 || keys[j - 1] != keys[j]) start[keys[j]] = j;
}

// one level of the tree: the thread at run position r, r a multiple of 64 stride, sums the partials at r, r + stride, ... (at most 64,
// within its run) left to right into part[r].  No thread of a level reads what another one writes: the targets are multiples of
// 64 stride, the other terms are not
__global__ __launch_bounds__(CL_BLOCK) void ca_level(SortedPairs sp, const MeshSortHead* __restrict__ h, const uint32_t* __restrict__ start,
                                                     double* __restrict__ part, uint64_t stride) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    const uint32_t n = h->n;
    if (j >= n || h->status) return;
    const uint64_t* keys = sp.keys(h->npasses);
    const uint64_t c = keys[j];
    if ((uint64_t)(j - start[c]) % (MT_ARITY * stride)) return;
    double s = part[j];
    for (int q = 1; q < MT_ARITY; ++q) {
        const uint64_t jj = (uint64_t)j + (uint64_t)q * stride;
        if (jj >= n || keys[jj] != c) break;
        s = s + part[jj];
    }
    part[j] = s;
}

__global__ __launch_bounds__(CL_BLOCK) void ca_out(const MeshSortHead* __restrict__ h, const uint32_t* __restrict__ start,
                                                   const double* __restrict__ part, uint32_t n_clusters, double* __restrict__ area) {
    const uint32_t c = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (c >= n_clusters) return;
    area[c] = h->status || start[c] == MT_NONE ? 0.0 : part[start[c]];
}

// ------------------------------------------------------------------------------------------------ select
// tflag[t] = the triangle survives; with drop_unreferenced, vflag[i] = 1 for its corners (all lanes store the same word)
__global__ __launch_bounds__(CL_BLOCK) void sel_triangles(const int32_t* __restrict__ tri, uint32_t n_tris, int64_t n_verts,
                                                          const uint8_t* __restrict__ tri_keep, const uint8_t* __restrict__ vert_keep,
                                                          int drop_unreferenced, uint32_t* __restrict__ tflag, uint32_t* __restrict__ vflag,
                                                          MeshSortHead* h) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    int64_t i[3];
    const bool ok = load_corners(tri, t, n_verts, i);
    bool keep = ok && (!tri_keep || tri_keep[t]);
    if (keep && vert_keep) keep = vert_keep[i[0]] && vert_keep[i[1]] && vert_keep[i[2]];
    tflag[t] = keep ? 1u : 0u;
    if (keep && drop_unreferenced) {
        vflag[i[0]] = 1u;
        vflag[i[1]] = 1u;
        vflag[i[2]] = 1u;
    }
    if (!ok) atomicOr(&h->status, (uint32_t)MT_ST_BAD_INDEX);
}

__global__ __launch_bounds__(CL_BLOCK) void sel_vertices(uint32_t n_verts, const uint8_t* __restrict__ vert_keep, int drop_unreferenced,
                                                         uint32_t* __restrict__ vflag) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n_verts) return;
    const bool keep = (!vert_keep || vert_keep[i]) && (!drop_unreferenced || vflag[i]);
    vflag[i] = keep ? 1u : 0u;
}

// vrank / trank: the exclusive scans of the flags; an element survives when the next rank (or the total) is larger
__global__ __launch_bounds__(CL_BLOCK) void sel_emit_vertices(const uint32_t* __restrict__ vrank, uint32_t n_verts,
                                                              const MeshSortHead* __restrict__ h, int32_t* __restrict__ vertex_map) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n_verts) return;
    const uint32_t r = vrank[i], next = i + 1 < n_verts ? vrank[i + 1] : h->n_a;
    vertex_map[i] = next != r ? (int32_t)r : -1;
}

__global__ __launch_bounds__(CL_BLOCK) void sel_emit_triangles(const int32_t* __restrict__ tri, const uint32_t* __restrict__ trank,
                                                               uint32_t n_tris, const uint32_t* __restrict__ vrank,
                                                               const MeshSortHead* __restrict__ h, int32_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    const uint32_t r = trank[t], next = t + 1 < n_tris ? trank[t + 1] : h->n_b;
    if (next == r) return;                                              // dropped; a survivor's corners are in range
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * (size_t)r + k] = (int32_t)vrank[tri[3 * (size_t)t + k]];
}

// ------------------------------------------------------------------------------------------------ vertex normals
__global__ __launch_bounds__(CL_BLOCK) void vn_keys(const int32_t* __restrict__ tri, uint32_t n_tris, int64_t n_verts,
                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ idx, MeshSortHead* h) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    int64_t i[3];
    const bool ok = load_corners(tri, t, n_verts, i);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        keys[3 * (size_t)t + k] = ok ? ((uint64_t)i[k] << 2) | (uint64_t)k : 0ull;
        idx[3 * (size_t)t + k] = t;
    }
    if (!ok) atomicOr(&h->status, (uint32_t)MT_ST_BAD_INDEX);
}

// the thread at the head of vertex v's run: the face normals of the run's triangles added one after the other to 0.0, in the run's
// order (corner slot, then triangle index), then the division by the norm
__global__ __launch_bounds__(CL_BLOCK) void vn_walk(const double* __restrict__ v, int64_t n_verts, const int32_t* __restrict__ tri,
                                                    SortedPairs sp, const MeshSortHead* __restrict__ h, double* __restrict__ normals) {
    const uint64_t j = (uint64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
    const uint32_t n = h->n;
    if (j >= n || h->status) return;
    const uint64_t* keys = sp.keys(h->npasses);
    const uint64_t vert = keys[j] >> 2;
    if (j > 0 && (keys[j - 1] >> 2) == vert) return;
    const uint32_t* idx = sp.idx(h->npasses);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint64_t jj = j; jj < n && (keys[jj] >> 2) == vert; ++jj) {
        int64_t i[3];
        load_corners(tri, idx[jj], n_verts, i);                         // in range: the status is clear
        const double *p0 = v + 3 * (size_t)i[0], *p1 = v + 3 * (size_t)i[1], *p2 = v + 3 * (size_t)i[2];
        const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        sx = sx + (ay * bz - az * by);
        sy = sy + (az * bx - ax * bz);
        sz = sz + (ax * by - ay * bx);
    }
    const double norm = sqrt((sx * sx + sy * sy) + sz * sz);
    const double d = norm > 0.0 ? norm : 1.0;
    normals[3 * (size_t)vert] = sx / d;
    normals[3 * (size_t)vert + 1] = sy / d;
    normals[3 * (size_t)vert + 2] = sz / d;
}

// ------------------------------------------------------------------------------------------------ host
// One workspace for the four entries: the head, the sort over 3 F pairs (its sums also scan F and V flags), three arrays of F words or
// doubles, and V words.
struct ToolsLayout {
    size_t head, wa, wb, dbl, vw, total;
    SortLayout sort;
};
ToolsLayout tools_layout(int64_t n_verts, int64_t n_tris) {
    ToolsLayout l;
    l.head = 0;
    l.sort = sort_layout(sizeof(MeshSortHead), 3 * n_tris, (uint64_t)(n_tris > n_verts ? n_tris : n_verts));
    l.wa = l.sort.end;
    l.wb = align256(l.wa + 4 * (size_t)n_tris);
    l.dbl = align256(l.wb + 4 * (size_t)n_tris);
    l.vw = align256(l.dbl + 8 * (size_t)n_tris);
    l.total = align256(l.vw + 4 * (size_t)n_verts);
    return l;
}

const int64_t MT_MAX_TRIANGLES = CL_MAX_POINTS / 3;     // three pairs per triangle

}  // namespace

extern "C" size_t lnr_mesh_tools_workspace(int64_t n_vertices, int64_t n_triangles) {
    if (!mesh_counts_ok(n_vertices, n_triangles, MT_MAX_TRIANGLES)) return 0;
    return tools_layout(n_vertices, n_triangles).total;
}

extern "C" int lnr_mesh_connected_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* workspace,
                                            size_t workspace_bytes, int32_t* triangle_clusters, int32_t* cluster_n_triangles,
                                            int64_t* info_dev, void* stream) {
    MESH_REQUIRE_COUNTS("lnr_mesh_connected_triangles", n_vertices, n_triangles, MT_MAX_TRIANGLES);
    LNR_REQUIRE(info_dev && workspace && (n_triangles == 0 || (triangles && triangle_clusters && cluster_n_triangles)),
                "lnr_mesh_connected_triangles: null argument");
    const ToolsLayout l = tools_layout(0, n_triangles);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_mesh_connected_triangles: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("mesh_connected_triangles", st);
    char* ws = (char*)workspace;
    MeshSortHead* h = (MeshSortHead*)(ws + l.head);
    const uint32_t F = (uint32_t)n_triangles, n = 3 * F;
    const int shift = (int)bit_length(n_vertices - 1);
    const int32_t npasses = (2 * shift + 7) / 8;
    hipLaunchKernelGGL(mesh_head_init, dim3(1), dim3(1), 0, st, h, n, npasses, 0);
    if (F) {
        const RadixBuffers r = radix_buffers(ws, l.sort);
        uint32_t *parent = (uint32_t*)(ws + l.wa), *root = (uint32_t*)(ws + l.wb), *flag = (uint32_t*)(ws + l.dbl);
        if (int rc = clear_words(cluster_n_triangles, 4 * (size_t)F, st, "lnr_mesh_connected_triangles", "cluster sizes")) return rc;
        hipLaunchKernelGGL(cc_keys, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, triangles, F, n_vertices, (uint32_t)shift, r.ka, r.ia, parent, h);
        LNR_CHECK_LAUNCH("lnr_mesh_connected_triangles");
        enqueue_radix_sort(r, &h->n, &h->npasses, st);
        hipLaunchKernelGGL(cc_link, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, sorted_pairs(r), parent, (const MeshSortHead*)h);
        hipLaunchKernelGGL(cc_flatten, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, parent, F, root, flag);
        enqueue_scan(flag, F, r.sums, &h->n_a, nullptr, 0, st);
        hipLaunchKernelGGL(cc_labels, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, (const uint32_t*)root, (const uint32_t*)flag, F,
                           triangle_clusters, cluster_n_triangles);
    }
    hipLaunchKernelGGL(mesh_head_info, dim3(1), dim3(1), 0, st, (const MeshSortHead*)h, info_dev, (int64_t)npasses);
    LNR_CHECK_LAUNCH("lnr_mesh_connected_triangles");
    return LNR_OK;
}

extern "C" int lnr_mesh_cluster_area(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                     const int32_t* triangle_clusters, int64_t n_clusters, void* workspace, size_t workspace_bytes,
                                     double* cluster_area, int64_t* info_dev, void* stream) {
    MESH_REQUIRE_COUNTS("lnr_mesh_cluster_area", n_vertices, n_triangles, MT_MAX_TRIANGLES);
    LNR_REQUIRE(n_clusters >= 0 && n_clusters <= n_triangles, "lnr_mesh_cluster_area: %lld clusters of %lld triangles", (long long)n_clusters,
                (long long)n_triangles);
    LNR_REQUIRE(info_dev && workspace && (n_triangles == 0 || (triangles && triangle_clusters)) && (n_vertices == 0 || vertices) &&
                    (n_clusters == 0 || cluster_area),
                "lnr_mesh_cluster_area: null argument");
    const ToolsLayout l = tools_layout(0, n_triangles);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_mesh_cluster_area: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("mesh_cluster_area", st);
    char* ws = (char*)workspace;
    MeshSortHead* h = (MeshSortHead*)(ws + l.head);
    const uint32_t F = (uint32_t)n_triangles, C = (uint32_t)n_clusters;
    const int32_t npasses = (int32_t)((bit_length(n_clusters - 1) + 7) / 8);
    hipLaunchKernelGGL(mesh_head_init, dim3(1), dim3(1), 0, st, h, F, npasses, 0);
    if (F && C) {
        const RadixBuffers r = radix_buffers(ws, l.sort, F);            // F pairs in buffers laid out for 3 F
        uint32_t* start = (uint32_t*)(ws + l.wa);
        double* part = (double*)(ws + l.dbl);
        if (hipMemsetAsync(start, 0xFF, 4 * (size_t)F, st) != hipSuccess) {
            lnr_set_error("lnr_mesh_cluster_area: clearing the run starts failed");
            return LNR_ERR_LAUNCH;
        }
        hipLaunchKernelGGL(ca_keys, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, triangles, F, n_vertices, triangle_clusters, n_clusters, r.ka,
                           r.ia, h);
        LNR_CHECK_LAUNCH("lnr_mesh_cluster_area");
        enqueue_radix_sort(r, &h->n, &h->npasses, st);
        hipLaunchKernelGGL(ca_gather, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, vertices, n_vertices, triangles, (const uint64_t*)r.ka,
                           (const uint64_t*)r.kb, (const uint32_t*)r.ia, (const uint32_t*)r.ib, (const MeshSortHead*)h, part, start);
        for (uint64_t stride = 1; stride < F; stride *= MT_ARITY)
            hipLaunchKernelGGL(ca_level, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, sorted_pairs(r), (const MeshSortHead*)h,
                               (const uint32_t*)start, part, stride);
        hipLaunchKernelGGL(ca_out, dim3(blocks_for(C)), dim3(CL_BLOCK), 0, st, (const MeshSortHead*)h, (const uint32_t*)start,
                           (const double*)part, C, cluster_area);
    }
    hipLaunchKernelGGL(mesh_head_info, dim3(1), dim3(1), 0, st, (const MeshSortHead*)h, info_dev, (int64_t)npasses);
    LNR_CHECK_LAUNCH("lnr_mesh_cluster_area");
    return LNR_OK;
}

extern "C" int lnr_mesh_select(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const uint8_t* triangle_keep,
                               const uint8_t* vertex_keep, int32_t drop_unreferenced, void* workspace, size_t workspace_bytes,
                               int32_t* triangles_out, int32_t* vertex_map, int64_t* info_dev, void* stream) {
    MESH_REQUIRE_COUNTS("lnr_mesh_select", n_vertices, n_triangles, MT_MAX_TRIANGLES);
    LNR_REQUIRE(info_dev && workspace && (n_triangles == 0 || (triangles && triangles_out)) && (n_vertices == 0 || vertex_map),
                "lnr_mesh_select: null argument");
    const ToolsLayout l = tools_layout(n_vertices, n_triangles);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_mesh_select: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("mesh_select", st);
    char* ws = (char*)workspace;
    MeshSortHead* h = (MeshSortHead*)(ws + l.head);
    const uint32_t F = (uint32_t)n_triangles, V = (uint32_t)n_vertices;
    uint32_t *tflag = (uint32_t*)(ws + l.wa), *vflag = (uint32_t*)(ws + l.vw), *sums = (uint32_t*)(ws + l.sort.sums);
    hipLaunchKernelGGL(mesh_head_init, dim3(1), dim3(1), 0, st, h, 0u, 0, 0);
    if (V) {
        if (int rc = clear_words(vflag, 4 * (size_t)V, st, "lnr_mesh_select", "vertex flags")) return rc;
    }
    if (F)
        hipLaunchKernelGGL(sel_triangles, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, triangles, F, n_vertices, triangle_keep, vertex_keep,
                           (int)drop_unreferenced, tflag, vflag, h);
    if (V) {
        hipLaunchKernelGGL(sel_vertices, dim3(blocks_for(V)), dim3(CL_BLOCK), 0, st, V, vertex_keep, (int)drop_unreferenced, vflag);
        enqueue_scan(vflag, V, sums, &h->n_a, nullptr, 0, st);
        hipLaunchKernelGGL(sel_emit_vertices, dim3(blocks_for(V)), dim3(CL_BLOCK), 0, st, (const uint32_t*)vflag, V, (const MeshSortHead*)h,
                           vertex_map);
    }
    if (F) {
        enqueue_scan(tflag, F, sums, &h->n_b, nullptr, 0, st);
        hipLaunchKernelGGL(sel_emit_triangles, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, triangles, (const uint32_t*)tflag, F,
                           (const uint32_t*)vflag, (const MeshSortHead*)h, triangles_out);
    }
    hipLaunchKernelGGL(mesh_head_info, dim3(1), dim3(1), 0, st, (const MeshSortHead*)h, info_dev, (int64_t)0);
    LNR_CHECK_LAUNCH("lnr_mesh_select");
    return LNR_OK;
}

extern "C" int lnr_mesh_vertex_normals(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                       void* workspace, size_t workspace_bytes, double* normals, int64_t* info_dev, void* stream) {
    MESH_REQUIRE_COUNTS("lnr_mesh_vertex_normals", n_vertices, n_triangles, MT_MAX_TRIANGLES);
    LNR_REQUIRE(info_dev && workspace && (n_triangles == 0 || triangles) && (n_vertices == 0 || (vertices && normals)),
                "lnr_mesh_vertex_normals: null argument");
    const ToolsLayout l = tools_layout(0, n_triangles);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_mesh_vertex_normals: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("mesh_vertex_normals", st);
    char* ws = (char*)workspace;
    MeshSortHead* h = (MeshSortHead*)(ws + l.head);
    const uint32_t F = (uint32_t)n_triangles, n = 3 * F;
    const int32_t npasses = (int32_t)((bit_length(n_vertices - 1) + 2 + 7) / 8);
    hipLaunchKernelGGL(mesh_head_init, dim3(1), dim3(1), 0, st, h, n, npasses, 0);
    if (n_vertices) {
        if (int rc = clear_words(normals, 24 * (size_t)n_vertices, st, "lnr_mesh_vertex_normals", "normals")) return rc;
    }
    if (F) {
        const RadixBuffers r = radix_buffers(ws, l.sort);
        hipLaunchKernelGGL(vn_keys, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, triangles, F, n_vertices, r.ka, r.ia, h);
        LNR_CHECK_LAUNCH("lnr_mesh_vertex_normals");
        enqueue_radix_sort(r, &h->n, &h->npasses, st);
        hipLaunchKernelGGL(vn_walk, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, vertices, n_vertices, triangles, sorted_pairs(r),
                           (const MeshSortHead*)h, normals);
    }
    hipLaunchKernelGGL(mesh_head_info, dim3(1), dim3(1), 0, st, (const MeshSortHead*)h, info_dev, (int64_t)npasses);
    LNR_CHECK_LAUNCH("lnr_mesh_vertex_normals");
    return LNR_OK;
}
