// Mesh simplification and smoothing (gfx950): what a user of open3d's TriangleMesh calls on an extracted mesh before viewing, shipping
// or scoring it.
//   SimplifyVertexClustering (Average), the vertex half                 lnr_mesh_vertex_clusters
//   RemoveDuplicatedTriangles, and the triangle half of the above       lnr_mesh_unique_triangles
//   the adjacency list of FilterSmooth*                                 lnr_mesh_vertex_adjacency
//   FilterSmoothSimple, FilterSmoothLaplacian, FilterSmoothTaubin       lnr_mesh_smooth
// with the definitions stated in include/loner_hip.h ("mesh simplification and smoothing").  This file is compiled with
// -ffp-contract=off (build.py EXACT): every fp64 expression below rounds operation by operation, as the numpy restatement
// (tests/mesh_filters_restatement.py) does.  Float results take no atomics: their order is a function of the mesh.  The integer atomics
// (counts, status) commute.
//   clusters   the voxel key of lnr_voxel_down_sample (lnr_cloud_keys.h) with the vertex as payload and the stable sort: a voxel's run
//              is in ascending vertex index, so its head is the voxel's first occurrence.  The heads are flagged per vertex, the
//              exclusive scan of the flags numbers the clusters, and the thread at the head of a run labels and sums it
//   unique     the canonical triple (a, b, c) per triangle, sorted by two stable passes of the sort: by c, then by (a, b) with the keys
//              rebuilt in the first pass's order.  Equal triples are then neighbours in ascending triangle index
//   adjacency  the six directed pairs of a triangle as keys (i << b | j), sorted; a key that differs from its predecessor is a
//              neighbour, the exclusive scan of those flags its place, and one binary search per vertex its row's start
//   smooth     one thread per vertex walks its row; one launch per step, ping-ponging so that the last step writes the caller's array
#include "lnr_cloud_keys.h"
#include "lnr_mesh_head.h"

namespace {

// the head's words here: status MF_ST_*, n_a the kept triangles or the neighbours, n_b the degenerate triangles; npasses2 is the second
// sort of the unique triangles
enum { MF_ST_BAD_INDEX = 1 };

// ------------------------------------------------------------------------------------------------ vertex clusters
// first[v] = 1 where v heads a voxel's run: the voxel's lowest vertex index
__global__ __launch_bounds__(CL_BLOCK) void vc_first(SortedPairs sp, const CloudParams* __restrict__ p, uint32_t* __restrict__ first) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (j >= p->n) return;
    const uint64_t* k = sp.keys(p->npasses);
    if (j == 0 || k[j] != k[j - 1]) first[sp.idx(p->npasses)[j]] = 1u;
}

// rank: the exclusive scan of first.  The thread at the head of a run: the cluster is its vertex's rank; every vertex of the run gets
// the label, and the run is summed in its order (ascending vertex index) and divided by the count
__global__ __launch_bounds__(CL_BLOCK) void vc_walk(const double* __restrict__ v, SortedPairs sp, const CloudParams* __restrict__ p,
                                                    const uint32_t* __restrict__ rank, int32_t* __restrict__ vertex_cluster,
                                                    double* __restrict__ cluster_vertices) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    const uint32_t n = p->n;
    if (j >= n) return;
    const uint64_t* k = sp.keys(p->npasses);
    const uint64_t key = k[j];
    if (j > 0 && k[j - 1] == key) return;
    const uint32_t* idx = sp.idx(p->npasses);
    const uint32_t c = rank[idx[j]];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    uint32_t jj = j;
    for (; jj < n && k[jj] == key; ++jj) {
        const uint32_t i = idx[jj];
        vertex_cluster[i] = (int32_t)c;
        sx = sx + v[3 * (size_t)i];
        sy = sy + v[3 * (size_t)i + 1];
        sz = sz + v[3 * (size_t)i + 2];
    }
    const double count = (double)(jj - j);
    cluster_vertices[3 * (size_t)c] = sx / count;
    cluster_vertices[3 * (size_t)c + 1] = sy / count;
    cluster_vertices[3 * (size_t)c + 2] = sz / count;
}

__global__ void vc_info(const CloudParams* __restrict__ p, int64_t* __restrict__ info) {
    info[0] = p->status;
    info[1] = p->n_seg;
    info[2] = (int64_t)p->nonfinite;
    info[3] = 0;
}

// ------------------------------------------------------------------------------------------------ unique triangles
// the canonical triple of triangle t (corners mapped, rotated), the first sort's key (its third entry) and the degenerate count
__global__ __launch_bounds__(CL_BLOCK) void ut_keys(const int32_t* __restrict__ tri, uint32_t n_tris, int64_t n_verts,
                                                    const int32_t* __restrict__ vertex_map, int64_t n_mapped,
                                                    int32_t* __restrict__ canonical, uint64_t* __restrict__ keys,
                                                    uint32_t* __restrict__ idx, MeshSortHead* h) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool active = t < n_tris;
    bool ok = false, degenerate = false;
    if (active) {
        int64_t m[3];
        ok = load_corners(tri, t, n_verts, m);
        if (ok) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (vertex_map) m[k] = vertex_map[m[k]];
                if (m[k] < 0 || m[k] >= n_mapped) ok = false;
            }
        }
        int64_t a = -1, b = -1, c = -1;
        if (ok) {
            if (m[0] <= m[1]) {
                if (m[0] <= m[2]) { a = m[0]; b = m[1]; c = m[2]; } else { a = m[2]; b = m[0]; c = m[1]; }
            } else {
                if (m[1] <= m[2]) { a = m[1]; b = m[2]; c = m[0]; } else { a = m[2]; b = m[0]; c = m[1]; }
            }
            degenerate = a == b || b == c || c == a;
        }
        canonical[3 * (size_t)t] = (int32_t)a;
        canonical[3 * (size_t)t + 1] = (int32_t)b;
        canonical[3 * (size_t)t + 2] = (int32_t)c;
        keys[t] = ok ? (uint64_t)c : 0ull;
        idx[t] = t;
        if (!ok) atomicOr(&h->status, (uint32_t)MF_ST_BAD_INDEX);
    }
    wave_count_add(degenerate, &h->n_b);
}

// the second sort's input, in the first sort's order: key (a << shift | b) and the triangle, into the a buffers.  Entry j is read and
// written by thread j only
__global__ __launch_bounds__(CL_BLOCK) void ut_rekey(const int32_t* __restrict__ canonical, uint64_t* ka, uint32_t* ia, const uint32_t* ib,
                                                     const MeshSortHead* __restrict__ h, uint32_t shift) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (j >= h->n) return;
    const uint32_t t = (h->npasses & 1) ? ib[j] : ia[j];
    const uint64_t a = (uint32_t)canonical[3 * (size_t)t] & 0x7FFFFFFFu, b = (uint32_t)canonical[3 * (size_t)t + 1] & 0x7FFFFFFFu;
    ka[j] = (a << shift) | b;
    ia[j] = t;
}

// after both sorts equal triples are neighbours, the lowest triangle index first
__global__ __launch_bounds__(CL_BLOCK) void ut_mark(const int32_t* __restrict__ canonical, SortedPairs sp, MeshSortHead* h, int drop_degenerate,
                                                    uint8_t* __restrict__ keep) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    bool kept = false;
    if (j < h->n) {
        const uint32_t* idx = sp.idx(h->npasses2);
        const uint32_t t = idx[j];
        const int32_t a = canonical[3 * (size_t)t], b = canonical[3 * (size_t)t + 1], c = canonical[3 * (size_t)t + 2];
        kept = h->status == 0;
        if (kept && j > 0) {
            const uint32_t u = idx[j - 1];
            kept = canonical[3 * (size_t)u] != a || canonical[3 * (size_t)u + 1] != b || canonical[3 * (size_t)u + 2] != c;
        }
        if (kept && drop_degenerate) kept = a != b && b != c && c != a;
        keep[t] = kept ? 1 : 0;
    }
    wave_count_add(kept, &h->n_a);
}

// ------------------------------------------------------------------------------------------------ vertex adjacency
// six keys per triangle: (i << shift | j) for both directions of its three edges; the key of row n_verts (past every real row) for a
// pair (i, i) and for a triangle with a corner out of range
__global__ __launch_bounds__(CL_BLOCK) void va_keys(const int32_t* __restrict__ tri, uint32_t n_tris, int64_t n_verts, uint32_t shift,
                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ idx, MeshSortHead* h) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    int64_t i[3];
    const bool ok = load_corners(tri, t, n_verts, i);
    const uint64_t none = (uint64_t)n_verts << shift;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t a = (uint64_t)i[k], b = (uint64_t)i[(k + 1) % 3];
        const bool valid = ok && a != b;
        keys[6 * (size_t)t + 2 * k] = valid ? (a << shift) | b : none;
        keys[6 * (size_t)t + 2 * k + 1] = valid ? (b << shift) | a : none;
        idx[6 * (size_t)t + 2 * k] = t;
        idx[6 * (size_t)t + 2 * k + 1] = t;
    }
    if (!ok) atomicOr(&h->status, (uint32_t)MF_ST_BAD_INDEX);
}

__device__ inline bool va_is_head(const uint64_t* keys, uint32_t j, uint64_t n_verts, uint32_t shift) {
    return (keys[j] >> shift) < n_verts && (j == 0 || keys[j] != keys[j - 1]);
}

__global__ __launch_bounds__(CL_BLOCK) void va_heads(const uint64_t* __restrict__ ka, const uint64_t* __restrict__ kb,
                                                     const MeshSortHead* __restrict__ h, uint64_t n_verts, uint32_t shift,
                                                     uint32_t* __restrict__ flags) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (j >= h->n) return;
    flags[j] = va_is_head(sorted_keys(h->npasses, ka, kb), j, n_verts, shift) ? 1u : 0u;
}

// rank: the exclusive scan of the flags
__global__ __launch_bounds__(CL_BLOCK) void va_emit(const uint64_t* __restrict__ ka, const uint64_t* __restrict__ kb,
                                                    const MeshSortHead* __restrict__ h, uint64_t n_verts, uint32_t shift,
                                                    const uint32_t* __restrict__ rank, int32_t* __restrict__ neighbours) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (j >= h->n) return;
    const uint64_t* keys = sorted_keys(h->npasses, ka, kb);
    if (va_is_head(keys, j, n_verts, shift)) neighbours[rank[j]] = (int32_t)(keys[j] & ((1ull << shift) - 1ull));
}

// row_start[r], r in [0, n_verts]: the neighbours of lower rows = the rank at the first sorted key not below (r << shift)
__global__ __launch_bounds__(CL_BLOCK) void va_rows(SortedPairs sp, const MeshSortHead* __restrict__ h, uint64_t n_verts, uint32_t shift,
                                                    const uint32_t* __restrict__ rank, int32_t* __restrict__ row_start) {
    const uint64_t r = (uint64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (r > n_verts) return;
    const uint64_t* keys = sp.keys(h->npasses);
    const uint64_t k0 = r << shift;
    const uint32_t n = h->n;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k0) lo = mid + 1; else hi = mid;
    }
    row_start[r] = (int32_t)(lo < n ? rank[lo] : h->n_a);
}

// ------------------------------------------------------------------------------------------------ smoothing
__global__ void sm_info(int64_t* info) {
    info[0] = 0;
    info[1] = 0;
    info[2] = 0;
    info[3] = 0;
}

// one step for vertex i: src -> dst.  A row or a neighbour out of range sets the status bit and leaves the vertex where it is
__global__ __launch_bounds__(CL_BLOCK) void sm_step(const double* __restrict__ src, double* __restrict__ dst, uint32_t n_verts,
                                                    const int32_t* __restrict__ row_start, const int32_t* __restrict__ neighbours,
                                                    int64_t n_neighbours, int kind, double f, int64_t* info) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n_verts) return;
    const double px = src[3 * (size_t)i], py = src[3 * (size_t)i + 1], pz = src[3 * (size_t)i + 2];
    const int64_t r0 = row_start[i], r1 = row_start[i + 1];
    bool ok = r0 >= 0 && r0 <= r1 && r1 <= n_neighbours;
    double ox = px, oy = py, oz = pz;
    if (ok && r1 > r0) {
        double sx, sy, sz, W = 0.0;
        if (kind == 0) { sx = px; sy = py; sz = pz; } else { sx = 0.0; sy = 0.0; sz = 0.0; }
        for (int64_t r = r0; r < r1; ++r) {
            const int64_t j = neighbours[r];
            if (j < 0 || j >= (int64_t)n_verts) { ok = false; break; }
            const double qx = src[3 * (size_t)j], qy = src[3 * (size_t)j + 1], qz = src[3 * (size_t)j + 2];
            if (kind == 0) {
                sx = sx + qx;
                sy = sy + qy;
                sz = sz + qz;
            } else {
                const double dx = px - qx, dy = py - qy, dz = pz - qz;
                const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
                const double w = 1.0 / (dist + 1e-12);
                W = W + w;
                sx = sx + w * qx;
                sy = sy + w * qy;
                sz = sz + w * qz;
            }
        }
        if (ok) {
            if (kind == 0) {
                const double c = (double)(1 + (r1 - r0));
                ox = sx / c;
                oy = sy / c;
                oz = sz / c;
            } else {
                ox = px + f * (sx / W - px);
                oy = py + f * (sy / W - py);
                oz = pz + f * (sz / W - pz);
            }
        }
    }
    dst[3 * (size_t)i] = ox;
    dst[3 * (size_t)i + 1] = oy;
    dst[3 * (size_t)i + 2] = oz;
    if (!ok) atomicOr((unsigned long long*)info, (unsigned long long)MF_ST_BAD_INDEX);
}

// ------------------------------------------------------------------------------------------------ host
// One workspace for the three sorting entries: the voxel parameters, the head, the bound partials, the sort over n = max(V, 6 F) pairs
// (its sums also scan n flags), and n words.
struct FiltersLayout {
    size_t params, head, part, words, total;
    SortLayout sort;
};
FiltersLayout filters_layout(int64_t n_verts, int64_t n_tris) {
    FiltersLayout l;
    const int64_t n = n_verts > 6 * n_tris ? n_verts : 6 * n_tris;
    l.params = 0;
    l.head = align256(sizeof(CloudParams));
    l.part = align256(l.head + sizeof(MeshSortHead));
    l.sort = sort_layout(l.part + 6 * sizeof(double) * CL_BOUND_BLOCKS, n, (uint64_t)n);
    l.words = l.sort.end;
    l.total = align256(l.words + 4 * (size_t)n);
    return l;
}

const int64_t MF_MAX_TRIANGLES = CL_MAX_POINTS / 6;     // six pairs per triangle (adjacency)

}  // namespace

extern "C" size_t lnr_mesh_filters_workspace(int64_t n_vertices, int64_t n_triangles) {
    if (!count_ok(n_vertices) || n_triangles < 0 || n_triangles > MF_MAX_TRIANGLES) return 0;
    return filters_layout(n_vertices, n_triangles).total;
}

extern "C" int lnr_mesh_vertex_clusters(const double* vertices, int64_t n_vertices, double voxel_size, void* workspace,
                                        size_t workspace_bytes, int32_t* vertex_cluster, double* cluster_vertices, int64_t* info_dev,
                                        void* stream) {
    CL_REQUIRE_COUNT("lnr_mesh_vertex_clusters", n_vertices, "vertices");
    LNR_REQUIRE(isfinite(voxel_size) && voxel_size > 0.0, "lnr_mesh_vertex_clusters: voxel_size must be finite and > 0, got %g", voxel_size);
    LNR_REQUIRE(info_dev && workspace && (n_vertices == 0 || (vertices && vertex_cluster && cluster_vertices)),
                "lnr_mesh_vertex_clusters: null argument");
    const FiltersLayout l = filters_layout(n_vertices, 0);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_mesh_vertex_clusters: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("mesh_vertex_clusters", st);
    char* ws = (char*)workspace;
    CloudParams* p = (CloudParams*)(ws + l.params);
    const uint32_t V = (uint32_t)n_vertices;
    if (int rc = clear_words(p, sizeof(CloudParams), st, "lnr_mesh_vertex_clusters", "parameters")) return rc;
    if (V == 0) {
        hipLaunchKernelGGL(cloud_params, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)(ws + l.part), 0, (const int32_t*)nullptr, 0u,
                           (int)CL_MODE_VOXEL, voxel_size, p);
    } else {
        const RadixBuffers r = radix_buffers(ws, l.sort);
        uint32_t* first = (uint32_t*)(ws + l.words);
        const int nbr = (int)(blocks_for(V) < CL_BOUND_BLOCKS ? blocks_for(V) : CL_BOUND_BLOCKS);
        if (int rc = clear_words(first, 4 * (size_t)V, st, "lnr_mesh_vertex_clusters", "first-occurrence flags")) return rc;
        hipLaunchKernelGGL(bound_partial, dim3(nbr), dim3(CL_BLOCK), 0, st, vertices, (const int32_t*)nullptr, V, (double*)(ws + l.part), p);
        hipLaunchKernelGGL(cloud_params, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)(ws + l.part), nbr, (const int32_t*)nullptr, V,
                           (int)CL_MODE_VOXEL, voxel_size, p);
        hipLaunchKernelGGL(cloud_keys, dim3(blocks_for(V)), dim3(CL_BLOCK), 0, st, vertices, (const CloudParams*)p, r.ka, r.ia);
        LNR_CHECK_LAUNCH("lnr_mesh_vertex_clusters");
        enqueue_radix_sort(r, &p->n, &p->npasses, st);
        hipLaunchKernelGGL(vc_first, dim3(blocks_for(V)), dim3(CL_BLOCK), 0, st, sorted_pairs(r), (const CloudParams*)p, first);
        enqueue_scan(first, V, r.sums, &p->n_seg, nullptr, 0, st);
        hipLaunchKernelGGL(vc_walk, dim3(blocks_for(V)), dim3(CL_BLOCK), 0, st, vertices, sorted_pairs(r), (const CloudParams*)p,
                           (const uint32_t*)first, vertex_cluster, cluster_vertices);
    }
    hipLaunchKernelGGL(vc_info, dim3(1), dim3(1), 0, st, (const CloudParams*)p, info_dev);
    LNR_CHECK_LAUNCH("lnr_mesh_vertex_clusters");
    return LNR_OK;
}

extern "C" int lnr_mesh_unique_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* vertex_map,
                                         int64_t n_mapped, int32_t drop_degenerate, void* workspace, size_t workspace_bytes,
                                         int32_t* canonical, uint8_t* triangle_keep, int64_t* info_dev, void* stream) {
    MESH_REQUIRE_COUNTS("lnr_mesh_unique_triangles", n_vertices, n_triangles, MF_MAX_TRIANGLES);
    LNR_REQUIRE(n_mapped >= 0 && n_mapped <= INT32_MAX && (vertex_map || n_mapped == n_vertices),
                "lnr_mesh_unique_triangles: n_mapped = %lld (0 .. 2^31 - 1; n_vertices = %lld without a map)", (long long)n_mapped,
                (long long)n_vertices);
    LNR_REQUIRE(info_dev && workspace && (n_triangles == 0 || (triangles && canonical && triangle_keep)),
                "lnr_mesh_unique_triangles: null argument");
    const FiltersLayout l = filters_layout(0, n_triangles);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_mesh_unique_triangles: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("mesh_unique_triangles", st);
    char* ws = (char*)workspace;
    MeshSortHead* h = (MeshSortHead*)(ws + l.head);
    const uint32_t F = (uint32_t)n_triangles;
    const int shift = (int)bit_length(n_mapped - 1);
    hipLaunchKernelGGL(mesh_head_init, dim3(1), dim3(1), 0, st, h, F, (int32_t)((shift + 7) / 8), (int32_t)((2 * shift + 7) / 8));
    if (F) {
        const RadixBuffers r = radix_buffers(ws, l.sort, F);            // F pairs in buffers laid out for 6 F
        hipLaunchKernelGGL(ut_keys, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, triangles, F, n_vertices, vertex_map, n_mapped, canonical,
                           r.ka, r.ia, h);
        LNR_CHECK_LAUNCH("lnr_mesh_unique_triangles");
        enqueue_radix_sort(r, &h->n, &h->npasses, st);
        hipLaunchKernelGGL(ut_rekey, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, (const int32_t*)canonical, r.ka, r.ia, (const uint32_t*)r.ib,
                           (const MeshSortHead*)h, (uint32_t)shift);
        enqueue_radix_sort(r, &h->n, &h->npasses2, st);
        hipLaunchKernelGGL(ut_mark, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, (const int32_t*)canonical, sorted_pairs(r), h,
                           (int)drop_degenerate, triangle_keep);
    }
    hipLaunchKernelGGL(mesh_head_info, dim3(1), dim3(1), 0, st, (const MeshSortHead*)h, info_dev, (int64_t)0);
    LNR_CHECK_LAUNCH("lnr_mesh_unique_triangles");
    return LNR_OK;
}

extern "C" int lnr_mesh_vertex_adjacency(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* workspace,
                                         size_t workspace_bytes, int32_t* row_start, int32_t* neighbours, int64_t* info_dev, void* stream) {
    MESH_REQUIRE_COUNTS("lnr_mesh_vertex_adjacency", n_vertices, n_triangles, MF_MAX_TRIANGLES);
    LNR_REQUIRE(info_dev && workspace && row_start && (n_triangles == 0 || (triangles && neighbours)),
                "lnr_mesh_vertex_adjacency: null argument");
    const FiltersLayout l = filters_layout(0, n_triangles);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_mesh_vertex_adjacency: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("mesh_vertex_adjacency", st);
    char* ws = (char*)workspace;
    MeshSortHead* h = (MeshSortHead*)(ws + l.head);
    const uint32_t F = (uint32_t)n_triangles, n = 6 * F;
    const uint64_t V = (uint64_t)n_vertices;
    const int shift = (int)bit_length(n_vertices - 1);
    const RadixBuffers r = radix_buffers(ws, l.sort);
    uint32_t* rank = (uint32_t*)(ws + l.words);
    hipLaunchKernelGGL(mesh_head_init, dim3(1), dim3(1), 0, st, h, n, (int32_t)(((int)bit_length(n_vertices) + shift + 7) / 8), 0);
    if (F) {
        hipLaunchKernelGGL(va_keys, dim3(blocks_for(F)), dim3(CL_BLOCK), 0, st, triangles, F, n_vertices, (uint32_t)shift, r.ka, r.ia, h);
        LNR_CHECK_LAUNCH("lnr_mesh_vertex_adjacency");
        enqueue_radix_sort(r, &h->n, &h->npasses, st);
        hipLaunchKernelGGL(va_heads, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, (const uint64_t*)r.ka, (const uint64_t*)r.kb,
                           (const MeshSortHead*)h, V, (uint32_t)shift, rank);
        enqueue_scan(rank, n, r.sums, &h->n_a, nullptr, 0, st);
        hipLaunchKernelGGL(va_emit, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, (const uint64_t*)r.ka, (const uint64_t*)r.kb,
                           (const MeshSortHead*)h, V, (uint32_t)shift, (const uint32_t*)rank, neighbours);
    }
    hipLaunchKernelGGL(va_rows, dim3(blocks_for(V + 1)), dim3(CL_BLOCK), 0, st, sorted_pairs(r), (const MeshSortHead*)h, V, (uint32_t)shift,
                       (const uint32_t*)rank, row_start);
    hipLaunchKernelGGL(mesh_head_info, dim3(1), dim3(1), 0, st, (const MeshSortHead*)h, info_dev, (int64_t)0);
    LNR_CHECK_LAUNCH("lnr_mesh_vertex_adjacency");
    return LNR_OK;
}

extern "C" int lnr_mesh_smooth(double* vertices, double* scratch, int64_t n_vertices, const int32_t* row_start, const int32_t* neighbours,
                               int64_t n_neighbours, int32_t kind, int32_t n_steps, double lambda, double mu, int64_t* info_dev,
                               void* stream) {
    LNR_REQUIRE(n_vertices >= 0 && n_vertices <= INT32_MAX && n_neighbours >= 0 && n_neighbours <= INT32_MAX,
                "lnr_mesh_smooth: %lld vertices, %lld neighbours, the limit is %d each", (long long)n_vertices, (long long)n_neighbours,
                INT32_MAX);
    LNR_REQUIRE((kind == 0 || kind == 1) && n_steps >= 0, "lnr_mesh_smooth: kind %d (0 simple, 1 Laplacian), %d steps", (int)kind,
                (int)n_steps);
    LNR_REQUIRE(isfinite(lambda) && isfinite(mu), "lnr_mesh_smooth: the factors must be finite, got %g and %g", lambda, mu);
    LNR_REQUIRE(info_dev && (n_vertices == 0 || (vertices && scratch && row_start)) && (n_neighbours == 0 || neighbours),
                "lnr_mesh_smooth: null argument");
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("mesh_smooth", st);
    const uint32_t V = (uint32_t)n_vertices;
    hipLaunchKernelGGL(sm_info, dim3(1), dim3(1), 0, st, info_dev);
    if (V && n_steps > 0) {
        // step s writes the caller's array when an even number of steps follow it; an odd count starts from a copy in scratch
        if ((n_steps & 1) && hipMemcpyAsync(scratch, vertices, 24 * (size_t)V, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            lnr_set_error("lnr_mesh_smooth: copying the vertices failed");
            return LNR_ERR_LAUNCH;
        }
        for (int s = 0; s < n_steps; ++s) {
            const bool to_caller = ((n_steps - 1 - s) & 1) == 0;
            hipLaunchKernelGGL(sm_step, dim3(blocks_for(V)), dim3(CL_BLOCK), 0, st, (const double*)(to_caller ? scratch : vertices),
                               to_caller ? vertices : scratch, V, row_start, neighbours, n_neighbours, (int)kind, (s & 1) ? mu : lambda,
                               info_dev);
        }
    }
    LNR_CHECK_LAUNCH("lnr_mesh_smooth");
    return LNR_OK;
}
