// Taking a point cloud apart (gfx950): radius counts, DBSCAN clusters and the RANSAC plane.
//
// Replaces open3d's PointCloud::RemoveRadiusOutliers, ClusterDBSCAN and SegmentPlane with the definitions stated in
// include/loner_hip.h ("segmentation").  This file is compiled with -ffp-contract=off (build.py EXACT): every fp64 expression below
// rounds operation by operation, as the numpy restatement (tests/segment_restatement.py) does.  No kernel hands anything between
// workgroups inside a launch and none waits for another: reductions are separate launches or one workgroup's fold, integer atomics
// (the union-find's hooks, counters) are the only atomics, and every loop is bounded by the call's arguments (a union-find walk by
// n: parents only ever fall).  Two runs give the same bytes.
//   neighbours one thread per point in *sorted* order (the grid's key order), in every pass that walks neighbours: the 64 lanes of a
//              wave then sit in the same or in adjacent cells, so their binary searches take the same branches and their reads of the
//              neighbouring rows hit the same cache lines (the points of a z-row are contiguous in the grid buffer).  A thread per
//              point in input order would scatter each wave over the whole cloud.  Results are written at the input index
//              (g.orig), which is the one scattered 4-byte store per point.  The walk is lnr_icp_correspondences' (ceil(r / edge)
//              + 1 shells at most, ended by the shells' lower bound), without a best-so-far: every target with d2 < r2 is visited
//   DBSCAN     count (cores; parent[i] = i), union (a core hooks itself to every core neighbour of lower input index:
//              lnr_union_find.h, so a root is its cluster's smallest core), roots (one find per core; flag[root] = 1), the exclusive
//              scan of the flags in input order (block counts, one workgroup's scan of them, ranks), labels, and the border pass
//              (a non-core takes the smallest label among its core neighbours).  The union-find runs on input indices, the walks on
//              sorted slots; the per-slot arrays (core, root / label) are what a neighbour's visit reads, contiguous like the points
//   plane      plane_check (every hypothesis: draw, repeated index, degenerate normal; one status byte each), plane_score (one
//              hypothesis per lane with its plane in 4 registers, a (chunk, tile of 256 hypotheses) grid, the chunk's points staged
//              through LDS and read as broadcasts), plane_fold (one thread per hypothesis adds its chunk partials in chunk order),
//              plane_select (one workgroup, the total order), plane_mask (one thread per point), and for the refit
//              plane_cumulants (lnr_cloud_outlier_threshold's order of summation) and plane_refit (one workgroup's fold, the
//              covariance and FastEigen3x3 of lnr_eigen3.h).  Rejected hypotheses are not compacted away as
//              lnr_ransac_correspondence's are: three distinct points are almost never collinear, so nearly every lane survives
#include "lnr_eigen3.h"
#include "lnr_union_find.h"

#define SG_NONE 0xFFFFFFFFu
#define PL_STAGE 512                    // points staged in LDS at a time by plane_score (a divisor of LNR_RANSAC_CHUNK)
#define PL_MAX_H ((int64_t)1 << 22)
#define PL_MAX_BLOCKS 2048              // blocks of plane_cumulants, at most
#define PL_TERMS 9

namespace {

enum { SG_ST_NONFINITE = 1, SG_ST_UNUSABLE = 2 };

__device__ inline bool grid_usable(const GridView& g, uint32_t n) { return g.p->status == 0 && g.p->n == n; }

// ------------------------------------------------------------------------------------------------ neighbours within a radius
__device__ inline int64_t radius_shells(const CloudParams* p, double r) {
    const double dmax = (double)(p->dims[0] > p->dims[1] ? (p->dims[0] > p->dims[2] ? p->dims[0] : p->dims[2])
                                                         : (p->dims[1] > p->dims[2] ? p->dims[1] : p->dims[2]));
    return (int64_t)fmin(ceil(r / p->edge) + 1.0, dmax);
}

// visit(k) for every sorted slot k with d2(p_j, p_k) < r2, slot j itself included; returns the shells walked
template <class F>
__device__ inline uint32_t radius_walk(const GridView& g, uint32_t j, double r2, int64_t max_shell, F& visit) {
    const double* q = g.pts + 3 * (size_t)j;
    const ShellQuery s = shell_query(g.p, q[0], q[1], q[2]);
    auto each = [&](uint32_t k) {
        if (sq_dist(s.q[0], s.q[1], s.q[2], g.pts + 3 * (size_t)k) < r2) visit(k);
    };
    uint32_t shells = 0;
    for (int64_t r = 0; r <= max_shell; ++r) {
        const double lb = shell_visit(g, s, r, each);
        ++shells;
        if (lb == INFINITY || r2 <= lb) break;
    }
    return shells;
}

// counts (input order, nullable): the neighbours of every point.  DBSCAN: core[slot] = count >= min_points and parent[i] = i as well.
// counters: [1] 1 when the grid is unusable (nothing else is written), [2] shells walked
template <bool DBSCAN>
__global__ __launch_bounds__(CL_BLOCK) void seg_count(GridView g, uint32_t n, double r, uint32_t min_points, uint32_t* __restrict__ counts,
                                                      unsigned char* __restrict__ core, uint32_t* __restrict__ parent,
                                                      unsigned long long* __restrict__ counters) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (!grid_usable(g, n)) {
        if (j == 0 && counters) counters[1] = 1ull;
        return;
    }
    unsigned long long shells = 0;
    if (j < n) {
        uint32_t c = 0;
        auto visit = [&](uint32_t) { ++c; };
        shells = radius_walk(g, j, r * r, radius_shells(g.p, r), visit);
        const uint32_t o = g.orig[j];
        if (o < n) {
            if (counts) counts[o] = c;
            if (DBSCAN) parent[o] = o;
        }
        if (DBSCAN) core[j] = c >= min_points ? 1 : 0;
    }
    if (counters) {
        shells = wave_sum(shells);
        if ((threadIdx.x & 63) == 0 && shells) atomicAdd(&counters[2], shells);
    }
}

// ------------------------------------------------------------------------------------------------ DBSCAN
// head (uint64 [8]): [0] clusters, [1] cores, [2] border points, [3] noise points
struct DbLayout { size_t core, parent, flag, rank, root, block_off, head, total; };
DbLayout db_layout(int64_t n) {
    DbLayout l;
    const size_t N = (size_t)n, nb = (N + CL_BLOCK - 1) / CL_BLOCK;
    l.core = 0;
    l.parent = align256(N);
    l.flag = align256(l.parent + 4 * N);
    l.rank = align256(l.flag + 4 * N);
    l.root = align256(l.rank + 4 * N);
    l.block_off = align256(l.root + 4 * N);
    l.head = align256(l.block_off + 4 * (nb + 1));
    l.total = align256(l.head + 64);
    return l;
}

// a core hooks itself to every core neighbour of lower input index (each adjacent pair once)
__global__ __launch_bounds__(CL_BLOCK) void db_union(GridView g, uint32_t n, double eps, const unsigned char* __restrict__ core,
                                                     uint32_t* __restrict__ parent) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (!grid_usable(g, n) || j >= n || !core[j]) return;
    const uint32_t me = g.orig[j];
    if (me >= n) return;
    auto visit = [&](uint32_t k) {
        if (!core[k]) return;
        const uint32_t o = g.orig[k];
        if (o < me) uf_unite(parent, me, o);
    };
    radius_walk(g, j, eps * eps, radius_shells(g.p, eps), visit);
}

// root[slot] of every core (SG_NONE otherwise) and flag[i] = 1 at the roots; no hook runs beside this kernel, so a root found is final
__global__ __launch_bounds__(CL_BLOCK) void db_roots(GridView g, uint32_t n, const unsigned char* __restrict__ core,
                                                     uint32_t* __restrict__ parent, uint32_t* __restrict__ root, uint32_t* __restrict__ flag) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (!grid_usable(g, n) || j >= n) return;
    const uint32_t me = g.orig[j];
    uint32_t r = SG_NONE;
    if (core[j] && me < n) {
        r = uf_find(parent, me);
        if (r == me) flag[me] = 1u;
    }
    root[j] = r;
}

__global__ __launch_bounds__(CL_BLOCK) void seg_block_count(const uint32_t* __restrict__ flag, uint32_t n, uint32_t* __restrict__ block_count) {
    __shared__ uint32_t lds[4];
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    uint32_t total;
    block_exclusive_scan(i < n ? flag[i] : 0u, lds, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// one workgroup: block_count [nb] -> its exclusive prefix in place, the total in head[0]
__global__ __launch_bounds__(CL_BLOCK) void seg_offsets(uint32_t* __restrict__ block_count, uint32_t nb, unsigned long long* __restrict__ head) {
    __shared__ uint32_t lds[4];
    const uint32_t per = (nb + CL_BLOCK - 1) / CL_BLOCK;
    const uint64_t b0 = (uint64_t)threadIdx.x * per;
    uint32_t mine = 0;
    for (uint32_t k = 0; k < per; ++k) mine += b0 + k < nb ? block_count[b0 + k] : 0u;
    uint32_t total;
    uint32_t run = block_exclusive_scan(mine, lds, &total);
    for (uint32_t k = 0; k < per; ++k) {
        if (b0 + k < nb) {
            const uint32_t c = block_count[b0 + k];
            block_count[b0 + k] = run;
            run += c;
        }
    }
    if (threadIdx.x == 0) head[0] = total;
}

// rank[i] = the flags before i
__global__ __launch_bounds__(CL_BLOCK) void seg_rank(const uint32_t* __restrict__ flag, uint32_t n, const uint32_t* __restrict__ block_off,
                                                     uint32_t* __restrict__ rank) {
    __shared__ uint32_t lds[4];
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    uint32_t total;
    const uint32_t before = block_exclusive_scan(i < n ? flag[i] : 0u, lds, &total);
    if (i < n) rank[i] = block_off[blockIdx.x] + before;
}

// a core's label = the rank of its root; root[slot] becomes the slot's label (SG_NONE stays for a non-core)
__global__ __launch_bounds__(CL_BLOCK) void db_labels(GridView g, uint32_t n, const uint32_t* __restrict__ rank, uint32_t* __restrict__ root,
                                                      int32_t* __restrict__ labels) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (!grid_usable(g, n) || j >= n) return;
    const uint32_t r = root[j];
    if (r == SG_NONE || r >= n) return;
    const uint32_t lab = rank[r];
    root[j] = lab;
    const uint32_t me = g.orig[j];
    if (me < n) labels[me] = (int32_t)lab;
}

// a non-core takes the smallest label among its core neighbours, or stays -1; the tallies
__global__ __launch_bounds__(CL_BLOCK) void db_border(GridView g, uint32_t n, double eps, const unsigned char* __restrict__ core,
                                                      const uint32_t* __restrict__ label_of, int32_t* __restrict__ labels,
                                                      unsigned long long* __restrict__ head) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (!grid_usable(g, n)) return;
    int cls = -1;                                              // 0 core, 1 border, 2 noise
    if (j < n) {
        cls = 0;
        if (!core[j]) {
            uint32_t best = SG_NONE;
            auto visit = [&](uint32_t k) {
                if (core[k]) best = label_of[k] < best ? label_of[k] : best;
            };
            radius_walk(g, j, eps * eps, radius_shells(g.p, eps), visit);
            cls = best == SG_NONE ? 2 : 1;
            const uint32_t me = g.orig[j];
            if (cls == 1 && me < n) labels[me] = (int32_t)best;
        }
    }
    wave_count_add(cls == 0, &head[1]);
    wave_count_add(cls == 1, &head[2]);
    wave_count_add(cls == 2, &head[3]);
}

__global__ void db_info(GridView g, uint32_t n, const unsigned long long* __restrict__ head, int64_t* __restrict__ info) {
    for (int k = 0; k < 8; ++k) info[k] = 0;
    if (n == 0) return;
    if (!grid_usable(g, n)) {
        info[0] = SG_ST_UNUSABLE | ((g.p->status & CL_ST_NONFINITE) ? SG_ST_NONFINITE : 0);
        return;
    }
    for (int k = 0; k < 4; ++k) info[1 + k] = (int64_t)head[k];
}

// ------------------------------------------------------------------------------------------------ the RANSAC plane
enum { PL_OK = 0, PL_REPEATED = 1, PL_DEGENERATE = 2 };
enum { PL_ST_FEW = 1, PL_ST_NONE = 2 };

// head (uint64 [8]): [1] rejected: repeated, [2] rejected: degenerate, [4] non-finite points
struct PlaneLayout { size_t status, head, part, part_cnt, part_sum, total; };
uint32_t plane_chunks(int64_t n) { return (uint32_t)((n + LNR_RANSAC_CHUNK - 1) / LNR_RANSAC_CHUNK); }
uint32_t plane_blocks(int64_t n) {
    const uint32_t b = blocks_for(n);
    return b < 1 ? 1u : (b < PL_MAX_BLOCKS ? b : (uint32_t)PL_MAX_BLOCKS);
}
PlaneLayout plane_layout(int64_t n, int64_t H) {
    PlaneLayout l;
    const size_t h = (size_t)H, nc = plane_chunks(n) ? plane_chunks(n) : 1;
    l.status = 0;
    l.head = align256(h);
    l.part = align256(l.head + 64);                              // the refit's block partials [PL_MAX_BLOCKS, 16]
    l.part_cnt = align256(l.part + 8 * 16 * (size_t)PL_MAX_BLOCKS);
    l.part_sum = align256(l.part_cnt + 4 * h * nc);
    l.total = align256(l.part_sum + 8 * h * nc);
    return l;
}

// hypothesis h: PL_OK and its plane pl = (nv, d), or why it is rejected; *first gets the index of its first sample.  n >= 3
__device__ inline int plane_hypothesis(const double* __restrict__ pts, uint32_t n, uint32_t h, uint64_t seed, double pl[4], uint32_t* first) {
    const Philox4 r = philox4x32_10((uint64_t)h, LNR_STREAM_PLANE, seed);
    const uint32_t i0 = (uint32_t)(((uint64_t)r.x * n) >> 32), i1 = (uint32_t)(((uint64_t)r.y * n) >> 32),
                   i2 = (uint32_t)(((uint64_t)r.z * n) >> 32);
    *first = i0;
    if (i0 == i1 || i0 == i2 || i1 == i2) return PL_REPEATED;
    const double *a = pts + 3 * (size_t)i0, *b = pts + 3 * (size_t)i1, *c = pts + 3 * (size_t)i2;
    const double a3[3] = {a[0], a[1], a[2]};
    const double ab[3] = {b[0] - a3[0], b[1] - a3[1], b[2] - a3[2]}, ac[3] = {c[0] - a3[0], c[1] - a3[1], c[2] - a3[2]};
    double nrm[3];
    cross3(ab, ac, nrm);
    const double L = sqrt(dot3(nrm, nrm));
    pl[0] = nrm[0] / L; pl[1] = nrm[1] / L; pl[2] = nrm[2] / L;
    pl[3] = -dot3(pl, a3);
    if (L == 0.0 || !isfinite(L) || !finite3(pl[0], pl[1], pl[2]) || !isfinite(pl[3])) return PL_DEGENERATE;
    return PL_OK;
}

__device__ inline double plane_residual(const double pl[4], double x, double y, double z) {
    return ((pl[0] * x + pl[1] * y) + pl[2] * z) + pl[3];
}

__global__ __launch_bounds__(CL_BLOCK) void plane_nonfinite(const double* __restrict__ pts, uint32_t n, unsigned long long* __restrict__ head) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool bad = i < n && !finite3(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
    wave_count_add(bad, &head[4]);
}

__global__ __launch_bounds__(CL_BLOCK) void plane_check(const double* __restrict__ pts, uint32_t n, uint32_t H, uint64_t seed,
                                                        unsigned char* __restrict__ status, unsigned long long* __restrict__ head) {
    const uint32_t h = blockIdx.x * CL_BLOCK + threadIdx.x;
    int st = -1;
    if (h < H) {
        double pl[4];
        uint32_t first;
        st = plane_hypothesis(pts, n, h, seed, pl, &first);
        status[h] = (unsigned char)st;
    }
    wave_count_add(st == PL_REPEATED, &head[1]);
    wave_count_add(st == PL_DEGENERATE, &head[2]);
}

// blockIdx.x: the chunk of points, blockIdx.y: the tile of 256 hypotheses; one hypothesis per lane.  A rejected hypothesis scores
// against a NaN plane: no inlier
__global__ __launch_bounds__(CL_BLOCK) void plane_score(const double* __restrict__ pts, uint32_t n, uint32_t H, uint64_t seed, double t,
                                                        uint32_t* __restrict__ part_cnt, double* __restrict__ part_sum) {
    __shared__ double stage[PL_STAGE * 3];
    const uint32_t h = blockIdx.y * CL_BLOCK + threadIdx.x;
    const bool active = h < H;
    double pl[4] = {0.0, 0.0, 0.0, (double)NAN};
    if (active) {
        uint32_t first;
        if (plane_hypothesis(pts, n, h, seed, pl, &first) != PL_OK) pl[3] = (double)NAN;
    }
    const uint32_t c0 = blockIdx.x * LNR_RANSAC_CHUNK;
    const uint32_t c1 = n - c0 < LNR_RANSAC_CHUNK ? n : c0 + LNR_RANSAC_CHUNK;
    uint32_t cnt = 0;
    double sum = 0.0;
    for (uint32_t b = c0; b < c1; b += PL_STAGE) {
        const uint32_t rows = c1 - b < PL_STAGE ? c1 - b : PL_STAGE;
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < 3 * rows; k += CL_BLOCK) stage[k] = pts[3 * (size_t)b + k];
        __syncthreads();
        for (uint32_t r = 0; r < rows; ++r) {
            const double e = plane_residual(pl, stage[3 * r], stage[3 * r + 1], stage[3 * r + 2]);
            if (fabs(e) < t) {
                ++cnt;
                sum = sum + e * e;
            }
        }
    }
    if (active) {
        part_cnt[(size_t)blockIdx.x * H + h] = cnt;
        part_sum[(size_t)blockIdx.x * H + h] = sum;
    }
}

// one thread per hypothesis: its chunk partials in chunk order, left in chunk 0's row
__global__ __launch_bounds__(CL_BLOCK) void plane_fold(uint32_t H, uint32_t n_chunks, uint32_t* __restrict__ part_cnt, double* __restrict__ part_sum) {
    const uint32_t h = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (h >= H) return;
    uint32_t c = 0;
    double sum = 0.0;
    for (uint32_t k = 0; k < n_chunks; ++k) {
        c += part_cnt[(size_t)k * H + h];
        sum = sum + part_sum[(size_t)k * H + h];
    }
    part_cnt[h] = c;
    part_sum[h] = sum;
}

__device__ inline bool plane_better(uint32_t c, double s, uint32_t h, uint32_t bc, double bs, uint32_t bh) {
    return c > bc || (c == bc && (s < bs || (s == bs && h < bh)));
}

// one workgroup: the best surviving hypothesis under (count desc, sum asc, h asc), both models and the info words.
// n < 3 (nothing else ran): PL_ST_FEW
__global__ __launch_bounds__(CL_BLOCK) void plane_select(const double* __restrict__ pts, uint32_t n, uint32_t H, uint64_t seed,
                                                         const unsigned char* __restrict__ status, const unsigned long long* __restrict__ head,
                                                         const uint32_t* __restrict__ tot_cnt, const double* __restrict__ tot_sum,
                                                         double* __restrict__ plane, int64_t* __restrict__ info) {
    __shared__ uint32_t s_cnt[CL_BLOCK], s_h[CL_BLOCK];
    __shared__ double s_sum[CL_BLOCK];
    const bool few = n < 3;
    uint32_t bc = 0, bh = SG_NONE;
    double bs = INFINITY;
    if (!few) {
        for (uint32_t h = threadIdx.x; h < H; h += CL_BLOCK) {
            if (status[h] != PL_OK) continue;
            const uint32_t c = tot_cnt[h];
            const double sum = tot_sum[h];
            if (bh == SG_NONE || plane_better(c, sum, h, bc, bs, bh)) { bc = c; bs = sum; bh = h; }
        }
    }
    s_cnt[threadIdx.x] = bc;
    s_sum[threadIdx.x] = bs;
    s_h[threadIdx.x] = bh;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int t = 1; t < CL_BLOCK; ++t)
        if (s_h[t] != SG_NONE && (bh == SG_NONE || plane_better(s_cnt[t], s_sum[t], s_h[t], bc, bs, bh))) { bc = s_cnt[t]; bs = s_sum[t]; bh = s_h[t]; }
    double pl[4] = {0.0, 0.0, 0.0, 0.0};
    const bool none = bh == SG_NONE;
    uint32_t first;
    if (!none) plane_hypothesis(pts, n, bh, seed, pl, &first);
    else bc = 0;
    for (int k = 0; k < 4; ++k) { plane[k] = pl[k]; plane[4 + k] = pl[k]; }
    const unsigned long long rejected = few ? 0ull : head[1] + head[2];
    info[0] = (few ? PL_ST_FEW : 0) | (!few && none ? PL_ST_NONE : 0);
    info[1] = none ? -1 : (int64_t)bh;
    info[2] = (int64_t)bc;
    info[3] = few ? 0 : (int64_t)H - (int64_t)rejected;
    info[4] = few ? 0 : (int64_t)head[1];
    info[5] = few ? 0 : (int64_t)head[2];
    info[6] = (int64_t)head[4];
    info[7] = (int64_t)n;
}

// the best hypothesis's mask: the test plane_score counted with
__global__ __launch_bounds__(CL_BLOCK) void plane_mask(const double* __restrict__ pts, uint32_t n, double t, const double* __restrict__ plane,
                                                       const int64_t* __restrict__ info, unsigned char* __restrict__ inlier) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n || info[1] < 0) return;
    const double pl[4] = {plane[4], plane[5], plane[6], plane[7]};
    const double e = plane_residual(pl, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
    inlier[i] = fabs(e) < t ? 1 : 0;
}

// the cumulants of the inliers about the hypothesis's first sample point a, with q = p - a per axis: (qx, qy, qz, qx qx, qx qy, qx qz,
// qy qy, qy qz, qz qz).  Thread by thread in index order (i = thread, thread + stride, ...), then the block's fixed-order sum
__global__ __launch_bounds__(CL_BLOCK) void plane_cumulants(const double* __restrict__ pts, uint32_t n, uint64_t seed,
                                                            const unsigned char* __restrict__ inlier, const int64_t* __restrict__ info,
                                                            double* __restrict__ part) {
    __shared__ double lds[CL_BLOCK / 64];
    if (info[1] < 0) return;
    const Philox4 r = philox4x32_10((uint64_t)info[1], LNR_STREAM_PLANE, seed);
    const uint32_t i0 = (uint32_t)(((uint64_t)r.x * n) >> 32);
    const double a[3] = {pts[3 * (size_t)i0], pts[3 * (size_t)i0 + 1], pts[3 * (size_t)i0 + 2]};
    double acc[PL_TERMS];
#pragma unroll
    for (int v = 0; v < PL_TERMS; ++v) acc[v] = 0.0;
    for (uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x; i < n; i += gridDim.x * CL_BLOCK) {
        if (!inlier[i]) continue;
        const double x = pts[3 * (size_t)i] - a[0], y = pts[3 * (size_t)i + 1] - a[1], z = pts[3 * (size_t)i + 2] - a[2];
        acc[0] = acc[0] + x; acc[1] = acc[1] + y; acc[2] = acc[2] + z;
        acc[3] = acc[3] + x * x; acc[4] = acc[4] + x * y; acc[5] = acc[5] + x * z;
        acc[6] = acc[6] + y * y; acc[7] = acc[7] + y * z; acc[8] = acc[8] + z * z;
    }
#pragma unroll
    for (int v = 0; v < PL_TERMS; ++v) {
        const double t = block_sum(acc[v], lds);
        if (threadIdx.x == 0) part[16 * (size_t)blockIdx.x + v] = t;
    }
}

// one workgroup: the partials as lnr_cloud_outlier_threshold folds them (thread t: blocks t, t + 256, ... in turn, then the block
// sum), the covariance as lnr_cloud_normals forms it, its normal turned towards the hypothesis's, d from the centroid
__global__ __launch_bounds__(CL_BLOCK) void plane_refit(const double* __restrict__ pts, uint32_t n, uint64_t seed, const double* __restrict__ part,
                                                        uint32_t n_part, const int64_t* __restrict__ info, double* __restrict__ plane) {
    __shared__ double lds[CL_BLOCK / 64];
    if (info[1] < 0 || info[2] < 3) return;
    double s[PL_TERMS];
    for (int v = 0; v < PL_TERMS; ++v) {
        double acc = 0.0;
        for (uint32_t b = threadIdx.x; b < n_part; b += CL_BLOCK) acc = acc + part[16 * (size_t)b + v];
        s[v] = block_sum(acc, lds);
    }
    if (threadIdx.x != 0) return;
    const Philox4 r = philox4x32_10((uint64_t)info[1], LNR_STREAM_PLANE, seed);
    const uint32_t i0 = (uint32_t)(((uint64_t)r.x * n) >> 32);
    const double c = (double)info[2];
    for (int v = 0; v < PL_TERMS; ++v) s[v] = s[v] / c;
    double C[3][3];
    C[0][0] = s[3] - s[0] * s[0]; C[1][1] = s[6] - s[1] * s[1]; C[2][2] = s[8] - s[2] * s[2];
    C[0][1] = C[1][0] = s[4] - s[0] * s[1];
    C[0][2] = C[2][0] = s[5] - s[0] * s[2];
    C[1][2] = C[2][1] = s[7] - s[1] * s[2];
    double nv[3];
    normal_of(C, nv);
    const double old[3] = {plane[4], plane[5], plane[6]};
    if (dot3(nv, old) < 0.0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
    const double centre[3] = {pts[3 * (size_t)i0] + s[0], pts[3 * (size_t)i0 + 1] + s[1], pts[3 * (size_t)i0 + 2] + s[2]};
    plane[0] = nv[0]; plane[1] = nv[1]; plane[2] = nv[2];
    plane[3] = -dot3(nv, centre);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host
extern "C" int lnr_cloud_radius_count(const void* grid, int64_t n_points, double radius, uint32_t* counts, int64_t* counters_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_radius_count", n_points, "points");
    LNR_REQUIRE(isfinite(radius) && radius > 0.0, "lnr_cloud_radius_count: radius must be finite and > 0, got %g", radius);
    LNR_REQUIRE(grid && counters_dev && (n_points == 0 || counts), "lnr_cloud_radius_count: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = clear_words(counters_dev, 4 * sizeof(int64_t), st, "lnr_cloud_radius_count", "counters")) return rc;
    if (n_points == 0) return LNR_OK;
    LnrProfScope prof("cloud_radius_count", st);
    const uint32_t n = (uint32_t)n_points;
    hipLaunchKernelGGL(seg_count<false>, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, grid_view(grid, n_points), n, radius, 0u, counts,
                       (unsigned char*)nullptr, (uint32_t*)nullptr, (unsigned long long*)counters_dev);
    LNR_CHECK_LAUNCH("lnr_cloud_radius_count");
    return LNR_OK;
}

extern "C" size_t lnr_cloud_dbscan_workspace(int64_t n_points) {
    if (!count_ok(n_points)) return 0;
    return db_layout(n_points).total;
}

extern "C" int lnr_cloud_dbscan(const void* grid, int64_t n_points, double eps, int32_t min_points, int32_t* labels, void* workspace,
                                size_t workspace_bytes, int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_dbscan", n_points, "points");
    LNR_REQUIRE(isfinite(eps) && eps > 0.0, "lnr_cloud_dbscan: eps must be finite and > 0, got %g", eps);
    LNR_REQUIRE(min_points >= 1, "lnr_cloud_dbscan: min_points must be >= 1, got %d", (int)min_points);
    LNR_REQUIRE(grid && workspace && info_dev && (n_points == 0 || labels), "lnr_cloud_dbscan: null argument");
    const DbLayout l = db_layout(n_points);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_cloud_dbscan: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("cloud_dbscan", st);
    char* ws = (char*)workspace;
    unsigned char* core = (unsigned char*)(ws + l.core);
    uint32_t* parent = (uint32_t*)(ws + l.parent);
    uint32_t* flag = (uint32_t*)(ws + l.flag);
    uint32_t* rank = (uint32_t*)(ws + l.rank);
    uint32_t* root = (uint32_t*)(ws + l.root);
    uint32_t* block_off = (uint32_t*)(ws + l.block_off);
    unsigned long long* head = (unsigned long long*)(ws + l.head);
    const uint32_t n = (uint32_t)n_points, nb = blocks_for(n);
    const GridView g = grid_view(grid, n_points);
    if (n) {
        // the core bytes, the parents and the flags start at 0, and every label at -1: a grid built for another cloud leaves nothing
        // unwritten that a later kernel or the caller reads
        if (int rc = clear_words(ws + l.core, l.rank - l.core, st, "lnr_cloud_dbscan", "workspace")) return rc;
        if (int rc = clear_words(head, 64, st, "lnr_cloud_dbscan", "counters")) return rc;
        if (hipMemsetAsync(labels, 0xFF, 4 * (size_t)n, st) != hipSuccess) {
            lnr_set_error("lnr_cloud_dbscan: clearing the labels failed");
            return LNR_ERR_LAUNCH;
        }
        const dim3 grd(nb), blk(CL_BLOCK);
        hipLaunchKernelGGL(seg_count<true>, grd, blk, 0, st, g, n, eps, (uint32_t)min_points, (uint32_t*)nullptr, core, parent,
                           (unsigned long long*)nullptr);
        hipLaunchKernelGGL(db_union, grd, blk, 0, st, g, n, eps, (const unsigned char*)core, parent);
        hipLaunchKernelGGL(db_roots, grd, blk, 0, st, g, n, (const unsigned char*)core, parent, root, flag);
        hipLaunchKernelGGL(seg_block_count, grd, blk, 0, st, (const uint32_t*)flag, n, block_off);
        hipLaunchKernelGGL(seg_offsets, dim3(1), blk, 0, st, block_off, nb, head);
        hipLaunchKernelGGL(seg_rank, grd, blk, 0, st, (const uint32_t*)flag, n, (const uint32_t*)block_off, rank);
        hipLaunchKernelGGL(db_labels, grd, blk, 0, st, g, n, (const uint32_t*)rank, root, labels);
        hipLaunchKernelGGL(db_border, grd, blk, 0, st, g, n, eps, (const unsigned char*)core, (const uint32_t*)root, labels, head);
    }
    hipLaunchKernelGGL(db_info, dim3(1), dim3(1), 0, st, g, n, (const unsigned long long*)head, info_dev);
    LNR_CHECK_LAUNCH("lnr_cloud_dbscan");
    return LNR_OK;
}

extern "C" size_t lnr_plane_workspace(int64_t n_points, int64_t n_hypotheses) {
    if (!count_ok(n_points) || n_hypotheses < 1 || n_hypotheses > PL_MAX_H) return 0;
    return plane_layout(n_points, n_hypotheses).total;
}

extern "C" int lnr_cloud_segment_plane(const double* points, int64_t n_points, double distance_threshold, int64_t n_hypotheses,
                                       uint64_t seed, int32_t refine, double* plane_dev, uint8_t* inlier, void* workspace,
                                       size_t workspace_bytes, int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_segment_plane", n_points, "points");
    LNR_REQUIRE(n_hypotheses >= 1 && n_hypotheses <= PL_MAX_H, "lnr_cloud_segment_plane: n_hypotheses must be in [1, %lld], got %lld",
                (long long)PL_MAX_H, (long long)n_hypotheses);
    LNR_REQUIRE(isfinite(distance_threshold) && distance_threshold > 0.0,
                "lnr_cloud_segment_plane: distance_threshold must be finite and > 0, got %g", distance_threshold);
    LNR_REQUIRE(workspace && plane_dev && info_dev && (n_points == 0 || (points && inlier)), "lnr_cloud_segment_plane: null argument");
    const PlaneLayout l = plane_layout(n_points, n_hypotheses);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_cloud_segment_plane: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("cloud_segment_plane", st);
    char* ws = (char*)workspace;
    unsigned char* status = (unsigned char*)(ws + l.status);
    unsigned long long* head = (unsigned long long*)(ws + l.head);
    double* part = (double*)(ws + l.part);
    uint32_t* part_cnt = (uint32_t*)(ws + l.part_cnt);
    double* part_sum = (double*)(ws + l.part_sum);
    const uint32_t n = (uint32_t)n_points, H = (uint32_t)n_hypotheses, hb = blocks_for(H), nc = plane_chunks(n_points);
    if (int rc = clear_words(head, 64, st, "lnr_cloud_segment_plane", "counters")) return rc;
    if (n)
        if (int rc = clear_words(inlier, n, st, "lnr_cloud_segment_plane", "mask")) return rc;
    if (n) hipLaunchKernelGGL(plane_nonfinite, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, points, n, head);
    if (n >= 3) {
        hipLaunchKernelGGL(plane_check, dim3(hb), dim3(CL_BLOCK), 0, st, points, n, H, seed, status, head);
        hipLaunchKernelGGL(plane_score, dim3(nc, hb), dim3(CL_BLOCK), 0, st, points, n, H, seed, distance_threshold, part_cnt, part_sum);
        hipLaunchKernelGGL(plane_fold, dim3(hb), dim3(CL_BLOCK), 0, st, H, nc, part_cnt, part_sum);
    }
    hipLaunchKernelGGL(plane_select, dim3(1), dim3(CL_BLOCK), 0, st, points, n, H, seed, (const unsigned char*)status,
                       (const unsigned long long*)head, (const uint32_t*)part_cnt, (const double*)part_sum, plane_dev, info_dev);
    if (n >= 3) {
        hipLaunchKernelGGL(plane_mask, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, points, n, distance_threshold, (const double*)plane_dev,
                           (const int64_t*)info_dev, inlier);
        if (refine) {
            const uint32_t pb = plane_blocks(n_points);
            hipLaunchKernelGGL(plane_cumulants, dim3(pb), dim3(CL_BLOCK), 0, st, points, n, seed, (const unsigned char*)inlier,
                               (const int64_t*)info_dev, part);
            hipLaunchKernelGGL(plane_refit, dim3(1), dim3(CL_BLOCK), 0, st, points, n, seed, (const double*)part, pb, (const int64_t*)info_dev,
                               plane_dev);
        }
    }
    LNR_CHECK_LAUNCH("lnr_cloud_segment_plane");
    return LNR_OK;
}
