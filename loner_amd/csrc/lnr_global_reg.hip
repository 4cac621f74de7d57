// Global registration of two point clouds without a starting pose (gfx950): normal orientation, FPFH features, the exact nearest
// neighbour in feature space and RANSAC on correspondences.
//
// Replaces open3d's orient_normals_towards_camera_location / orient_normals_to_align_with_direction, compute_fpfh_feature,
// the feature search of registration_ransac_based_on_feature_matching and registration_ransac_based_on_correspondence with the
// definitions stated in include/loner_hip.h ("global registration").  This file is compiled with -ffp-contract=off (build.py EXACT):
// every fp64 expression below rounds operation by operation, as the numpy restatement (tests/global_reg_restatement.py) does.  No
// kernel hands anything between workgroups inside a launch: reductions are separate launches or one workgroup's fold, integer counters
// are the only atomics, and every loop is bounded by the call's arguments.
//   orient     one thread per normal
//   FPFH       fpfh_inverse (sorted slot of every input index), then lnr_cloud_knn.h's search whose Finish (FpfhListFinish) writes the
//              radius-cut neighbour list (ids, d2, count) to the workspace; fpfh_spfh (one thread per point) walks that list from
//              memory, so the KnnList registers are free again, and counts the 33 bins in a per-thread column of LDS bytes (a
//              runtime-indexed private histogram would live in scratch; counts reach 32 when a point has more than max_nn exact
//              duplicates before it, one more than a 5-bit field of a packed word holds); fpfh_gather forms the weighted sum
//   nearest    one query per thread with its feature in registers (three instantiations by the dimension's cap), targets tiled through
//              LDS and read as broadcasts; the targets split over blockIdx.y, and feature_fold takes the minimum of the partial
//              (d2, index) pairs, a total order, so the result does not depend on the split
//   RANSAC     ransac_gather (the (s, t) pairs, contiguous), ransac_check (every hypothesis: draw, repeated index, edge checker, frames;
//              one status byte each and the survivors per block), ransac_offsets (one workgroup's scan of the block counts),
//              ransac_compact (the survivors' h in ascending order), ransac_score (one survivor per lane with its 12 doubles in
//              registers, a (chunk, survivor tile) grid, correspondences staged in LDS), ransac_select (one workgroup folds the chunk
//              partials in chunk order, selects under the total order and writes the result)
#include "lnr_cloud_knn.h"

#define FN_TILE 64                      // target rows per LDS tile of feature_nearest
#define FN_MAX_SPLIT 512                // blockIdx.y slices of the targets, at most
#define RS_STAGE 512                    // correspondences staged in LDS at a time by ransac_score (a divisor of LNR_RANSAC_CHUNK)
#define RS_MAX_H ((int64_t)1 << 22)

namespace {

__device__ inline void cross3(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// ------------------------------------------------------------------------------------------------ orientation
struct Vec3 { double v[3]; };

// counters: [0] non-finite normals (left as they are), [1] normals flipped
__global__ __launch_bounds__(CL_BLOCK) void orient_normals(const double* __restrict__ points, double* __restrict__ normals, uint32_t n,
                                                           int mode, Vec3 ref, unsigned long long* __restrict__ counters) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    bool bad = false, flip = false;
    if (i < n) {
        double* nv = normals + 3 * (size_t)i;
        const double nn[3] = {nv[0], nv[1], nv[2]};
        bad = !finite3(nn[0], nn[1], nn[2]);
        if (!bad) {
            double d;
            if (mode == LNR_ORIENT_LOCATION) {
                const double* p = points + 3 * (size_t)i;
                const double to[3] = {ref.v[0] - p[0], ref.v[1] - p[1], ref.v[2] - p[2]};
                d = dot3(to, nn);
            } else {
                d = dot3(nn, ref.v);
            }
            flip = d < 0.0;
            if (flip) { nv[0] = -nn[0]; nv[1] = -nn[1]; nv[2] = -nn[2]; }
        }
    }
    wave_count_add(bad, &counters[0]);
    wave_count_add(flip, &counters[1]);
}

// ------------------------------------------------------------------------------------------------ FPFH
// cos and sin of theta_b = -pi + 2 pi b / 11 for b = 1..10 (fp64 literals, correctly rounded): the edges of the angle bins
#define FPFH_EDGE_LITERALS                                                                                                          \
    -0.8412535328311812, -0.5406408174555976, -0.41541501300188644, -0.9096319953545183, 0.14231483827328514, -0.9898214418809327,  \
        0.6548607339452851, -0.7557495743542583, 0.9594929736144974, -0.28173255684142967, 0.9594929736144974, 0.28173255684142967, \
        0.6548607339452851, 0.7557495743542583, 0.14231483827328514, 0.9898214418809327, -0.41541501300188644, 0.9096319953545183,  \
        -0.8412535328311812, 0.5406408174555976
__device__ __constant__ double FPFH_EDGES_DEV[20] = {FPFH_EDGE_LITERALS};
const double FPFH_EDGES_HOST[20] = {FPFH_EDGE_LITERALS};

struct FpfhLayout { size_t fallback, inv, cnt, id, d2, spfh, total; };
FpfhLayout fpfh_layout(int64_t n) {
    FpfhLayout l;
    const size_t N = (size_t)n;
    l.fallback = 0;
    l.inv = align256(4 * N);
    l.cnt = align256(l.inv + 4 * N);
    l.id = align256(l.cnt + 4 * N);
    l.d2 = align256(l.id + 4 * N * LNR_KNN_MAX);
    l.spfh = align256(l.d2 + 8 * N * LNR_KNN_MAX);
    l.total = align256(l.spfh + 8 * N * LNR_FPFH_DIM);
    return l;
}

__device__ inline bool grid_usable(const GridView& g, uint32_t n) { return g.p->status == 0 && g.p->n == n; }

// inv[input index] = sorted slot
__global__ __launch_bounds__(CL_BLOCK) void fpfh_inverse(GridView g, uint32_t n, uint32_t* __restrict__ inv) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (!grid_usable(g, n) || j >= n) return;
    const uint32_t o = g.orig[j];
    if (o < n) inv[o] = j;
}

// lnr_cloud_knn.h's Finish: the entries with d2 < r2 other than the query itself, in list order
struct FpfhListFinish {
    uint32_t* __restrict__ nb_id;
    double* __restrict__ nb_d2;
    uint32_t* __restrict__ nb_cnt;
    double r2;
    uint32_t n;

    __device__ inline void operator()(const GridView& g, const KnnList& L, int k, uint32_t out) const {
        if (out >= n) return;                                  // a grid built for a larger cloud
        const uint32_t m = L.found < (uint32_t)k ? L.found : (uint32_t)k;
        uint32_t c = 0;
        const size_t base = (size_t)out * LNR_KNN_MAX;
#pragma unroll
        for (int j = 0; j < LNR_KNN_MAX; ++j) {
            if ((uint32_t)j < m && L.d[j] < r2 && L.id[j] != out) {
                nb_id[base + c] = L.id[j];
                nb_d2[base + c] = L.d[j];
                ++c;
            }
        }
        nb_cnt[out] = c;
    }
};

__device__ inline int unit_bin(double f) {
    double b = floor(11.0 * ((f + 1.0) * 0.5));
    b = b > 10.0 ? 10.0 : b;
    b = b >= 0.0 ? b : 0.0;                                    // a NaN lands in bin 0
    return (int)b;
}

// the bin of the angle atan2(y, x) in 11 equal parts of [-pi, pi), from the signs of y c_b - x s_b
__device__ inline int angle_bin(double y, double x) {
    if (x == 0.0 && y == 0.0) return 5;
    int c = 0;
    if (y < 0.0) {
#pragma unroll
        for (int b = 1; b <= 5; ++b) c += (y * FPFH_EDGES_DEV[2 * (b - 1)] - x * FPFH_EDGES_DEV[2 * (b - 1) + 1]) >= 0.0 ? 1 : 0;
        return c;
    }
#pragma unroll
    for (int b = 6; b <= 10; ++b) c += (y * FPFH_EDGES_DEV[2 * (b - 1)] - x * FPFH_EDGES_DEV[2 * (b - 1) + 1]) >= 0.0 ? 1 : 0;
    return 5 + c;
}

// one thread per point (input order): the pair features of its neighbour list, counted in an LDS column, times 100 / m.
// counters[3]: points whose own normal is not finite
__global__ __launch_bounds__(CL_BLOCK) void fpfh_spfh(GridView g, uint32_t n, const double* __restrict__ normals,
                                                      const uint32_t* __restrict__ inv, const uint32_t* __restrict__ nb_id,
                                                      const uint32_t* __restrict__ nb_cnt, double* __restrict__ spfh,
                                                      unsigned long long* __restrict__ counters) {
    __shared__ unsigned char hist[LNR_FPFH_DIM * CL_BLOCK];
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool usable = grid_usable(g, n);
    bool bad = false;
    if (usable && i < n) {
        for (int j = 0; j < LNR_FPFH_DIM; ++j) hist[j * CL_BLOCK + threadIdx.x] = 0;
        const double* pp = g.pts + 3 * (size_t)inv[i];
        const double p1[3] = {pp[0], pp[1], pp[2]};
        const double own[3] = {normals[3 * (size_t)i], normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2]};
        bad = !finite3(own[0], own[1], own[2]);
        uint32_t m = nb_cnt[i];
        m = m < LNR_KNN_MAX ? m : LNR_KNN_MAX;
        for (uint32_t s = 0; s < m; ++s) {
            uint32_t k = nb_id[(size_t)i * LNR_KNN_MAX + s];
            k = k < n ? k : i;
            const double* qp = g.pts + 3 * (size_t)inv[k];
            double d[3] = {qp[0] - p1[0], qp[1] - p1[1], qp[2] - p1[2]};
            double n1[3] = {own[0], own[1], own[2]};
            double n2[3] = {normals[3 * (size_t)k], normals[3 * (size_t)k + 1], normals[3 * (size_t)k + 2]};
            int ba = 5, b1 = 5, b2 = 5;                       // the bins of (0, 0, 0)
            const double f3 = sqrt(dot3(d, d));
            if (!bad && finite3(n2[0], n2[1], n2[2]) && f3 != 0.0) {
                const double a1 = dot3(n1, d) / f3, a2 = dot3(n2, d) / f3;
                double f2 = a1;
                if (fabs(a1) < fabs(a2)) {
                    for (int a = 0; a < 3; ++a) {
                        const double t = n1[a];
                        n1[a] = n2[a];
                        n2[a] = t;
                        d[a] = -d[a];
                    }
                    f2 = -a2;
                }
                double v[3], w[3];
                cross3(d, n1, v);
                const double vn = sqrt(dot3(v, v));
                if (vn != 0.0) {
                    for (int a = 0; a < 3; ++a) v[a] = v[a] / vn;
                    cross3(n1, v, w);
                    const double f1 = dot3(v, n2);
                    const double y = dot3(w, n2), x = dot3(n1, n2);
                    ba = angle_bin(y, x);
                    b1 = unit_bin(f1);
                    b2 = unit_bin(f2);
                }
            }
            hist[ba * CL_BLOCK + threadIdx.x] += 1;
            hist[(11 + b1) * CL_BLOCK + threadIdx.x] += 1;
            hist[(22 + b2) * CL_BLOCK + threadIdx.x] += 1;
        }
        const double scale = m ? 100.0 / (double)m : 0.0;
        for (int j = 0; j < LNR_FPFH_DIM; ++j)
            spfh[(size_t)i * LNR_FPFH_DIM + j] = m ? (double)hist[j * CL_BLOCK + threadIdx.x] * scale : 0.0;
    }
    wave_count_add(bad, &counters[3]);
}

// one thread per point: the neighbours' SPFH weighted by 1 / d2 in list order, each 11-bin block scaled to 100, plus its own SPFH
__global__ __launch_bounds__(CL_BLOCK) void fpfh_gather(GridView g, uint32_t n, const uint32_t* __restrict__ nb_id,
                                                        const double* __restrict__ nb_d2, const uint32_t* __restrict__ nb_cnt,
                                                        const double* __restrict__ spfh, double* __restrict__ features) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (!grid_usable(g, n) || i >= n) return;
    double acc[LNR_FPFH_DIM], sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < LNR_FPFH_DIM; ++j) acc[j] = 0.0;
    uint32_t m = nb_cnt[i];
    m = m < LNR_KNN_MAX ? m : LNR_KNN_MAX;
    for (uint32_t s = 0; s < m; ++s) {
        const double d2 = nb_d2[(size_t)i * LNR_KNN_MAX + s];
        if (d2 == 0.0) continue;
        uint32_t k = nb_id[(size_t)i * LNR_KNN_MAX + s];
        k = k < n ? k : i;
        const double* row = spfh + (size_t)k * LNR_FPFH_DIM;
#pragma unroll
        for (int j = 0; j < LNR_FPFH_DIM; ++j) {
            const double val = row[j] / d2;
            acc[j] = acc[j] + val;
            sum[j / 11] = sum[j / 11] + val;
        }
    }
    const double* own = spfh + (size_t)i * LNR_FPFH_DIM;
#pragma unroll
    for (int j = 0; j < LNR_FPFH_DIM; ++j) {
        const double s = sum[j / 11];
        const double a = s != 0.0 ? acc[j] * (100.0 / s) : acc[j];
        features[(size_t)i * LNR_FPFH_DIM + j] = a + own[j];
    }
}

// ------------------------------------------------------------------------------------------------ nearest neighbour in feature space
// One query per thread, its feature in CAP registers; slice blockIdx.y takes the target tiles [y * tiles_per, (y + 1) * tiles_per).
// best_d / best_i: [gridDim.y, n_q]
template <int CAP>
__global__ __launch_bounds__(CL_BLOCK) void feature_nearest(const double* __restrict__ targets, uint32_t n_t,
                                                            const double* __restrict__ queries, uint32_t n_q, int dim,
                                                            uint32_t tiles_per, double* __restrict__ best_d,
                                                            uint32_t* __restrict__ best_i) {
    __shared__ double tile[FN_TILE * LNR_FEATURE_DIM_MAX];
    const uint32_t q = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool active = q < n_q;
    double f[CAP];
#pragma unroll
    for (int j = 0; j < CAP; ++j) f[j] = active && j < dim ? queries[(size_t)q * dim + j] : 0.0;
    double bd = INFINITY;
    uint32_t bi = 0xffffffffu;
    const uint64_t first = (uint64_t)blockIdx.y * tiles_per * FN_TILE;
    uint64_t last = first + (uint64_t)tiles_per * FN_TILE;
    last = last < n_t ? last : n_t;
    for (uint64_t t0 = first; t0 < last; t0 += FN_TILE) {
        const uint32_t rows = (uint32_t)(last - t0 < FN_TILE ? last - t0 : FN_TILE);
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < rows * (uint32_t)dim; e += CL_BLOCK) tile[e] = targets[t0 * dim + e];
        __syncthreads();
        for (uint32_t r = 0; r < rows; ++r) {
            const double* t = tile + r * dim;
            double d2 = 0.0;
#pragma unroll
            for (int j = 0; j < CAP; ++j) {
                if (j < dim) {
                    const double df = f[j] - t[j];
                    d2 = d2 + df * df;
                }
            }
            const uint32_t id = (uint32_t)(t0 + r);
            if (pair_less(d2, id, bd, bi)) { bd = d2; bi = id; }
        }
    }
    if (active) {
        best_d[(size_t)blockIdx.y * n_q + q] = bd;
        best_i[(size_t)blockIdx.y * n_q + q] = bi;
    }
}

__global__ __launch_bounds__(CL_BLOCK) void feature_fold(const double* __restrict__ best_d, const uint32_t* __restrict__ best_i,
                                                         uint32_t n_q, uint32_t split, int32_t* __restrict__ index,
                                                         double* __restrict__ sq_distance) {
    const uint32_t q = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (q >= n_q) return;
    double bd = INFINITY;
    uint32_t bi = 0xffffffffu;
    for (uint32_t y = 0; y < split; ++y) {
        const double d = best_d[(size_t)y * n_q + q];
        const uint32_t id = best_i[(size_t)y * n_q + q];
        if (pair_less(d, id, bd, bi)) { bd = d; bi = id; }
    }
    index[q] = bi == 0xffffffffu ? -1 : (int32_t)bi;
    sq_distance[q] = bd;
}

struct FnLayout { size_t d, i, total; };
FnLayout fn_layout(int64_t n_q) {
    FnLayout l;
    l.d = 0;
    l.i = align256(8 * (size_t)n_q * FN_MAX_SPLIT);
    l.total = align256(l.i + 4 * (size_t)n_q * FN_MAX_SPLIT);
    return l;
}

// ------------------------------------------------------------------------------------------------ RANSAC on correspondences
enum { RS_OK = 0, RS_REPEATED = 1, RS_EDGE = 2, RS_FRAME = 3 };
enum { RS_ST_FEW = 1, RS_ST_NONE = 2, RS_ST_INDEX = 4 };

struct RansacLayout { size_t pairs, status, block_off, surv, head, part_cnt, part_sum, total; };
uint32_t ransac_chunks(int64_t m) { return (uint32_t)((m + LNR_RANSAC_CHUNK - 1) / LNR_RANSAC_CHUNK); }
RansacLayout ransac_layout(int64_t m, int64_t H) {
    RansacLayout l;
    const size_t M = (size_t)m, h = (size_t)H, nb = (h + CL_BLOCK - 1) / CL_BLOCK, nc = ransac_chunks(m);
    l.pairs = 0;
    l.status = align256(48 * M);
    l.block_off = align256(l.status + h);
    l.surv = align256(l.block_off + 4 * (nb + 1));
    l.head = align256(l.surv + 4 * h);                           // uint64 [8]: [0] survivors, [1..3] rejected, [4] bad indices
    l.part_cnt = align256(l.head + 64);
    l.part_sum = align256(l.part_cnt + 4 * h * nc);
    l.total = align256(l.part_sum + 8 * h * nc);
    return l;
}

// pairs[i] = (source[corr[i][0]], target[corr[i][1]]); an index out of range gives a NaN pair (never an inlier, never a frame)
__global__ __launch_bounds__(CL_BLOCK) void ransac_gather(const double* __restrict__ source, uint32_t n_s, const double* __restrict__ target,
                                                          uint32_t n_t, const int32_t* __restrict__ corr, uint32_t m,
                                                          double* __restrict__ pairs, unsigned long long* __restrict__ head) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < m) {
        const int32_t a = corr[2 * (size_t)i], b = corr[2 * (size_t)i + 1];
        bad = a < 0 || (uint32_t)a >= n_s || b < 0 || (uint32_t)b >= n_t;
        for (int c = 0; c < 3; ++c) {
            pairs[6 * (size_t)i + c] = bad ? (double)NAN : source[3 * (size_t)a + c];
            pairs[6 * (size_t)i + 3 + c] = bad ? (double)NAN : target[3 * (size_t)b + c];
        }
    }
    wave_count_add(bad, &head[4]);
}

__device__ inline bool triangle_frame(const double* a, const double* b, const double* c, double F[3][3]) {   // F[k] = e_{k+1}
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double l1 = sqrt(dot3(ab, ab));
    for (int k = 0; k < 3; ++k) F[0][k] = ab[k] / l1;
    double nrm[3];
    cross3(F[0], ac, nrm);
    const double l3 = sqrt(dot3(nrm, nrm));
    for (int k = 0; k < 3; ++k) F[2][k] = nrm[k] / l3;
    cross3(F[2], F[0], F[1]);
    bool ok = true;
    for (int r = 0; r < 3; ++r) ok = ok && finite3(F[r][0], F[r][1], F[r][2]);
    return ok;
}

// hypothesis h: RS_OK and its pose T [12], or why it is rejected.  m >= 3
__device__ inline int ransac_hypothesis(const double* __restrict__ pairs, uint32_t m, uint32_t h, uint64_t seed, double e, double* T) {
    const Philox4 r = philox4x32_10((uint64_t)h, LNR_STREAM_RANSAC, seed);
    const uint32_t i0 = (uint32_t)(((uint64_t)r.x * m) >> 32), i1 = (uint32_t)(((uint64_t)r.y * m) >> 32),
                   i2 = (uint32_t)(((uint64_t)r.z * m) >> 32);
    if (i0 == i1 || i0 == i2 || i1 == i2) return RS_REPEATED;
    const uint32_t idx[3] = {i0, i1, i2};
    double s[3][3], t[3][3];
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) {
            s[k][c] = pairs[6 * (size_t)idx[k] + c];
            t[k][c] = pairs[6 * (size_t)idx[k] + 3 + c];
        }
    if (e != 0.0) {
        for (int k = 0; k < 3; ++k) {
            const int j = (k + 1) % 3;
            const double ls = sqrt(sq_dist(s[k][0], s[k][1], s[k][2], s[j])), lt = sqrt(sq_dist(t[k][0], t[k][1], t[k][2], t[j]));
            if (!(ls >= e * lt && lt >= e * ls)) return RS_EDGE;
        }
    }
    double Fs[3][3], Ft[3][3];
    const bool oks = triangle_frame(s[0], s[1], s[2], Fs), okt = triangle_frame(t[0], t[1], t[2], Ft);
    if (!(oks && okt)) return RS_FRAME;
    double cs[3], ct[3];
    for (int c = 0; c < 3; ++c) {
        cs[c] = ((s[0][c] + s[1][c]) + s[2][c]) / 3.0;
        ct[c] = ((t[0][c] + t[1][c]) + t[2][c]) / 3.0;
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) T[4 * a + b] = (Ft[0][a] * Fs[0][b] + Ft[1][a] * Fs[1][b]) + Ft[2][a] * Fs[2][b];
        T[4 * a + 3] = ct[a] - ((T[4 * a] * cs[0] + T[4 * a + 1] * cs[1]) + T[4 * a + 2] * cs[2]);
    }
    return RS_OK;
}

// every hypothesis once: its status byte, the survivors of each block, the reject counters
__global__ __launch_bounds__(CL_BLOCK) void ransac_check(const double* __restrict__ pairs, uint32_t m, uint32_t H, uint64_t seed, double e,
                                                         unsigned char* __restrict__ status, uint32_t* __restrict__ block_count,
                                                         unsigned long long* __restrict__ head) {
    __shared__ uint32_t lds[4];
    const uint32_t h = blockIdx.x * CL_BLOCK + threadIdx.x;
    int st = -1;
    if (h < H) {
        double T[12];
        st = ransac_hypothesis(pairs, m, h, seed, e, T);
        status[h] = (unsigned char)st;
    }
    uint32_t total;
    block_exclusive_scan(st == RS_OK ? 1u : 0u, lds, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
    wave_count_add(st == RS_REPEATED, &head[1]);
    wave_count_add(st == RS_EDGE, &head[2]);
    wave_count_add(st == RS_FRAME, &head[3]);
}

// one workgroup: block_count [nb] -> its exclusive prefix in place, the total at [nb] and in head[0]
__global__ __launch_bounds__(CL_BLOCK) void ransac_offsets(uint32_t* __restrict__ block_count, uint32_t nb, unsigned long long* __restrict__ head) {
    __shared__ uint32_t lds[4];
    const uint32_t per = (nb + CL_BLOCK - 1) / CL_BLOCK;
    const uint32_t b0 = threadIdx.x * per;
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
    if (threadIdx.x == 0) {
        block_count[nb] = total;
        head[0] = total;
    }
}

__global__ __launch_bounds__(CL_BLOCK) void ransac_compact(const unsigned char* __restrict__ status, uint32_t H,
                                                           const uint32_t* __restrict__ block_off, uint32_t* __restrict__ surv) {
    __shared__ uint32_t lds[4];
    const uint32_t h = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool ok = h < H && status[h] == RS_OK;
    uint32_t total;
    const uint32_t rank = block_exclusive_scan(ok ? 1u : 0u, lds, &total);
    const uint32_t pos = block_off[blockIdx.x] + rank;
    if (ok && pos < H) surv[pos] = h;
}

// blockIdx.x: the chunk of correspondences, blockIdx.y: the tile of 256 survivors; one survivor per lane
__global__ __launch_bounds__(CL_BLOCK) void ransac_score(const double* __restrict__ pairs, uint32_t m, uint32_t H, uint64_t seed, double e,
                                                         double dd, const uint32_t* __restrict__ surv,
                                                         const unsigned long long* __restrict__ head, uint32_t* __restrict__ part_cnt,
                                                         double* __restrict__ part_sum) {
    __shared__ double stage[RS_STAGE * 6];
    const uint64_t n_surv = head[0] < H ? head[0] : H;
    if ((uint64_t)blockIdx.y * CL_BLOCK >= n_surv) return;
    const uint32_t sidx = blockIdx.y * CL_BLOCK + threadIdx.x;
    const bool active = sidx < n_surv;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = 0.0;
    if (active) {
        const uint32_t h = surv[sidx];
        if (h < H) ransac_hypothesis(pairs, m, h, seed, e, T);
    }
    const uint32_t c0 = blockIdx.x * LNR_RANSAC_CHUNK;
    const uint32_t c1 = m - c0 < LNR_RANSAC_CHUNK ? m : c0 + LNR_RANSAC_CHUNK;
    uint32_t cnt = 0;
    double sum = 0.0;
    for (uint32_t b = c0; b < c1; b += RS_STAGE) {
        const uint32_t rows = c1 - b < RS_STAGE ? c1 - b : RS_STAGE;
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < 6 * rows; k += CL_BLOCK) stage[k] = pairs[6 * (size_t)b + k];
        __syncthreads();
        for (uint32_t r = 0; r < rows; ++r) {
            const double* sp = stage + 6 * r;
            const double x = sp[0], y = sp[1], z = sp[2];
            const double px = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
            const double py = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
            const double pz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
            const double d2 = sq_dist(px, py, pz, sp + 3);
            if (d2 < dd) {
                ++cnt;
                sum = sum + d2;
            }
        }
    }
    if (active) {
        part_cnt[(size_t)blockIdx.x * H + sidx] = cnt;
        part_sum[(size_t)blockIdx.x * H + sidx] = sum;
    }
}

__device__ inline bool ransac_better(uint32_t c, double s, uint32_t h, uint32_t bc, double bs, uint32_t bh) {
    return c > bc || (c == bc && (s < bs || (s == bs && h < bh)));
}

// one workgroup: per survivor the chunk partials in chunk order, the best under (count desc, sum asc, h asc), the result.
// m < 3 (nothing else ran): the identity and RS_ST_FEW
__global__ __launch_bounds__(CL_BLOCK) void ransac_select(const double* __restrict__ pairs, uint32_t m, uint32_t H, uint64_t seed, double e,
                                                          uint32_t n_chunks, const uint32_t* __restrict__ surv,
                                                          const unsigned long long* __restrict__ head, const uint32_t* __restrict__ part_cnt,
                                                          const double* __restrict__ part_sum, double* __restrict__ result,
                                                          int64_t* __restrict__ info) {
    __shared__ uint32_t s_cnt[CL_BLOCK], s_h[CL_BLOCK];
    __shared__ double s_sum[CL_BLOCK];
    const bool few = m < 3;
    const uint64_t n_surv = few ? 0 : (head[0] < H ? head[0] : H);
    uint32_t bc = 0, bh = 0xffffffffu;
    double bs = INFINITY;
    for (uint64_t s = threadIdx.x; s < n_surv; s += CL_BLOCK) {
        uint32_t c = 0;
        double sum = 0.0;
        for (uint32_t k = 0; k < n_chunks; ++k) {
            c += part_cnt[(size_t)k * H + s];
            sum = sum + part_sum[(size_t)k * H + s];
        }
        const uint32_t h = surv[s];
        if (ransac_better(c, sum, h, bc, bs, bh)) { bc = c; bs = sum; bh = h; }
    }
    s_cnt[threadIdx.x] = bc;
    s_sum[threadIdx.x] = bs;
    s_h[threadIdx.x] = bh;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int t = 1; t < CL_BLOCK; ++t)
        if (ransac_better(s_cnt[t], s_sum[t], s_h[t], bc, bs, bh)) { bc = s_cnt[t]; bs = s_sum[t]; bh = s_h[t]; }
    double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    const bool none = bh == 0xffffffffu || bh >= H;
    if (!none) ransac_hypothesis(pairs, m, bh, seed, e, T);
    else bc = 0;
    for (int k = 0; k < 12; ++k) result[k] = T[k];
    result[12] = 0.0; result[13] = 0.0; result[14] = 0.0; result[15] = 1.0;
    result[16] = bc ? (double)bc / (double)m : 0.0;
    result[17] = bc ? sqrt(bs / (double)bc) : 0.0;
    const unsigned long long bad = few ? 0ull : head[4];
    info[0] = (few ? RS_ST_FEW : 0) | (!few && none ? RS_ST_NONE : 0) | (bad ? RS_ST_INDEX : 0);
    info[1] = none ? -1 : (int64_t)bh;
    info[2] = (int64_t)bc;
    info[3] = (int64_t)n_surv;
    info[4] = few ? 0 : (int64_t)head[1];
    info[5] = few ? 0 : (int64_t)head[2];
    info[6] = few ? 0 : (int64_t)head[3];
    info[7] = (int64_t)m;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host
extern "C" int lnr_cloud_orient_normals(const double* points, int64_t n_points, double* normals, int32_t mode, const double* reference,
                                        int64_t* counters_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_orient_normals", n_points, "points");
    LNR_REQUIRE(mode == LNR_ORIENT_LOCATION || mode == LNR_ORIENT_DIRECTION, "lnr_cloud_orient_normals: mode must be 0 (location) or 1 (direction), got %d",
                (int)mode);
    LNR_REQUIRE(reference && counters_dev && (n_points == 0 || (normals && (mode == LNR_ORIENT_DIRECTION || points))),
                "lnr_cloud_orient_normals: null argument");
    LNR_REQUIRE(isfinite(reference[0]) && isfinite(reference[1]) && isfinite(reference[2]),
                "lnr_cloud_orient_normals: the reference must be finite, got (%g, %g, %g)", reference[0], reference[1], reference[2]);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = clear_words(counters_dev, 4 * sizeof(int64_t), st, "lnr_cloud_orient_normals", "counters")) return rc;
    if (n_points == 0) return LNR_OK;
    LnrProfScope prof("cloud_orient_normals", st);
    const Vec3 ref{{reference[0], reference[1], reference[2]}};
    hipLaunchKernelGGL(orient_normals, dim3(blocks_for(n_points)), dim3(CL_BLOCK), 0, st, points, normals, (uint32_t)n_points, (int)mode, ref,
                       (unsigned long long*)counters_dev);
    LNR_CHECK_LAUNCH("lnr_cloud_orient_normals");
    return LNR_OK;
}

extern "C" int lnr_fpfh_bin_edges(double* out) {
    LNR_REQUIRE(out != nullptr, "lnr_fpfh_bin_edges: null argument");
    for (int k = 0; k < 20; ++k) out[k] = FPFH_EDGES_HOST[k];
    return LNR_OK;
}

extern "C" size_t lnr_cloud_fpfh_workspace(int64_t n_points) {
    if (!count_ok(n_points)) return 0;
    return fpfh_layout(n_points).total;
}

extern "C" int lnr_cloud_fpfh(const void* grid, int64_t n_points, const double* normals, double radius, int32_t max_nn, double* features,
                              void* workspace, size_t workspace_bytes, int64_t* counters_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_cloud_fpfh", n_points, "points");
    LNR_REQUIRE(max_nn >= 2 && max_nn <= LNR_KNN_MAX, "lnr_cloud_fpfh: max_nn must be in [2, %d], got %d", LNR_KNN_MAX, (int)max_nn);
    LNR_REQUIRE(isfinite(radius) && radius > 0.0, "lnr_cloud_fpfh: radius must be finite and > 0, got %g", radius);
    LNR_REQUIRE(grid && counters_dev && workspace && (n_points == 0 || (normals && features)), "lnr_cloud_fpfh: null argument");
    const FpfhLayout l = fpfh_layout(n_points);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_cloud_fpfh: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = clear_words(counters_dev, 4 * sizeof(int64_t), st, "lnr_cloud_fpfh", "counters")) return rc;
    if (n_points == 0) return LNR_OK;
    LnrProfScope prof("cloud_fpfh", st);
    const GridView g = grid_view(grid, n_points);
    char* ws = (char*)workspace;
    uint32_t* fb = (uint32_t*)(ws + l.fallback);
    uint32_t* inv = (uint32_t*)(ws + l.inv);
    uint32_t* nb_cnt = (uint32_t*)(ws + l.cnt);
    uint32_t* nb_id = (uint32_t*)(ws + l.id);
    double* nb_d2 = (double*)(ws + l.d2);
    double* spfh = (double*)(ws + l.spfh);
    unsigned long long* cnt = (unsigned long long*)counters_dev;
    const uint32_t n = (uint32_t)n_points;
    // inv and the counts start at 0: a grid built for another cloud leaves nothing unwritten that a later kernel reads
    if (int rc = clear_words(ws + l.inv, l.id - l.inv, st, "lnr_cloud_fpfh", "workspace")) return rc;
    hipLaunchKernelGGL(fpfh_inverse, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, g, n, inv);
    enqueue_knn(g, n, (int)max_nn, FpfhListFinish{nb_id, nb_d2, nb_cnt, radius * radius, n}, fb, cnt, st);
    hipLaunchKernelGGL(fpfh_spfh, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, g, n, normals, (const uint32_t*)inv, (const uint32_t*)nb_id,
                       (const uint32_t*)nb_cnt, spfh, cnt);
    hipLaunchKernelGGL(fpfh_gather, dim3(blocks_for(n)), dim3(CL_BLOCK), 0, st, g, n, (const uint32_t*)nb_id, (const double*)nb_d2,
                       (const uint32_t*)nb_cnt, (const double*)spfh, features);
    LNR_CHECK_LAUNCH("lnr_cloud_fpfh");
    return LNR_OK;
}

extern "C" size_t lnr_feature_nearest_workspace(int64_t n_queries) {
    if (!count_ok(n_queries)) return 0;
    return fn_layout(n_queries).total;
}

extern "C" int lnr_feature_nearest(const double* targets, int64_t n_targets, const double* queries, int64_t n_queries, int32_t dim,
                                   int32_t split, int32_t* index, double* sq_distance, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    CL_REQUIRE_COUNTS("lnr_feature_nearest", n_targets, "targets", n_queries, "queries");
    LNR_REQUIRE(dim >= 1 && dim <= LNR_FEATURE_DIM_MAX, "lnr_feature_nearest: dim must be in [1, %d], got %d", LNR_FEATURE_DIM_MAX, (int)dim);
    LNR_REQUIRE(split >= 0 && split <= FN_MAX_SPLIT, "lnr_feature_nearest: split must be in [0, %d], got %d", FN_MAX_SPLIT, (int)split);
    LNR_REQUIRE(workspace && (n_targets == 0 || targets) && (n_queries == 0 || (queries && index && sq_distance)),
                "lnr_feature_nearest: null argument");
    const FnLayout l = fn_layout(n_queries);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_feature_nearest: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    if (n_queries == 0) return LNR_OK;
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("feature_nearest", st);
    const uint32_t n_q = (uint32_t)n_queries, n_t = (uint32_t)n_targets;
    const uint32_t qb = blocks_for(n_q);
    uint32_t tiles = (uint32_t)(((uint64_t)n_t + FN_TILE - 1) / FN_TILE);
    tiles = tiles ? tiles : 1;
    uint32_t want = split ? (uint32_t)split : (FN_MAX_SPLIT / qb ? FN_MAX_SPLIT / qb : 1u);
    want = want < tiles ? want : tiles;
    const uint32_t tiles_per = (tiles + want - 1) / want;
    const uint32_t slices = (tiles + tiles_per - 1) / tiles_per;        // <= want <= FN_MAX_SPLIT, every slice non-empty
    double* bd = (double*)((char*)workspace + l.d);
    uint32_t* bi = (uint32_t*)((char*)workspace + l.i);
    const dim3 grid(qb, slices);
    if (dim <= 8)
        hipLaunchKernelGGL(feature_nearest<8>, grid, dim3(CL_BLOCK), 0, st, targets, n_t, queries, n_q, (int)dim, tiles_per, bd, bi);
    else if (dim <= 40)
        hipLaunchKernelGGL(feature_nearest<40>, grid, dim3(CL_BLOCK), 0, st, targets, n_t, queries, n_q, (int)dim, tiles_per, bd, bi);
    else
        hipLaunchKernelGGL(feature_nearest<LNR_FEATURE_DIM_MAX>, grid, dim3(CL_BLOCK), 0, st, targets, n_t, queries, n_q, (int)dim, tiles_per,
                           bd, bi);
    hipLaunchKernelGGL(feature_fold, dim3(qb), dim3(CL_BLOCK), 0, st, (const double*)bd, (const uint32_t*)bi, n_q, slices, index, sq_distance);
    LNR_CHECK_LAUNCH("lnr_feature_nearest");
    return LNR_OK;
}

extern "C" size_t lnr_ransac_workspace(int64_t n_correspondences, int64_t n_hypotheses) {
    if (!count_ok(n_correspondences) || n_hypotheses < 1 || n_hypotheses > RS_MAX_H) return 0;
    return ransac_layout(n_correspondences, n_hypotheses).total;
}

extern "C" int lnr_ransac_correspondence(const double* source, int64_t n_source, const double* target, int64_t n_target, const int32_t* corr,
                                         int64_t n_correspondences, int64_t n_hypotheses, uint64_t seed, double max_distance,
                                         double edge_similarity, void* workspace, size_t workspace_bytes, double* result_dev,
                                         int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNTS("lnr_ransac_correspondence", n_source, "source points", n_target, "target points");
    CL_REQUIRE_COUNT("lnr_ransac_correspondence", n_correspondences, "correspondences");
    LNR_REQUIRE(n_hypotheses >= 1 && n_hypotheses <= RS_MAX_H, "lnr_ransac_correspondence: n_hypotheses must be in [1, %lld], got %lld",
                (long long)RS_MAX_H, (long long)n_hypotheses);
    LNR_REQUIRE(isfinite(max_distance) && max_distance > 0.0, "lnr_ransac_correspondence: max_distance must be finite and > 0, got %g",
                max_distance);
    LNR_REQUIRE(edge_similarity >= 0.0 && edge_similarity <= 1.0, "lnr_ransac_correspondence: edge_similarity must be in [0, 1], got %g",
                edge_similarity);
    LNR_REQUIRE(workspace && result_dev && info_dev && (n_correspondences == 0 || (corr && source && target)),
                "lnr_ransac_correspondence: null argument");
    const RansacLayout l = ransac_layout(n_correspondences, n_hypotheses);
    LNR_REQUIRE(workspace_bytes >= l.total, "lnr_ransac_correspondence: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("ransac_correspondence", st);
    char* ws = (char*)workspace;
    double* pairs = (double*)(ws + l.pairs);
    unsigned char* status = (unsigned char*)(ws + l.status);
    uint32_t* block_off = (uint32_t*)(ws + l.block_off);
    uint32_t* surv = (uint32_t*)(ws + l.surv);
    unsigned long long* head = (unsigned long long*)(ws + l.head);
    uint32_t* part_cnt = (uint32_t*)(ws + l.part_cnt);
    double* part_sum = (double*)(ws + l.part_sum);
    const uint32_t m = (uint32_t)n_correspondences, H = (uint32_t)n_hypotheses, nb = blocks_for(H), nc = ransac_chunks(m);
    if (int rc = clear_words(head, 64, st, "lnr_ransac_correspondence", "counters")) return rc;
    if (m >= 3) {
        hipLaunchKernelGGL(ransac_gather, dim3(blocks_for(m)), dim3(CL_BLOCK), 0, st, source, (uint32_t)n_source, target, (uint32_t)n_target, corr, m,
                           pairs, head);
        hipLaunchKernelGGL(ransac_check, dim3(nb), dim3(CL_BLOCK), 0, st, (const double*)pairs, m, H, seed, edge_similarity, status, block_off, head);
        hipLaunchKernelGGL(ransac_offsets, dim3(1), dim3(CL_BLOCK), 0, st, block_off, nb, head);
        hipLaunchKernelGGL(ransac_compact, dim3(nb), dim3(CL_BLOCK), 0, st, (const unsigned char*)status, H, (const uint32_t*)block_off, surv);
        hipLaunchKernelGGL(ransac_score, dim3(nc, nb), dim3(CL_BLOCK), 0, st, (const double*)pairs, m, H, seed, edge_similarity,
                           max_distance * max_distance, (const uint32_t*)surv, (const unsigned long long*)head, part_cnt, part_sum);
    }
    hipLaunchKernelGGL(ransac_select, dim3(1), dim3(CL_BLOCK), 0, st, (const double*)pairs, m, H, seed, edge_similarity, nc, (const uint32_t*)surv,
                       (const unsigned long long*)head, (const uint32_t*)part_cnt, (const double*)part_sum, result_dev, info_dev);
    LNR_CHECK_LAUNCH("lnr_ransac_correspondence");
    return LNR_OK;
}
