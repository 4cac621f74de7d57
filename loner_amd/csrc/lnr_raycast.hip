// Ray casting against triangle meshes (gfx950): what a user of open3d's RaycastingScene calls, and the rays of a sweeping LiDAR.
//   RaycastingScene(mesh)                                            lnr_bvh_build
//   RaycastingScene.cast_rays                                        lnr_cast_rays
//   RaycastingScene.compute_closest_points / compute_distance        lnr_closest_points
//   RaycastingScene.count_intersections / compute_occupancy          lnr_count_intersections
//   the rays of a sensor that moves while it sweeps                  lnr_trajectory_rays
// with the definitions stated in include/loner_hip.h ("ray casting").  This file is compiled with -ffp-contract=off (build.py EXACT):
// every fp64 expression of the triangle rule and of the pose rule rounds operation by operation, as the numpy restatement
// (tests/raycast_restatement.py) does.  The tree is an accelerator only: its arithmetic (Morton codes, boxes, padded slab tests) decides
// which triangles a ray meets, never what a meeting returns.  No float goes through an atomic; the integer atomics (counts, box images,
// status) commute.
//   bounds     per triangle: corners in range and finite, else counted and left out; the box of the box centres (atomic min / max of
//              order-preserving images)
//   keys       63-bit Morton code of the centre over that box (an axis without extent contributes 0, nothing is divided by it); a
//              triangle left out gets the key of all ones and sorts behind the tree
//   sort       the stable LSD radix sort of lnr_radix_sort.h; the sorted position breaks ties between equal codes (Karras 2012)
//   leaves     the corners gathered in sorted order, so a leaf is one 72-byte read
//   nodes      Karras' radix tree: one thread per internal node finds its range and its split
//   fit        LNR_BVH_STACK rounds, one launch each: a node takes its children's boxes once both were fitted by an EARLIER launch (a
//              child's round word is compared with the round of the launch), so every box a node reads crossed a kernel boundary;
//              a device word counts the nodes still open and later rounds return at once when it is 0.  Nothing spins.  The round in
//              which the root is fitted is the height of the tree
//   cast       one ray per lane, one wave per workgroup; the stack is a column of LDS per lane (LNR_BVH_STACK words, no private array
//              is indexed at run time); near child first; a node is dropped only when its padded entry distance is strictly greater
//              than the best t, so equal t still reaches the lower index
//   closest    the same walk for a point: the child with the smaller bound first; a node is dropped only when a lower bound of the
//              squared distance to its box is strictly greater than the best so far (box_bound)
//   count      the cast's walk without a best t: every box whose padded slab meets the window is visited
#include "lnr_mesh_args.h"
#include "lnr_radix_sort.h"
#include "lnr_traj.h"

namespace {

enum { RC_ST_BAD_INDEX = 1, RC_ST_TOO_DEEP = 2, RC_ST_VISIT_CAP = 4, RC_ST_STACK = 8, RC_ST_NONFINITE = 1 };

#define RC_WAVE 64
#define RC_MORTON_BITS 21
// the slab test's padding, relative to the largest slab distance of the box: 2^-36, some 10^5 ulps.  The triangle rule's edge functions
// are exact to a few ulps of their products, which for a triangle of edge l seen from a distance L misplaces an edge by about
// 2^-53 L^2 / l; the padding covers L / l up to 10^4 and costs no measurable visit
#define RC_PAD 1.4551915228366852e-11

struct BvhNode {
    double lo[2][3], hi[2][3];      // the boxes of the two children
    int32_t child[2];               // >= 0: an internal node; < 0: ~(sorted position of a leaf)
    int32_t round;                  // the fit round that wrote the boxes; 0: still open
    int32_t pad;
};

// the head of a BVH buffer, written by the build
struct BvhHead {
    uint32_t n_sort;                // pairs the sort works on: every triangle
    int32_t npasses;
    uint32_t n;                     // triangles in the tree
    uint32_t status;                // RC_ST_BAD_INDEX | RC_ST_TOO_DEEP
    uint32_t nonfinite, bad_index;  // triangles left out
    uint32_t open;                  // internal nodes not yet fitted
    uint32_t depth;                 // height of the tree in edges
    unsigned long long lo_img[3], hi_img[3];
    double lo[3], inv[3];           // scene box of the centres: low corner and 2^21 / extent (0 where the extent is 0)
};

struct BvhLayout { size_t head, nodes, leaf_v, leaf_id, total; };
BvhLayout bvh_layout(int64_t f) {
    BvhLayout l;
    l.head = 0;
    l.nodes = align256(sizeof(BvhHead));
    l.leaf_v = align256(l.nodes + sizeof(BvhNode) * (size_t)f);
    l.leaf_id = align256(l.leaf_v + 72 * (size_t)f);
    l.total = align256(l.leaf_id + 4 * (size_t)f);
    return l;
}

// the build's workspace is the sort over f pairs and nothing else
SortLayout build_layout(int64_t f) { return sort_layout(0, f, 0); }

// order-preserving 64-bit image of a double, and back
__device__ inline unsigned long long dbl_image(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double image_dbl(unsigned long long m) {
    return __longlong_as_double((long long)((m >> 63) ? (m & 0x7FFFFFFFFFFFFFFFull) : ~m));
}

__device__ inline double sel3(int k, double x, double y, double z) { return k == 0 ? x : (k == 1 ? y : z); }

// ------------------------------------------------------------------------------------------------ build
__global__ void bvh_head_init(BvhHead* h, uint32_t f) {
    h->n_sort = f;
    h->npasses = CL_MAX_PASSES;
    h->n = 0;
    h->status = 0;
    h->nonfinite = 0;
    h->bad_index = 0;
    h->open = 0;
    h->depth = 0;
    for (int a = 0; a < 3; ++a) {
        h->lo_img[a] = ~0ull;
        h->hi_img[a] = 0ull;
        h->lo[a] = 0.0;
        h->inv[a] = 0.0;
    }
}

// the corners of triangle t -> 0: usable (c holds the 9 coordinates), 1: a non-finite corner, 2: an index outside [0, V)
__device__ inline int load_triangle(const double* __restrict__ v, int64_t n_verts, const int32_t* __restrict__ tri, uint32_t t, double* c) {
    int64_t i[3];
    if (!load_corners(tri, t, n_verts, i)) return 2;
    bool fin = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] = v[3 * (size_t)i[0] + a];
        c[3 + a] = v[3 * (size_t)i[1] + a];
        c[6 + a] = v[3 * (size_t)i[2] + a];
        fin = fin && isfinite(c[a]) && isfinite(c[3 + a]) && isfinite(c[6 + a]);
    }
    return fin ? 0 : 1;
}

__device__ inline double box_centre(const double* c, int a) {
    const double lo = fmin(fmin(c[a], c[3 + a]), c[6 + a]), hi = fmax(fmax(c[a], c[3 + a]), c[6 + a]);
    return 0.5 * lo + 0.5 * hi;
}

__global__ __launch_bounds__(CL_BLOCK) void bvh_bounds(const double* __restrict__ v, int64_t n_verts, const int32_t* __restrict__ tri,
                                                       uint32_t f, BvhHead* h) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    double c[9];
    const int cls = t < f ? load_triangle(v, n_verts, tri, t, c) : -1;
    wave_count_add(cls == 1, &h->nonfinite);
    wave_count_add(cls == 2, &h->bad_index);
    if (cls != 0) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const unsigned long long m = dbl_image(box_centre(c, a));
        atomicMin(&h->lo_img[a], m);
        atomicMax(&h->hi_img[a], m);
    }
}

__global__ void bvh_params(BvhHead* h) {
    const uint32_t n = h->n_sort - h->nonfinite - h->bad_index;
    h->n = n;
    h->open = n > 1 ? n - 1 : 0;
    if (h->bad_index) h->status |= RC_ST_BAD_INDEX;
    for (int a = 0; a < 3; ++a) {
        if (n == 0) continue;
        const double lo = image_dbl(h->lo_img[a]), hi = image_dbl(h->hi_img[a]);
        const double ext = hi - lo;
        h->lo[a] = lo;
        h->inv[a] = (ext > 0.0 && isfinite(ext)) ? (double)(1u << RC_MORTON_BITS) / ext : 0.0;
    }
}

__device__ inline uint64_t spread21(uint64_t x) {      // bit i -> bit 3 i
    x &= 0x1FFFFFull;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ __launch_bounds__(CL_BLOCK) void bvh_keys(const double* __restrict__ v, int64_t n_verts, const int32_t* __restrict__ tri,
                                                     uint32_t f, const BvhHead* __restrict__ h, uint64_t* __restrict__ keys,
                                                     uint32_t* __restrict__ idx) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (t >= f) return;
    double c[9];
    uint64_t key = ~0ull;
    if (load_triangle(v, n_verts, tri, t, c) == 0) {
        key = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double q = (box_centre(c, a) - h->lo[a]) * h->inv[a];
            q = fmin(fmax(q, 0.0), (double)((1u << RC_MORTON_BITS) - 1u));      // fmax drops a NaN
            key |= spread21((uint64_t)q) << (2 - a);
        }
    }
    keys[t] = key;
    idx[t] = t;
}

__global__ __launch_bounds__(CL_BLOCK) void bvh_leaves(const double* __restrict__ v, int64_t n_verts, const int32_t* __restrict__ tri,
                                                       const BvhHead* __restrict__ h, SortedPairs sp, double* __restrict__ leaf_v,
                                                       int32_t* __restrict__ leaf_id) {
    const uint32_t j = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (j >= h->n) return;
    const uint32_t t = sp.idx(h->npasses)[j];
    double c[9];
    load_triangle(v, n_verts, tri, t, c);               // usable: it sorted in front of the keys of all ones
#pragma unroll
    for (int e = 0; e < 9; ++e) leaf_v[9 * (size_t)j + e] = c[e];
    leaf_id[j] = (int32_t)t;
}

// the length of the common prefix of the keys at sorted positions i and j, the position itself breaking ties; -1 outside [0, n)
__device__ inline int prefix_len(const uint64_t* __restrict__ k, uint32_t n, int64_t i, int64_t j) {
    if (j < 0 || j >= (int64_t)n) return -1;
    const uint64_t x = k[i] ^ k[j];
    return x ? __clzll((long long)x) : 64 + __clz((int)((uint32_t)i ^ (uint32_t)j));
}

__global__ __launch_bounds__(CL_BLOCK) void bvh_nodes(const BvhHead* __restrict__ h, const uint64_t* __restrict__ ka,
                                                      const uint64_t* __restrict__ kb, BvhNode* __restrict__ nodes) {
    const uint32_t n = h->n;
    const int64_t i = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (n < 2 || i >= (int64_t)n - 1) return;
    const uint64_t* k = sorted_keys(h->npasses, ka, kb);
    const int d = prefix_len(k, n, i, i + 1) > prefix_len(k, n, i, i - 1) ? 1 : -1;
    const int dmin = prefix_len(k, n, i, i - d);
    int64_t lmax = 2;
    while (prefix_len(k, n, i, i + lmax * d) > dmin) lmax <<= 1;          // ends: the prefix is -1 outside the array
    int64_t l = 0;
    for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
        if (prefix_len(k, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = prefix_len(k, n, i, j);
    int64_t s = 0;
    for (int64_t t = (l + 1) >> 1;; t = (t + 1) >> 1) {
        if (prefix_len(k, n, i, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    BvhNode* nd = nodes + i;
    nd->child[0] = first == g ? ~(int32_t)g : (int32_t)g;
    nd->child[1] = last == g + 1 ? ~(int32_t)(g + 1) : (int32_t)(g + 1);
    nd->round = 0;
    nd->pad = 0;
}

// one round of the fit.  A child counts as fitted only when its round word is below this launch's round: its boxes were then written
// by an earlier launch and the kernel boundary made them visible.  A word written during this launch, seen or not, leaves the node open
__global__ __launch_bounds__(CL_BLOCK) void bvh_fit(BvhHead* h, BvhNode* __restrict__ nodes, const double* __restrict__ leaf_v, int32_t round) {
    if (h->open == 0) return;
    const uint32_t n = h->n;
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    bool done = false;
    if (n >= 2 && i < n - 1 && nodes[i].round == 0) {
        BvhNode* nd = nodes + i;
        double lo[2][3], hi[2][3];
        bool ready = true;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int32_t c = nd->child[s];
            if (c < 0) {
                const double* p = leaf_v + 9 * (size_t)(uint32_t)(~c);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    lo[s][a] = fmin(fmin(p[a], p[3 + a]), p[6 + a]);
                    hi[s][a] = fmax(fmax(p[a], p[3 + a]), p[6 + a]);
                }
            } else {
                const BvhNode* q = nodes + c;
                const int32_t r = q->round;
                if (r == 0 || r >= round) {
                    ready = false;
                } else {
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        lo[s][a] = fmin(q->lo[0][a], q->lo[1][a]);
                        hi[s][a] = fmax(q->hi[0][a], q->hi[1][a]);
                    }
                }
            }
        }
        if (ready) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    nd->lo[s][a] = lo[s][a];
                    nd->hi[s][a] = hi[s][a];
                }
            nd->round = round;
            if (i == 0) h->depth = (uint32_t)round;
            done = true;
        }
    }
    const unsigned long long m = __ballot(done);
    if (m && (threadIdx.x & 63) == 0) atomicSub(&h->open, (uint32_t)__popcll(m));
}

__global__ void bvh_info(BvhHead* h, int64_t* __restrict__ info) {
    if (h->open != 0 || h->depth >= LNR_BVH_STACK) h->status |= RC_ST_TOO_DEEP;
    info[0] = h->status;
    info[1] = h->n;
    info[2] = h->nonfinite;
    info[3] = h->bad_index;
    info[4] = h->depth;
    info[5] = h->n > 1 ? 2 * (int64_t)h->n - 1 : h->n;
    info[6] = 0;
    info[7] = 0;
}

// ------------------------------------------------------------------------------------------------ cast
struct RayCtx {
    double o[3], inv[3];            // origin; 1 / d, 0 marks an axis the ray does not move along (d = 0, or 1 / d not finite)
    bool par[3];
    int kx, ky, kz;
    double sx, sy, sz;
    double okx, oky, okz;
    double t_min, t_max;
};

// the padded slab test -> false: the box can hold no accepted hit with t <= best; entry: the padded entry distance.  Every compare is
// written so that a NaN keeps the box
__device__ inline bool slab(const RayCtx& r, const double* lo, const double* hi, double best, double* entry_out) {
    double entry = -INFINITY, exit = INFINITY, scale = 0.0;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double dl = lo[a] - r.o[a], dh = hi[a] - r.o[a];
        if (r.par[a]) {
            const double p = RC_PAD * fmax(fabs(dl), fabs(dh));
            if (dl > p || dh < -p) inside = false;
        } else {
            const double t1 = dl * r.inv[a], t2 = dh * r.inv[a];
            entry = fmax(entry, fmin(t1, t2));
            exit = fmin(exit, fmax(t1, t2));
            scale = fmax(scale, fmax(fabs(t1), fabs(t2)));
        }
    }
    const double pad = RC_PAD * scale;
    entry -= pad;
    exit += pad;
    *entry_out = entry;
    return inside && !(entry > exit) && !(entry > best) && !(exit < r.t_min) && !(entry > r.t_max);
}

// the watertight rule of include/loner_hip.h on the triangle at sorted position j -> accepted; t, and U, V, det for the barycentrics
__device__ inline bool hit_rule(const RayCtx& r, const double* __restrict__ leaf_v, uint32_t j, double* t_out, double* U_out, double* V_out,
                                double* det_out) {
    const double* p = leaf_v + 9 * (size_t)j;
    const double a0 = p[0] - r.o[0], a1 = p[1] - r.o[1], a2 = p[2] - r.o[2];
    const double b0 = p[3] - r.o[0], b1 = p[4] - r.o[1], b2 = p[5] - r.o[2];
    const double c0 = p[6] - r.o[0], c1 = p[7] - r.o[1], c2 = p[8] - r.o[2];
    const double akz = sel3(r.kz, a0, a1, a2), bkz = sel3(r.kz, b0, b1, b2), ckz = sel3(r.kz, c0, c1, c2);
    const double ax = sel3(r.kx, a0, a1, a2) - r.sx * akz, ay = sel3(r.ky, a0, a1, a2) - r.sy * akz;
    const double bx = sel3(r.kx, b0, b1, b2) - r.sx * bkz, by = sel3(r.ky, b0, b1, b2) - r.sy * bkz;
    const double cx = sel3(r.kx, c0, c1, c2) - r.sx * ckz, cy = sel3(r.ky, c0, c1, c2) - r.sy * ckz;
    const double U = cx * by - cy * bx, V = ax * cy - ay * cx, W = bx * ay - by * ax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;
    const double det = (U + V) + W;
    if (det == 0.0) return false;
    const double t = ((U * (r.sz * akz) + V * (r.sz * bkz)) + W * (r.sz * ckz)) / det;
    if (!(t >= r.t_min && t <= r.t_max)) return false;
    *t_out = t;
    *U_out = U;
    *V_out = V;
    *det_out = det;
    return true;
}

__device__ inline void hit_leaf(const RayCtx& r, const double* __restrict__ leaf_v, const int32_t* __restrict__ leaf_id, uint32_t j,
                                double* best_t, int32_t* best_id, double* best_u, double* best_v) {
    double t, U, V, det;
    if (!hit_rule(r, leaf_v, j, &t, &U, &V, &det)) return;
    const int32_t id = leaf_id[j];
    if (t < *best_t || (t == *best_t && id < *best_id)) {
        *best_t = t;
        *best_id = id;
        *best_u = U / det;
        *best_v = V / det;
    }
}

// ray i of rays [n,6] -> false: not finite or a zero direction; else r holds what the slab test and the triangle rule need
__device__ inline bool ray_setup(const double* __restrict__ rays, uint32_t i, double t_min, double t_max, RayCtx& r) {
    double d[3];
    bool fin = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.o[a] = rays[6 * (size_t)i + a];
        d[a] = rays[6 * (size_t)i + 3 + a];
        fin = fin && isfinite(r.o[a]) && isfinite(d[a]);
    }
    if (!fin || (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double inv = 1.0 / d[a];
        r.par[a] = d[a] == 0.0 || !isfinite(inv);
        r.inv[a] = r.par[a] ? 0.0 : inv;
    }
    int kz = 0;
    if (fabs(d[1]) > fabs(d[0])) kz = 1;
    if (fabs(d[2]) > fabs(sel3(kz, d[0], d[1], d[2]))) kz = 2;
    int kx = (kz + 1) % 3, ky = (kx + 1) % 3;
    const double dkz = sel3(kz, d[0], d[1], d[2]);
    if (dkz < 0.0) { const int s = kx; kx = ky; ky = s; }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.sx = sel3(kx, d[0], d[1], d[2]) / dkz;
    r.sy = sel3(ky, d[0], d[1], d[2]) / dkz;
    r.sz = 1.0 / dkz;
    r.t_min = t_min;
    r.t_max = t_max;
    return true;
}

// the usable triangles and the visit cap of a walk: none when the build set a status bit
__device__ inline uint32_t walk_size(const BvhHead* __restrict__ h, unsigned long long* cap) {
    const uint32_t n = (h->status & (RC_ST_BAD_INDEX | RC_ST_TOO_DEEP)) ? 0u : h->n;
    *cap = 2ull * (n > 1 ? 2ull * n - 1ull : (unsigned long long)n);
    return n;
}

// a call's counts: one atomic per wave and quantity
__device__ inline void wave_tally(uint32_t lane, bool found, bool invalid, bool capped, bool overflow, unsigned long long visits,
                                  unsigned long long* __restrict__ tally) {
    const unsigned long long hits = __ballot(found), bad = __ballot(invalid), cp = __ballot(capped), ov = __ballot(overflow);
    unsigned long long vs = visits;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vs += __shfl_xor(vs, o, 64);
    if (lane == 0) {
        if (hits) atomicAdd(&tally[0], (unsigned long long)__popcll(hits));
        if (bad) atomicAdd(&tally[1], (unsigned long long)__popcll(bad));
        if (vs) atomicAdd(&tally[2], vs);
        if (cp) atomicAdd(&tally[3], (unsigned long long)__popcll(cp));
        if (ov) atomicAdd(&tally[4], (unsigned long long)__popcll(ov));
    }
}

// The walk the three queries share, one node per turn: leaf(sorted position) tests a triangle; boxes(node, &h0, &h1) says which
// children to enter and returns whether child 0 goes first.  The other child waits in the lane's stack column; a full column drops it
// and reports it, and cap visits end any walk
template <class Boxes, class Leaf>
__device__ inline void walk(const BvhNode* __restrict__ nodes, uint32_t n, unsigned long long cap, int32_t (*stack)[RC_WAVE], uint32_t lane,
                            Boxes boxes, Leaf leaf, unsigned long long* visits_out, bool* capped, bool* overflow) {
    unsigned long long visits = 0;
    int sp = 0;
    int32_t node = n == 1 ? ~0 : 0;
    for (;;) {
        if (visits >= cap) { *capped = true; break; }
        ++visits;
        bool pop = true;
        if (node < 0) {
            leaf((uint32_t)(~node));
        } else {
            const BvhNode* nd = nodes + node;
            bool h0, h1;
            const bool first0 = boxes(nd, &h0, &h1);
            const int32_t c0 = nd->child[0], c1 = nd->child[1];
            if (h0 && h1) {
                if (sp < LNR_BVH_STACK) {
                    stack[sp][lane] = first0 ? c1 : c0;
                    ++sp;
                } else {
                    *overflow = true;
                }
                node = first0 ? c0 : c1;
                pop = false;
            } else if (h0 || h1) {
                node = h0 ? c0 : c1;
                pop = false;
            }
        }
        if (pop) {
            if (sp == 0) break;
            --sp;
            node = stack[sp][lane];
        }
    }
    *visits_out = visits;
}

__global__ __launch_bounds__(RC_WAVE) void cast_rays_kernel(const BvhHead* __restrict__ h, const BvhNode* __restrict__ nodes,
                                                            const double* __restrict__ leaf_v, const int32_t* __restrict__ leaf_id,
                                                            const double* __restrict__ rays, uint32_t n_rays, double t_min, double t_max,
                                                            double* __restrict__ t_hit, int32_t* __restrict__ ids, double* __restrict__ uvs,
                                                            unsigned long long* __restrict__ tally) {
    __shared__ int32_t stack[LNR_BVH_STACK][RC_WAVE];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x * RC_WAVE + lane;
    unsigned long long cap;
    const uint32_t n = walk_size(h, &cap);
    double best_t = INFINITY, best_u = 0.0, best_v = 0.0;
    int32_t best_id = -1;
    unsigned long long visits = 0;
    bool invalid = false, capped = false, overflow = false;
    if (i < n_rays) {
        RayCtx r;
        invalid = !ray_setup(rays, i, t_min, t_max, r);
        if (!invalid && n > 0) {
            walk(nodes, n, cap, stack, lane,
                 [&](const BvhNode* nd, bool* h0, bool* h1) {
                     double e0, e1;
                     *h0 = slab(r, nd->lo[0], nd->hi[0], best_t, &e0);
                     *h1 = slab(r, nd->lo[1], nd->hi[1], best_t, &e1);
                     return !(e1 < e0);
                 },
                 [&](uint32_t j) { hit_leaf(r, leaf_v, leaf_id, j, &best_t, &best_id, &best_u, &best_v); }, &visits, &capped, &overflow);
        }
        t_hit[i] = best_t;
        ids[i] = best_id;
        if (uvs) {
            uvs[2 * (size_t)i] = best_u;
            uvs[2 * (size_t)i + 1] = best_v;
        }
    }
    wave_tally(lane, best_id >= 0, invalid, capped, overflow, visits, tally);
}

// info_dev doubles as the tally while a walk (cast, closest points, crossing counts) runs (words 1..5); this puts the words in their
// stated places
__global__ void cast_info(const BvhHead* __restrict__ h, int64_t* __restrict__ info) {
    const int64_t capped = info[4], overflow = info[5];
    info[0] = (int64_t)(h->status & (RC_ST_BAD_INDEX | RC_ST_TOO_DEEP)) | (capped ? RC_ST_VISIT_CAP : 0) | (overflow ? RC_ST_STACK : 0);
    info[5] = h->nonfinite + h->bad_index;
    info[6] = h->depth;
    info[7] = 0;
}

// ------------------------------------------------------------------------------------------------ closest points
// Ericson's region walk as include/loner_hip.h states it, on the triangle at sorted position j: the candidate replaces the best when
// the answer rule says so
__device__ inline void closest_leaf(const double* p, double max_d2, const double* __restrict__ leaf_v, const int32_t* __restrict__ leaf_id,
                                    uint32_t j, double* best_d2, int32_t* best_id, double* best_q, double* best_u, double* best_v) {
    const double* c = leaf_v + 9 * (size_t)j;
    double A[3], B[3], ab[3], ac[3], ap[3], bp[3], cp[3], q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        A[a] = c[a];
        B[a] = c[3 + a];
        ab[a] = c[3 + a] - c[a];
        ac[a] = c[6 + a] - c[a];
        ap[a] = p[a] - c[a];
        bp[a] = p[a] - c[3 + a];
        cp[a] = p[a] - c[6 + a];
    }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double vB, wC;                                      // the weights of B and C
    if (d1 <= 0.0 && d2 <= 0.0) {
        vB = 0.0; wC = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = A[a];
    } else if (d3 >= 0.0 && d4 <= d3) {
        vB = 1.0; wC = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = B[a];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        vB = d1 / (d1 - d3); wC = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = A[a] + vB * ab[a];
    } else if (d6 >= 0.0 && d5 <= d6) {
        vB = 0.0; wC = 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = c[6 + a];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        vB = 0.0; wC = d2 / (d2 - d6);
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = A[a] + wC * ac[a];
    } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        wC = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        vB = 1.0 - wC;
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = B[a] + wC * (c[6 + a] - B[a]);
    } else {
        const double den = 1.0 / ((va + vb) + vc);
        vB = vb * den; wC = vc * den;
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = (A[a] + ab[a] * vB) + ac[a] * wC;
    }
    double pq[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) pq[a] = p[a] - q[a];
    const double dd = dot3(pq, pq);
    if (!(dd <= max_d2)) return;                        // a NaN is no candidate
    const int32_t id = leaf_id[j];
    if (*best_id < 0 || dd < *best_d2 || (dd == *best_d2 && id < *best_id)) {
        *best_d2 = dd;
        *best_id = id;
        best_q[0] = q[0]; best_q[1] = q[1]; best_q[2] = q[2];
        *best_u = (1.0 - vB) - wC;
        *best_v = vB;
    }
}

// A lower bound of every squared distance closest_leaf computes for a triangle inside the box [lo, hi].  With M = max(|lo_a|, |hi_a|,
// |p_a|): the computed q_a is a convex combination of corners in [lo_a, hi_a] up to the rounding of the rule's own operations; with
// weights in [0, 1] that is a few ulps of M, and inside the triangle, where the weights come from differences of products of the d's,
// about 2^-53 M r^2 for a triangle of aspect ratio r = edge^2 / (2 area).  So |p_a - q_a| >= g_a - e M with g_a = max(lo_a - p_a,
// p_a - hi_a, 0), and the relative part alone would not do: at a box face g_a is 0 or tiny while e M is not, hence the absolute
// reduction by RC_PAD M (2^-36 M: 10^5 ulps of M, r up to 300) and the clamp at 0.  Rounding is monotone, so with reduced gaps no
// larger than |p_a - q_a| their squares, summed in dot3's order, are no larger than the computed dot3(p - q, p - q).  A NaN cannot
// arise: p is finite here and so are the boxes of usable triangles
__device__ inline double box_bound(const double* p, const double* lo, const double* hi) {
    double g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double gap = fmax(fmax(lo[a] - p[a], p[a] - hi[a]), 0.0);
        g[a] = fmax(gap - RC_PAD * fmax(fmax(fabs(lo[a]), fabs(hi[a])), fabs(p[a])), 0.0);
    }
    return dot3(g, g);
}

__global__ __launch_bounds__(RC_WAVE) void closest_points_kernel(const BvhHead* __restrict__ h, const BvhNode* __restrict__ nodes,
                                                                 const double* __restrict__ leaf_v, const int32_t* __restrict__ leaf_id,
                                                                 const double* __restrict__ points, uint32_t n_points, double max_d2,
                                                                 double* __restrict__ dist_sq, int32_t* __restrict__ ids,
                                                                 double* __restrict__ closest, double* __restrict__ uvs,
                                                                 unsigned long long* __restrict__ tally) {
    __shared__ int32_t stack[LNR_BVH_STACK][RC_WAVE];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x * RC_WAVE + lane;
    unsigned long long cap;
    const uint32_t n = walk_size(h, &cap);
    double best_d2 = INFINITY, best_u = 0.0, best_v = 0.0, best_q[3] = {0.0, 0.0, 0.0};
    int32_t best_id = -1;
    unsigned long long visits = 0;
    bool invalid = false, capped = false, overflow = false;
    if (i < n_points) {
        const double p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
        invalid = !finite3(p[0], p[1], p[2]);
        if (!invalid && n > 0) {
            walk(nodes, n, cap, stack, lane,
                 [&](const BvhNode* nd, bool* h0, bool* h1) {
                     const double b0 = box_bound(p, nd->lo[0], nd->hi[0]), b1 = box_bound(p, nd->lo[1], nd->hi[1]);
                     *h0 = !(b0 > best_d2) && !(b0 > max_d2);
                     *h1 = !(b1 > best_d2) && !(b1 > max_d2);
                     return !(b1 < b0);
                 },
                 [&](uint32_t j) { closest_leaf(p, max_d2, leaf_v, leaf_id, j, &best_d2, &best_id, best_q, &best_u, &best_v); }, &visits,
                 &capped, &overflow);
        }
        dist_sq[i] = best_d2;
        ids[i] = best_id;
        if (closest) {
            closest[3 * (size_t)i] = best_q[0];
            closest[3 * (size_t)i + 1] = best_q[1];
            closest[3 * (size_t)i + 2] = best_q[2];
        }
        if (uvs) {
            uvs[2 * (size_t)i] = best_u;
            uvs[2 * (size_t)i + 1] = best_v;
        }
    }
    wave_tally(lane, best_id >= 0, invalid, capped, overflow, visits, tally);
}

// ------------------------------------------------------------------------------------------------ crossing counts
__global__ __launch_bounds__(RC_WAVE) void count_intersections_kernel(const BvhHead* __restrict__ h, const BvhNode* __restrict__ nodes,
                                                                      const double* __restrict__ leaf_v, const double* __restrict__ rays,
                                                                      uint32_t n_rays, double t_min, double t_max,
                                                                      int32_t* __restrict__ counts, unsigned long long* __restrict__ tally) {
    __shared__ int32_t stack[LNR_BVH_STACK][RC_WAVE];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x * RC_WAVE + lane;
    unsigned long long cap;
    const uint32_t n = walk_size(h, &cap);
    int32_t count = 0;
    unsigned long long visits = 0;
    bool invalid = false, capped = false, overflow = false;
    if (i < n_rays) {
        RayCtx r;
        invalid = !ray_setup(rays, i, t_min, t_max, r);
        if (!invalid && n > 0) {
            walk(nodes, n, cap, stack, lane,
                 [&](const BvhNode* nd, bool* h0, bool* h1) {
                     double e0, e1;
                     *h0 = slab(r, nd->lo[0], nd->hi[0], INFINITY, &e0);
                     *h1 = slab(r, nd->lo[1], nd->hi[1], INFINITY, &e1);
                     return true;
                 },
                 [&](uint32_t j) {
                     double t, U, V, det;
                     if (hit_rule(r, leaf_v, j, &t, &U, &V, &det)) ++count;
                 },
                 &visits, &capped, &overflow);
        }
        counts[i] = count;
    }
    wave_tally(lane, count > 0, invalid, capped, overflow, visits, tally);
}

// ------------------------------------------------------------------------------------------------ trajectory rays
// sin and cos of theta >= 0 as include/loner_hip.h states them: plain fp64 operations in a fixed order, so that the numpy restatement
// gives the same bits on any host (a library sine is good to an ulp, and which ulp differs between libraries)
__device__ inline void stated_sincos(double theta, double* s_out, double* c_out) {
    const double kf = floor(theta * 0.6366197723675814 + 0.5);
    const double r = (theta - kf * 1.5707963267948966) - kf * 6.123233995736766e-17;
    const double z = r * r;
    double ps = 1.0, pc = 1.0;
#pragma unroll
    for (int k = 10; k >= 1; --k) {
        ps = 1.0 - (z * ps) / (double)((2 * k) * (2 * k + 1));
        pc = 1.0 - (z * pc) / (double)((2 * k - 1) * (2 * k));
    }
    const double S = r * ps, C = pc;
    const int q = (int)fmod(kf, 4.0);
    *s_out = q == 0 ? S : (q == 1 ? C : (q == 2 ? -S : -C));
    *c_out = q == 0 ? C : (q == 1 ? -S : (q == 2 ? -C : S));
}

// the pose rule of lnr_traj.h with the stated sine, applied to a direction; the origin is the interpolated translation
__global__ __launch_bounds__(CL_BLOCK) void traj_rays(const float* __restrict__ dirs, const double* __restrict__ stamps, uint32_t n, TrajView tv,
                                                      double* __restrict__ rays, unsigned long long* __restrict__ tally) {
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    int cls = -1;                                               // 0: a ray, 1: outside the trajectory, 2: non-finite
    if (i < n) {
        const double x = (double)dirs[i], y = (double)dirs[(size_t)n + i], z = (double)dirs[2 * (size_t)n + i], tau = stamps[i];
        double out[6];
        if (!(finite3(x, y, z) && isfinite(tau))) cls = 2;
        else if (tau < tv.T[0] || tau > tv.T[tv.K - 1]) cls = 1;
        else cls = 0;
        if (cls != 0) {
#pragma unroll
            for (int e = 0; e < 6; ++e) out[e] = NAN;
        } else {
            double R[9];
            traj_pose<stated_sincos>(tv, tau, R, out);
#pragma unroll
            for (int a = 0; a < 3; ++a) out[3 + a] = (R[3 * a] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z;
        }
#pragma unroll
        for (int e = 0; e < 6; ++e) rays[6 * (size_t)i + e] = out[e];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) wave_count_add(cls == c, &tally[c]);
}

// tally {rays, outside, non-finite} in words 1..3 -> the stated info
__global__ void traj_rays_info(int64_t* __restrict__ info) {
    info[0] = info[3] ? RC_ST_NONFINITE : 0;
    for (int e = 4; e < 8; ++e) info[e] = 0;
}

}  // namespace

extern "C" size_t lnr_bvh_workspace(int64_t n_triangles) {
    if (!count_ok(n_triangles)) return 0;
    return build_layout(n_triangles).end;
}

extern "C" size_t lnr_bvh_bytes(int64_t n_triangles) {
    if (!count_ok(n_triangles)) return 0;
    return bvh_layout(n_triangles).total;
}

extern "C" int lnr_bvh_build(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, void* workspace,
                             size_t workspace_bytes, void* bvh, size_t bvh_bytes, int64_t* info_dev, void* stream) {
    LNR_REQUIRE(mesh_counts_ok(n_vertices, n_triangles, CL_MAX_POINTS),
                "lnr_bvh_build: %lld vertices and %lld triangles, the limits are %d and %lld", (long long)n_vertices, (long long)n_triangles,
                INT32_MAX, (long long)CL_MAX_POINTS);
    LNR_REQUIRE(info_dev && workspace && bvh && (n_triangles == 0 || triangles) && (n_vertices == 0 || vertices),
                "lnr_bvh_build: null argument");
    const SortLayout l = build_layout(n_triangles);
    const BvhLayout b = bvh_layout(n_triangles);
    LNR_REQUIRE(workspace_bytes >= l.end, "lnr_bvh_build: workspace of %zu bytes, %zu needed", workspace_bytes, l.end);
    LNR_REQUIRE(bvh_bytes >= b.total, "lnr_bvh_build: a BVH buffer of %zu bytes, %zu needed", bvh_bytes, b.total);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("bvh_build", st);
    char *ws = (char*)workspace, *bb = (char*)bvh;
    BvhHead* h = (BvhHead*)(bb + b.head);
    BvhNode* nodes = (BvhNode*)(bb + b.nodes);
    double* leaf_v = (double*)(bb + b.leaf_v);
    int32_t* leaf_id = (int32_t*)(bb + b.leaf_id);
    const uint32_t f = (uint32_t)n_triangles;
    hipLaunchKernelGGL(bvh_head_init, dim3(1), dim3(1), 0, st, h, f);
    if (f > 0) {
        const RadixBuffers r = radix_buffers(ws, l);
        const uint32_t nb = blocks_for(f);
        hipLaunchKernelGGL(bvh_bounds, dim3(nb), dim3(CL_BLOCK), 0, st, vertices, n_vertices, triangles, f, h);
        hipLaunchKernelGGL(bvh_params, dim3(1), dim3(1), 0, st, h);
        hipLaunchKernelGGL(bvh_keys, dim3(nb), dim3(CL_BLOCK), 0, st, vertices, n_vertices, triangles, f, (const BvhHead*)h, r.ka, r.ia);
        LNR_CHECK_LAUNCH("lnr_bvh_build");
        enqueue_radix_sort(r, &h->n_sort, &h->npasses, st);
        hipLaunchKernelGGL(bvh_leaves, dim3(nb), dim3(CL_BLOCK), 0, st, vertices, n_vertices, triangles, (const BvhHead*)h, sorted_pairs(r),
                           leaf_v, leaf_id);
        hipLaunchKernelGGL(bvh_nodes, dim3(nb), dim3(CL_BLOCK), 0, st, (const BvhHead*)h, (const uint64_t*)r.ka, (const uint64_t*)r.kb, nodes);
        for (int32_t round = 1; round <= LNR_BVH_STACK; ++round)
            hipLaunchKernelGGL(bvh_fit, dim3(nb), dim3(CL_BLOCK), 0, st, h, nodes, (const double*)leaf_v, round);
    }
    hipLaunchKernelGGL(bvh_info, dim3(1), dim3(1), 0, st, h, info_dev);
    LNR_CHECK_LAUNCH("lnr_bvh_build");
    return LNR_OK;
}

extern "C" int lnr_cast_rays(const void* bvh, int64_t n_triangles, const double* rays, int64_t n_rays, double t_min, double t_max,
                             double* t_hit, int32_t* primitive_ids, double* primitive_uvs, int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNTS("lnr_cast_rays", n_triangles, "triangles", n_rays, "rays");
    LNR_REQUIRE(!(t_min != t_min) && !(t_max != t_max), "lnr_cast_rays: t_min or t_max is NaN");
    LNR_REQUIRE(bvh && info_dev && (n_rays == 0 || (rays && t_hit && primitive_ids)), "lnr_cast_rays: null argument");
    const BvhLayout b = bvh_layout(n_triangles);
    const char* bb = (const char*)bvh;
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("cast_rays", st);
    if (int rc = clear_words(info_dev, 8 * sizeof(int64_t), st, "lnr_cast_rays", "info words")) return rc;
    if (n_rays > 0)
        hipLaunchKernelGGL(cast_rays_kernel, dim3((uint32_t)((n_rays + RC_WAVE - 1) / RC_WAVE)), dim3(RC_WAVE), 0, st,
                           (const BvhHead*)(bb + b.head), (const BvhNode*)(bb + b.nodes), (const double*)(bb + b.leaf_v),
                           (const int32_t*)(bb + b.leaf_id), rays, (uint32_t)n_rays, t_min, t_max, t_hit, primitive_ids, primitive_uvs,
                           (unsigned long long*)(info_dev + 1));
    hipLaunchKernelGGL(cast_info, dim3(1), dim3(1), 0, st, (const BvhHead*)(bb + b.head), info_dev);
    LNR_CHECK_LAUNCH("lnr_cast_rays");
    return LNR_OK;
}

extern "C" int lnr_closest_points(const void* bvh, int64_t n_triangles, const double* points, int64_t n_points, double max_distance_sq,
                                  double* dist_sq, int32_t* primitive_ids, double* closest, double* primitive_uvs, int64_t* info_dev,
                                  void* stream) {
    CL_REQUIRE_COUNTS("lnr_closest_points", n_triangles, "triangles", n_points, "points");
    LNR_REQUIRE(!(max_distance_sq != max_distance_sq), "lnr_closest_points: max_distance_sq is NaN");
    LNR_REQUIRE(bvh && info_dev && (n_points == 0 || (points && dist_sq && primitive_ids)), "lnr_closest_points: null argument");
    const BvhLayout b = bvh_layout(n_triangles);
    const char* bb = (const char*)bvh;
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("closest_points", st);
    if (int rc = clear_words(info_dev, 8 * sizeof(int64_t), st, "lnr_closest_points", "info words")) return rc;
    if (n_points > 0)
        hipLaunchKernelGGL(closest_points_kernel, dim3((uint32_t)((n_points + RC_WAVE - 1) / RC_WAVE)), dim3(RC_WAVE), 0, st,
                           (const BvhHead*)(bb + b.head), (const BvhNode*)(bb + b.nodes), (const double*)(bb + b.leaf_v),
                           (const int32_t*)(bb + b.leaf_id), points, (uint32_t)n_points, max_distance_sq, dist_sq, primitive_ids, closest,
                           primitive_uvs, (unsigned long long*)(info_dev + 1));
    hipLaunchKernelGGL(cast_info, dim3(1), dim3(1), 0, st, (const BvhHead*)(bb + b.head), info_dev);
    LNR_CHECK_LAUNCH("lnr_closest_points");
    return LNR_OK;
}

extern "C" int lnr_count_intersections(const void* bvh, int64_t n_triangles, const double* rays, int64_t n_rays, double t_min, double t_max,
                                       int32_t* counts, int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNTS("lnr_count_intersections", n_triangles, "triangles", n_rays, "rays");
    LNR_REQUIRE(!(t_min != t_min) && !(t_max != t_max), "lnr_count_intersections: t_min or t_max is NaN");
    LNR_REQUIRE(bvh && info_dev && (n_rays == 0 || (rays && counts)), "lnr_count_intersections: null argument");
    const BvhLayout b = bvh_layout(n_triangles);
    const char* bb = (const char*)bvh;
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("count_intersections", st);
    if (int rc = clear_words(info_dev, 8 * sizeof(int64_t), st, "lnr_count_intersections", "info words")) return rc;
    if (n_rays > 0)
        hipLaunchKernelGGL(count_intersections_kernel, dim3((uint32_t)((n_rays + RC_WAVE - 1) / RC_WAVE)), dim3(RC_WAVE), 0, st,
                           (const BvhHead*)(bb + b.head), (const BvhNode*)(bb + b.nodes), (const double*)(bb + b.leaf_v), rays,
                           (uint32_t)n_rays, t_min, t_max, counts, (unsigned long long*)(info_dev + 1));
    hipLaunchKernelGGL(cast_info, dim3(1), dim3(1), 0, st, (const BvhHead*)(bb + b.head), info_dev);
    LNR_CHECK_LAUNCH("lnr_count_intersections");
    return LNR_OK;
}

extern "C" int lnr_trajectory_rays(const float* directions, const double* timestamps, int64_t n_rays, const double* traj_times,
                                   const double* traj_positions, const double* traj_rotations, const double* traj_rotvecs, int64_t n_poses,
                                   double* rays, int64_t* info_dev, void* stream) {
    CL_REQUIRE_COUNT("lnr_trajectory_rays", n_rays, "rays");
    LNR_REQUIRE(n_poses >= 2 && n_poses <= INT32_MAX, "lnr_trajectory_rays: %lld poses, at least 2 are needed", (long long)n_poses);
    LNR_REQUIRE(info_dev && traj_times && traj_positions && traj_rotations && traj_rotvecs && (n_rays == 0 || (directions && timestamps && rays)),
                "lnr_trajectory_rays: null argument");
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("trajectory_rays", st);
    if (int rc = clear_words(info_dev, 8 * sizeof(int64_t), st, "lnr_trajectory_rays", "info words")) return rc;
    const TrajView tv{traj_times, traj_positions, traj_rotations, traj_rotvecs, (uint32_t)n_poses};
    if (n_rays > 0)
        hipLaunchKernelGGL(traj_rays, dim3(blocks_for((uint64_t)n_rays)), dim3(CL_BLOCK), 0, st, directions, timestamps, (uint32_t)n_rays, tv,
                           rays, (unsigned long long*)(info_dev + 1));
    hipLaunchKernelGGL(traj_rays_info, dim3(1), dim3(1), 0, st, info_dev);
    LNR_CHECK_LAUNCH("lnr_trajectory_rays");
    return LNR_OK;
}
