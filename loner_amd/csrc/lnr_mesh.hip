// The mesher (gfx950): the weight volume, accumulated in the compositing kernel, and marching cubes over it.
//
// This file is compiled without SLP vectorisation (build.py).  render_mesh_accumulate_kernel composites with the same render_ray as
// lnr_render_forward (lnr_render_ray.h), and the contraction of a multiply-add into an fma (-ffp-contract=fast) depends on the code
// around it: with the SLP vectoriser on, some of render_ray's multiplies became packed v_pk_mul_f32 here, their adds stayed separate,
// and weights came out an ulp away from lnr_render_forward's.  Without it every multiply-add contracts as in render_forward_kernel, and
// the fused kernel's weights are lnr_render_forward's bit for bit (tests/test_gpu_mesh.py).
//
// Replaces  skimage.measure.marching_cubes   as called by analysis/mesher.py:183-207
// with a definition of our own (include/loner_hip.h, "meshing"): inside is v > level, one vertex per crossing lattice edge owned by
// the edge's lower node, and a case table generated here from a single face rule instead of the Lorensen-Cline / Lewiner tables.
//
// Three passes, each one thread per node (a cell is named by its lower node):
//   count      per block: vertices (sign changes on the node's +x/+y/+z edges) and triangles (the case's count) -> block sums
//   scan       one workgroup: exclusive scan of the block sums (uint64) and the two totals, which the host reads once
//   vertices   per block again: each node's first vertex id (block offset + in-block prefix) and its vertex positions; the id is
//              stored with the node's x- and y-edge bits (what a neighbour needs to find the id of any of the node's vertices)
//   triangles  per block again: the cell's case, its triangle slots, and for each triangle corner the id of the vertex on that edge
// Ids and slots come from prefix sums in node order, so the output is the same on every run.  A wave owns 1024 consecutive nodes
// (16 per lane, lane-fastest: coalesced loads); its in-wave prefix of the small per-node counts is a handful of ballots.
#include "lnr_common.h"
#include "lnr_render_ray.h"

#define MC_BLOCK 256
#define MC_PER_LANE 16
#define MC_WAVE_NODES (64 * MC_PER_LANE)
#define MC_BLOCK_NODES ((MC_BLOCK / 64) * MC_WAVE_NODES)
#define MC_SCAN_BLOCK 1024
#define MC_W LNR_MC_TABLE_WIDTH

__constant__ int8_t c_mc_table[256 * MC_W];
__constant__ uint8_t c_mc_ntri[256];

// ------------------------------------------------------------------------------------------------ case table (host)
// Corner c sits at (c & 1, c >> 1 & 1, c >> 2 & 1).  Edge e = 4 a + q runs along axis a from the q-th corner (in corner order) whose
// bit a is clear.  Per case: on every cube face, the crossing edges of the face are joined by segments - one when two edges cross,
// and when all four do (the two inside corners diagonal) one segment around each inside corner: they are separated.  The rule reads
// the face's four corners only, so the cell on the other side of the face draws the same segments.  Each segment is directed with
// the inside on its left seen from outside the cube; the segments then chain into closed loops (every crossing edge lies on two
// faces), and each loop is fanned into triangles (a, c, b) - reversed, so that they face the outside (lower values).  The fan's apex
// is the loop rotation whose worst triangle, taken at the edge midpoints, faces the outside best (the first such rotation): a plain
// fan from the first edge can make triangles of three collinear midpoints.
namespace {

struct V3 { double x, y, z; };
V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 corner_pos(int c) { return {(double)(c & 1), (double)(c >> 1 & 1), (double)(c >> 2 & 1)}; }

void edge_corners(int e, int* c0, int* c1) {
    const int a = e >> 2, q = e & 3;
    const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;
    *c0 = ((q & 1) << o0) | (((q >> 1) & 1) << o1);
    *c1 = *c0 | (1 << a);
}
int edge_of(int c0, int c1) {
    const int d = c0 ^ c1, a = d == 1 ? 0 : (d == 2 ? 1 : 2), c = c0 < c1 ? c0 : c1;
    const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;
    return 4 * a + (((c >> o0) & 1) | (((c >> o1) & 1) << 1));
}
V3 edge_mid(int e) {
    int c0, c1;
    edge_corners(e, &c0, &c1);
    const V3 p = corner_pos(c0), r = corner_pos(c1);
    return {(p.x + r.x) / 2, (p.y + r.y) / 2, (p.z + r.z) / 2};
}
// sum over the triangle's corners of (normal . inside->outside direction of the corner's edge): > 0 when it faces the outside
double facing(const int t[3], int cas) {
    const V3 p0 = edge_mid(t[0]), p1 = edge_mid(t[1]), p2 = edge_mid(t[2]);
    const V3 n = cross(p1 - p0, p2 - p0);
    double s = 0.0;
    for (int m = 0; m < 3; ++m) {
        int c0, c1;
        edge_corners(t[m], &c0, &c1);
        const V3 d = corner_pos(c1) - corner_pos(c0);
        s += ((cas >> c1) & 1) ? -dot(n, d) : dot(n, d);
    }
    return s;
}

struct McTable {
    int8_t t[256][MC_W];
    uint8_t ntri[256];
    McTable() {
        for (int cas = 0; cas < 256; ++cas) {
            auto in = [&](int c) { return (cas >> c) & 1; };
            int next[12];
            for (int e = 0; e < 12; ++e) next[e] = -1;
            for (int a = 0; a < 3; ++a) {
                const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
                for (int s = 0; s < 2; ++s) {
                    V3 n = {0, 0, 0};
                    (a == 0 ? n.x : a == 1 ? n.y : n.z) = 2.0 * s - 1.0;
                    int cyc[4];
                    const int uv[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
                    for (int i = 0; i < 4; ++i) cyc[i] = (s << a) | (uv[i][0] << b) | (uv[i][1] << c);
                    int cross_at[4], nc = 0;                      // face edge i joins cyc[i] and cyc[i + 1]
                    for (int i = 0; i < 4; ++i) if (in(cyc[i]) != in(cyc[(i + 1) & 3])) cross_at[nc++] = i;
                    int segs[2][3], ns = 0;                       // {edge, edge, an inside corner on its side}
                    if (nc == 2) {
                        int pin = -1;
                        for (int i = 0; i < 4 && pin < 0; ++i) if (in(cyc[i])) pin = cyc[i];
                        segs[ns][0] = edge_of(cyc[cross_at[0]], cyc[(cross_at[0] + 1) & 3]);
                        segs[ns][1] = edge_of(cyc[cross_at[1]], cyc[(cross_at[1] + 1) & 3]);
                        segs[ns++][2] = pin;
                    } else if (nc == 4) {
                        for (int i = 0; i < 4; ++i) {
                            if (!in(cyc[i])) continue;
                            segs[ns][0] = edge_of(cyc[(i + 3) & 3], cyc[i]);
                            segs[ns][1] = edge_of(cyc[i], cyc[(i + 1) & 3]);
                            segs[ns++][2] = cyc[i];
                        }
                    }
                    for (int k = 0; k < ns; ++k) {
                        int e1 = segs[k][0], e2 = segs[k][1];
                        const V3 m1 = edge_mid(e1), m2 = edge_mid(e2);
                        if (dot(n, cross(m2 - m1, corner_pos(segs[k][2]) - m1)) < 0) { const int x = e1; e1 = e2; e2 = x; }
                        next[e1] = e2;
                    }
                }
            }
            int ntri = 0;
            bool seen[12] = {};
            for (int e = 0; e < 12; ++e) {
                if (next[e] < 0 || seen[e]) continue;
                int loop[12], len = 0;
                for (int x = e; !seen[x]; x = next[x]) { seen[x] = true; loop[len++] = x; }
                int best_r = 0;
                double best = -1e300;
                for (int r = 0; r < len; ++r) {
                    double worst = 1e300;
                    for (int i = 1; i + 1 < len; ++i) {
                        const int tri[3] = {loop[r], loop[(r + i + 1) % len], loop[(r + i) % len]};
                        const double f = facing(tri, cas);
                        worst = f < worst ? f : worst;
                    }
                    if (worst > best) { best = worst; best_r = r; }
                }
                for (int i = 1; i + 1 < len; ++i) {
                    t[cas][3 * ntri] = (int8_t)loop[best_r];
                    t[cas][3 * ntri + 1] = (int8_t)loop[(best_r + i + 1) % len];
                    t[cas][3 * ntri + 2] = (int8_t)loop[(best_r + i) % len];
                    ++ntri;
                }
            }
            ntri_ok = ntri_ok && 3 * ntri < MC_W;
            for (int k = 3 * ntri; k < MC_W; ++k) t[cas][k] = -1;
            this->ntri[cas] = (uint8_t)ntri;
        }
    }
    bool ntri_ok = true;
};

const McTable& mc_table() {
    static const McTable tab;
    return tab;
}

}  // namespace

extern "C" int lnr_mc_case_table(int8_t* out) {
    LNR_REQUIRE(out != nullptr, "lnr_mc_case_table: null argument");
    const McTable& tab = mc_table();
    LNR_REQUIRE(tab.ntri_ok, "lnr_mc_case_table: a case needs more than %d triangles", (MC_W - 1) / 3);
    memcpy(out, tab.t, sizeof(tab.t));
    return LNR_OK;
}

// ------------------------------------------------------------------------------------------------ device
struct McDims {
    uint32_t nx, ny, nz, nyz, n;
};

__device__ __forceinline__ void mc_ijk(uint32_t node, const McDims& d, uint32_t& i, uint32_t& j, uint32_t& k) {
    i = node / d.nyz;
    const uint32_t r = node - i * d.nyz;
    j = r / d.nz;
    k = r - j * d.nz;
}

// bits 0..2: the node's +x / +y / +z edge crosses the level.  MASKED (lnr_mc_*_masked): and both its ends are valid
template <bool MASKED>
__device__ __forceinline__ uint32_t mc_edge_bits(const float* __restrict__ v, const uint8_t* __restrict__ valid, uint32_t node, uint32_t i,
                                                 uint32_t j, uint32_t k, const McDims& d, float level) {
    if (MASKED && !valid[node]) return 0;
    const bool a = v[node] > level;
    uint32_t bits = 0;
    if (i + 1 < d.nx && (!MASKED || valid[node + d.nyz]) && (v[node + d.nyz] > level) != a) bits |= 1u;
    if (j + 1 < d.ny && (!MASKED || valid[node + d.nz]) && (v[node + d.nz] > level) != a) bits |= 2u;
    if (k + 1 < d.nz && (!MASKED || valid[node + 1]) && (v[node + 1] > level) != a) bits |= 4u;
    return bits;
}

// the case of the cell whose lower node this is (0 for nodes on the upper faces: they name no cell).  MASKED: 0 as well for a cell
// with a corner that is not valid
template <bool MASKED>
__device__ __forceinline__ uint32_t mc_case(const float* __restrict__ v, const uint8_t* __restrict__ valid, uint32_t node, uint32_t i,
                                            uint32_t j, uint32_t k, const McDims& d, float level) {
    if (i + 1 >= d.nx || j + 1 >= d.ny || k + 1 >= d.nz) return 0;
    uint32_t cas = 0;
    bool all_valid = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t off = ((c & 1) ? d.nyz : 0u) + ((c & 2) ? d.nz : 0u) + ((c & 4) ? 1u : 0u);
        cas |= (v[node + off] > level ? 1u : 0u) << c;
        if (MASKED) all_valid = all_valid && valid[node + off];
    }
    return all_valid ? cas : 0;
}

__device__ __forceinline__ uint32_t popc64(uint64_t m) { return (uint32_t)__popcll(m); }

// in-wave exclusive prefix and wave total of a per-lane count < 8, from its three bits
__device__ __forceinline__ uint32_t mc_wave_prefix(uint32_t cnt, uint64_t lt_mask, uint32_t* total) {
    const uint64_t b0 = __ballot(cnt & 1u), b1 = __ballot(cnt & 2u), b2 = __ballot(cnt & 4u);
    *total = popc64(b0) + 2u * popc64(b1) + 4u * popc64(b2);
    return popc64(b0 & lt_mask) + 2u * popc64(b1 & lt_mask) + 4u * popc64(b2 & lt_mask);
}

template <bool MASKED>
__global__ void __launch_bounds__(MC_BLOCK)
mc_count_kernel(const float* __restrict__ v, const uint8_t* __restrict__ valid, const McDims d, float level,
                uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t part[MC_BLOCK / 64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * MC_BLOCK_NODES + wave * MC_WAVE_NODES;
    uint32_t nv = 0, nt = 0;
#pragma unroll 4
    for (int it = 0; it < MC_PER_LANE; ++it) {
        const uint32_t node = base + it * 64 + lane;
        if (node < d.n) {
            uint32_t i, j, k;
            mc_ijk(node, d, i, j, k);
            nv += __popc(mc_edge_bits<MASKED>(v, valid, node, i, j, k, d, level));
            nt += c_mc_ntri[mc_case<MASKED>(v, valid, node, i, j, k, d, level)];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nv += __shfl_xor(nv, o, 64); nt += __shfl_xor(nt, o, 64); }
    if (lane == 0) { part[wave][0] = nv; part[wave][1] = nt; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t s = 0;
        for (int w = 0; w < MC_BLOCK / 64; ++w) s += part[w][threadIdx.x];
        block_counts[2 * blockIdx.x + threadIdx.x] = s;
    }
}

// exclusive scan of the block counts (two interleaved columns) in one workgroup, chunk after chunk with a running carry
__global__ void __launch_bounds__(MC_SCAN_BLOCK)
mc_scan_kernel(const uint32_t* __restrict__ block_counts, int n_blocks, uint64_t* __restrict__ block_offsets,
               unsigned long long* __restrict__ totals) {
    __shared__ uint64_t wsum[MC_SCAN_BLOCK / 64][2];
    __shared__ uint64_t carry[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 2) carry[threadIdx.x] = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n_blocks; c0 += MC_SCAN_BLOCK) {
        const int b = c0 + threadIdx.x;
        unsigned long long x[2], inc[2];
        x[0] = b < n_blocks ? block_counts[2 * b] : 0;
        x[1] = b < n_blocks ? block_counts[2 * b + 1] : 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            inc[q] = x[q];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long t = __shfl_up(inc[q], o, 64);
                if (lane >= o) inc[q] += t;
            }
            if (lane == 63) wsum[wave][q] = inc[q];
        }
        __syncthreads();
        if (threadIdx.x < 2) {                                  // wave totals -> exclusive wave offsets (+ carry)
            uint64_t s = carry[threadIdx.x];
            for (int w = 0; w < MC_SCAN_BLOCK / 64; ++w) { const uint64_t t = wsum[w][threadIdx.x]; wsum[w][threadIdx.x] = s; s += t; }
            carry[threadIdx.x] = s;
        }
        __syncthreads();
        if (b < n_blocks) {
            block_offsets[2 * b] = wsum[wave][0] + inc[0] - x[0];
            block_offsets[2 * b + 1] = wsum[wave][1] + inc[1] - x[1];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) totals[threadIdx.x] = carry[threadIdx.x];
}

// the first vertex id of the node in bits 2.., its x- and y-edge bits in bits 0 and 1: the id of its vertex on axis a is
// (w >> 2) + the number of its crossing edges on the axes before a
template <bool MASKED>
__global__ void __launch_bounds__(MC_BLOCK)
mc_vertex_kernel(const float* __restrict__ v, const uint8_t* __restrict__ valid, const McDims d, float level,
                 const uint64_t* __restrict__ block_offsets,
                 float sx, float sy, float sz, float ox, float oy, float oz, uint32_t* __restrict__ packed, float* __restrict__ verts,
                 uint64_t n_verts) {
    __shared__ uint32_t wtot[MC_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lt = (1ull << lane) - 1ull;
    const uint32_t base = blockIdx.x * MC_BLOCK_NODES + wave * MC_WAVE_NODES;
    uint64_t bits_all = 0;                                       // 3 bits per node of the lane, 16 nodes
    uint32_t total = 0;
#pragma unroll
    for (int it = 0; it < MC_PER_LANE; ++it) {
        const uint32_t node = base + it * 64 + lane;
        uint32_t bits = 0;
        if (node < d.n) {
            uint32_t i, j, k;
            mc_ijk(node, d, i, j, k);
            bits = mc_edge_bits<MASKED>(v, valid, node, i, j, k, d, level);
        }
        bits_all |= (uint64_t)bits << (3 * it);
        uint32_t t;
        mc_wave_prefix(__popc(bits), lt, &t);
        total += t;
    }
    if (lane == 0) wtot[wave] = total;
    __syncthreads();
    uint64_t off = block_offsets[2 * blockIdx.x];
    for (int w = 0; w < wave; ++w) off += wtot[w];
    const float sp[3] = {sx, sy, sz}, org[3] = {ox, oy, oz};
#pragma unroll
    for (int it = 0; it < MC_PER_LANE; ++it) {
        const uint32_t node = base + it * 64 + lane;
        const uint32_t bits = (uint32_t)(bits_all >> (3 * it)) & 7u;
        uint32_t t;
        const uint32_t pre = mc_wave_prefix(__popc(bits), lt, &t);
        if (bits && off + pre + __popc(bits) <= n_verts) {           // (always: the count pass saw the same bits)
            const uint32_t id0 = (uint32_t)off + pre;
            packed[node] = (id0 << 2) | (bits & 3u);
            uint32_t ijk[3];
            mc_ijk(node, d, ijk[0], ijk[1], ijk[2]);
            const float va = v[node];
            const uint32_t stride[3] = {d.nyz, d.nz, 1u};
            uint32_t id = id0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!((bits >> a) & 1u)) continue;
                const float vb = v[node + stride[a]];
                const float tt = __fdiv_rn(level - va, vb - va);
                float* o = verts + 3 * (size_t)id;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float f = q == a ? lnr_add_rn((float)ijk[q], tt) : (float)ijk[q];
                    o[q] = lnr_add_rn(lnr_mul_rn(f, sp[q]), org[q]);
                }
                ++id;
            }
        }
        off += t;
    }
}

template <bool MASKED>
__global__ void __launch_bounds__(MC_BLOCK)
mc_triangle_kernel(const float* __restrict__ v, const uint8_t* __restrict__ valid, const McDims d, float level,
                   const uint64_t* __restrict__ block_offsets,
                   const uint32_t* __restrict__ packed, int32_t* __restrict__ tris, uint64_t n_tris) {
    __shared__ uint32_t wtot[MC_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lt = (1ull << lane) - 1ull;
    const uint32_t base = blockIdx.x * MC_BLOCK_NODES + wave * MC_WAVE_NODES;
    uint32_t cases[MC_PER_LANE];
    uint32_t total = 0;
#pragma unroll
    for (int it = 0; it < MC_PER_LANE; ++it) {
        const uint32_t node = base + it * 64 + lane;
        uint32_t cas = 0;
        if (node < d.n) {
            uint32_t i, j, k;
            mc_ijk(node, d, i, j, k);
            cas = mc_case<MASKED>(v, valid, node, i, j, k, d, level);
        }
        cases[it] = cas;
        uint32_t t;
        mc_wave_prefix(c_mc_ntri[cas], lt, &t);
        total += t;
    }
    if (lane == 0) wtot[wave] = total;
    __syncthreads();
    uint64_t off = block_offsets[2 * blockIdx.x + 1];
    for (int w = 0; w < wave; ++w) off += wtot[w];
#pragma unroll
    for (int it = 0; it < MC_PER_LANE; ++it) {
        const uint32_t node = base + it * 64 + lane;
        const uint32_t cas = cases[it];
        const uint32_t nt = c_mc_ntri[cas];
        uint32_t t;
        const uint32_t pre = mc_wave_prefix(nt, lt, &t);
        for (uint32_t q = 0; q < nt && off + pre + q < n_tris; ++q) {     // (always: the count pass saw the same cases)
            int32_t* o = tris + 3 * (size_t)(off + pre + q);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int e = c_mc_table[cas * MC_W + 3 * q + m];
                const int a = e >> 2, qq = e & 3;
                const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;
                const int c = ((qq & 1) << o0) | (((qq >> 1) & 1) << o1);
                const uint32_t owner = node + ((c & 1) ? d.nyz : 0u) + ((c & 2) ? d.nz : 0u) + ((c & 4) ? 1u : 0u);
                const uint32_t w = packed[owner];
                o[m] = (int32_t)((w >> 2) + (a >= 1 ? (w & 1u) : 0u) + (a == 2 ? ((w >> 1) & 1u) : 0u));
            }
        }
        off += t;
    }
}

// ------------------------------------------------------------------------------------------------
// Weight volume of the mesher (analysis/mesher.py:143-180): render_ray's weights go straight into a scatter-max over the lattice.
// The reference materialises points and weights [N,S] per 512-ray chunk and runs ~10 torch ops on them; here a sample's weight
// never leaves its register.  Atomics are the cost (one per sample would be ~6 ms per scan at the measured 21 G/s), so three
// filters that cannot change the result come first: w > 0 only, a lane's run of consecutive samples in one voxel is merged into
// its max, and a voxel that already holds at least the weight (the volume only grows) is not touched.
// ------------------------------------------------------------------------------------------------
// torch.bucketize(x, axis) of an fp32 point against an fp64 axis: the smallest i with (double) x <= axis[i] (n when there is none).
// The guess from the axis' first node and spacing is corrected against the axis values, so the result does not depend on it.
__device__ __forceinline__ int mesh_bucket(float xf, const double* __restrict__ axis, int n, double first, double inv_step) {
    const double x = (double)xf;
    const double g = ceil((x - first) * inv_step);
    int i = g <= 0.0 ? 0 : (g >= (double)n ? n : (int)g);
    while (i > 0 && x <= axis[i - 1]) --i;
    while (i < n && x > axis[i]) ++i;
    return i;
}

template <int C>
__global__ void __launch_bounds__(RENDER_BLOCK)
render_mesh_accumulate_kernel(const float* __restrict__ sigma, const float* __restrict__ z, const float* __restrict__ rays, int n_rays,
                              const int32_t* __restrict__ n_rays_dev, int S, const float* __restrict__ noise, float noise_std,
                              uint64_t seed, const LnrMeshGrid g, float depth_max, int use_var, float var_max,
                              uint32_t* __restrict__ volume, unsigned long long* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= lnr_live_rays(n_rays, n_rays_dev)) return;
    const float* rr = rays + (size_t)ray * LNR_RAY_STRIDE;
    RayState<C> st;
    extern __shared__ __attribute__((aligned(16))) float mesh_stage[];
    float* stage = C >= 16 ? mesh_stage + (threadIdx.x >> 6) * 64 * (C + 4) : nullptr;
    render_ray<C>(st, sigma, z, noise, noise_std, seed, ray, S, lane, rr, stage);
    // (depth and variance are wave sums over an xor butterfly: every lane holds the same bits, the test is wave-uniform)
    if (!(st.depth < depth_max) || (use_var && !(st.variance < var_max))) return;
    const float ox = rr[0], oy = rr[1], oz = rr[2], dx = rr[3], dy = rr[4], dz = rr[5];
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
    const int64_t n_nodes = (int64_t)nx * ny * nz;
    int64_t cur = -1;
    uint32_t cur_w = 0;
    uint32_t n_in = 0, n_atomic = 0;
    auto flush = [&]() {
        if (cur >= 0) {
            // a stale read only lets an atomic through; the volume never shrinks, so a skipped update was never needed
            if (cur_w > volume[cur]) { atomicMax(volume + cur, cur_w); ++n_atomic; }
        }
    };
#pragma unroll
    for (int t = 0; t < C; ++t) {
        const float w = st.w[t];
        if (lane * C + t < S && w > 0.0f) {
            const float zt = st.z[t];
            const float px = lnr_add_rn(ox, lnr_mul_rn(dx, zt));          // rays_o + rays_d * z, two roundings (rendering_tcnn.py:241)
            const float py = lnr_add_rn(oy, lnr_mul_rn(dy, zt));
            const float pz = lnr_add_rn(oz, lnr_mul_rn(dz, zt));
            if (px >= g.lo[0] && px <= g.hi[0] && py >= g.lo[1] && py <= g.hi[1] && pz >= g.lo[2] && pz <= g.hi[2]) {
                const int xb = mesh_bucket(px, g.axis[0], nx, g.first[0], g.inv_step[0]);
                const int yb = mesh_bucket(py, g.axis[1], ny, g.first[1], g.inv_step[1]);
                const int zb = mesh_bucket(pz, g.axis[2], nz, g.first[2], g.inv_step[2]);
                const int64_t idx = (int64_t)xb * nz + (int64_t)yb * nx * nz + zb;       // mesher.py:173, incl. its row aliasing
                if (idx < n_nodes) {                                                     // mesher.py:176
                    ++n_in;
                    const uint32_t wb = __float_as_uint(w);
                    if (idx == cur) {
                        cur_w = wb > cur_w ? wb : cur_w;
                    } else {
                        flush();
                        cur = idx;
                        cur_w = wb;
                    }
                }
            }
        }
    }
    flush();
    if (counters != nullptr) {
        unsigned long long a = n_in, b = n_atomic;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
        if (lane == 0) { atomicAdd(counters, a); atomicAdd(counters + 1, b); }
    }
}

extern "C" int lnr_render_mesh_accumulate(const float* sigma, const float* z, const float* rays, int32_t n_rays, const int32_t* n_rays_dev,
                                          int32_t n_samples, const float* noise, float noise_std, uint64_t seed, const LnrMeshGrid* grid,
                                          float depth_max, int32_t use_var, float var_max, float* volume, uint64_t* counters, void* stream) {
    LNR_REQUIRE(sigma && z && rays && grid && volume && n_rays >= 0 && n_samples >= 2, "lnr_render_mesh_accumulate: bad argument");
    for (int a = 0; a < 3; ++a)
        LNR_REQUIRE(grid->n[a] >= 1 && grid->axis[a] != nullptr, "lnr_render_mesh_accumulate: axis %d is empty", a);
    LNR_REQUIRE((int64_t)grid->n[0] * grid->n[1] * grid->n[2] < ((int64_t)1 << 31), "lnr_render_mesh_accumulate: 2^31 nodes or more");
    if (n_rays == 0) return LNR_OK;
    const dim3 grd(lnr_div_up(n_rays, RAYS_PER_BLOCK)), block(RENDER_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    LnrProfScope prof("render_mesh_accumulate", st);
    DISPATCH_C(n_samples, hipLaunchKernelGGL(render_mesh_accumulate_kernel<C>, grd, block, C >= 16 ? RAYS_PER_BLOCK * 64 * (C + 4) * sizeof(float) : 0,
                                             st, sigma, z, rays, n_rays, n_rays_dev, n_samples, noise, noise_std, seed, *grid, depth_max,
                                             use_var, var_max, reinterpret_cast<uint32_t*>(volume),
                                             reinterpret_cast<unsigned long long*>(counters)));
    LNR_CHECK_LAUNCH("lnr_render_mesh_accumulate");
    return LNR_OK;
}

// ------------------------------------------------------------------------------------------------ host
namespace {
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
struct McLayout {
    int n_blocks;
    size_t counts, offsets, packed, total;
};
McLayout mc_layout(int64_t n) {
    McLayout l;
    l.n_blocks = (int)((n + MC_BLOCK_NODES - 1) / MC_BLOCK_NODES);
    l.counts = 0;
    l.offsets = align256(l.counts + 2 * sizeof(uint32_t) * (size_t)l.n_blocks);
    l.packed = align256(l.offsets + 2 * sizeof(uint64_t) * (size_t)l.n_blocks);
    l.total = align256(l.packed + sizeof(uint32_t) * (size_t)n);
    return l;
}
int mc_check_dims(int32_t nx, int32_t ny, int32_t nz, const char* what) {
    LNR_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: every axis needs at least two nodes (%d x %d x %d)", what, nx, ny, nz);
    LNR_REQUIRE((int64_t)nx * ny * nz < ((int64_t)1 << 31), "%s: %lld nodes, the limit is 2^31 - 1", what, (long long)nx * ny * nz);
    return LNR_OK;
}
McDims mc_dims(int32_t nx, int32_t ny, int32_t nz) {
    McDims d;
    d.nx = (uint32_t)nx; d.ny = (uint32_t)ny; d.nz = (uint32_t)nz;
    d.nyz = d.ny * d.nz;
    d.n = d.nx * d.nyz;
    return d;
}
}  // namespace

extern "C" size_t lnr_mc_workspace(int32_t nx, int32_t ny, int32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    return mc_layout((int64_t)nx * ny * nz).total;
}

namespace {
template <bool MASKED>
int mc_count_impl(const char* fn, const float* volume, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz, float level, void* workspace,
                  size_t workspace_bytes, uint64_t* totals_dev, void* stream) {
    if (int rc = mc_check_dims(nx, ny, nz, fn)) return rc;
    LNR_REQUIRE(volume && workspace && totals_dev && (!MASKED || valid), "%s: null argument", fn);
    const McLayout l = mc_layout((int64_t)nx * ny * nz);
    LNR_REQUIRE(workspace_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, l.total);
    const McTable& tab = mc_table();
    LNR_REQUIRE(tab.ntri_ok, "%s: case table overflow", fn);
    hipStream_t st = (hipStream_t)stream;
    // the table goes to constant memory of the current device with every call (4.3 KB, stream ordered: any device, any stream)
    if (hipMemcpyToSymbolAsync(HIP_SYMBOL(c_mc_table), tab.t, sizeof(tab.t), 0, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyToSymbolAsync(HIP_SYMBOL(c_mc_ntri), tab.ntri, sizeof(tab.ntri), 0, hipMemcpyHostToDevice, st) != hipSuccess) {
        lnr_set_error("%s: upload of the case table failed", fn);
        return LNR_ERR_LAUNCH;
    }
    char* ws = (char*)workspace;
    const McDims d = mc_dims(nx, ny, nz);
    {
        LnrProfScope prof("mc_count", st);
        hipLaunchKernelGGL(mc_count_kernel<MASKED>, dim3(l.n_blocks), dim3(MC_BLOCK), 0, st, volume, valid, d, level,
                           (uint32_t*)(ws + l.counts));
        LNR_CHECK_LAUNCH(fn);
    }
    {
        LnrProfScope prof("mc_scan", st);
        hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, (const uint32_t*)(ws + l.counts), l.n_blocks,
                           (uint64_t*)(ws + l.offsets), (unsigned long long*)totals_dev);
        LNR_CHECK_LAUNCH(fn);
    }
    return LNR_OK;
}

template <bool MASKED>
int mc_emit_impl(const char* fn, const float* volume, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz, float level,
                 const float* spacing, const float* origin, void* workspace, size_t workspace_bytes, int64_t n_verts, int64_t n_tris,
                 float* verts, int32_t* tris, void* stream) {
    if (int rc = mc_check_dims(nx, ny, nz, fn)) return rc;
    LNR_REQUIRE(volume && workspace && spacing && origin && (!MASKED || valid), "%s: null argument", fn);
    LNR_REQUIRE(n_verts >= 0 && n_verts < ((int64_t)1 << 30), "%s: %lld vertices, the limit is 2^30 - 1", fn, (long long)n_verts);
    // (masked: vertices whose cells all lost a corner come without a triangle)
    LNR_REQUIRE(n_tris >= 0 && (n_verts == 0 || (verts && (tris || (MASKED && n_tris == 0)))), "%s: bad outputs", fn);
    const McLayout l = mc_layout((int64_t)nx * ny * nz);
    LNR_REQUIRE(workspace_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, l.total);
    if (n_verts == 0) return LNR_OK;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const McDims d = mc_dims(nx, ny, nz);
    {
        LnrProfScope prof("mc_vertices", st);
        hipLaunchKernelGGL(mc_vertex_kernel<MASKED>, dim3(l.n_blocks), dim3(MC_BLOCK), 0, st, volume, valid, d, level,
                           (const uint64_t*)(ws + l.offsets), spacing[0], spacing[1], spacing[2], origin[0], origin[1], origin[2],
                           (uint32_t*)(ws + l.packed), verts, (uint64_t)n_verts);
        LNR_CHECK_LAUNCH(fn);
    }
    if (n_tris > 0) {
        LnrProfScope prof("mc_triangles", st);
        hipLaunchKernelGGL(mc_triangle_kernel<MASKED>, dim3(l.n_blocks), dim3(MC_BLOCK), 0, st, volume, valid, d, level,
                           (const uint64_t*)(ws + l.offsets), (const uint32_t*)(ws + l.packed), tris, (uint64_t)n_tris);
        LNR_CHECK_LAUNCH(fn);
    }
    return LNR_OK;
}
}  // namespace

extern "C" int lnr_mc_count(const float* volume, int32_t nx, int32_t ny, int32_t nz, float level, void* workspace, size_t workspace_bytes,
                            uint64_t* totals_dev, void* stream) {
    return mc_count_impl<false>("lnr_mc_count", volume, nullptr, nx, ny, nz, level, workspace, workspace_bytes, totals_dev, stream);
}

extern "C" int lnr_mc_emit(const float* volume, int32_t nx, int32_t ny, int32_t nz, float level, const float* spacing, const float* origin,
                           void* workspace, size_t workspace_bytes, int64_t n_verts, int64_t n_tris, float* verts, int32_t* tris, void* stream) {
    return mc_emit_impl<false>("lnr_mc_emit", volume, nullptr, nx, ny, nz, level, spacing, origin, workspace, workspace_bytes, n_verts, n_tris,
                               verts, tris, stream);
}

extern "C" int lnr_mc_count_masked(const float* volume, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz, float level,
                                   void* workspace, size_t workspace_bytes, uint64_t* totals_dev, void* stream) {
    return mc_count_impl<true>("lnr_mc_count_masked", volume, valid, nx, ny, nz, level, workspace, workspace_bytes, totals_dev, stream);
}

extern "C" int lnr_mc_emit_masked(const float* volume, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz, float level,
                                  const float* spacing, const float* origin, void* workspace, size_t workspace_bytes, int64_t n_verts,
                                  int64_t n_tris, float* verts, int32_t* tris, void* stream) {
    return mc_emit_impl<true>("lnr_mc_emit_masked", volume, valid, nx, ny, nz, level, spacing, origin, workspace, workspace_bytes, n_verts,
                              n_tris, verts, tris, stream);
}
