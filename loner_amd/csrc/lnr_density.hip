// Density network: host-side dispatch (C ABI) of the level-major pipeline
//   forward : encode (level-major, lnr_encode.hip) -> feature planes -> MLP (fp32 MFMA, lnr_density_impl.h)
//   backward: [encode] -> MLP backward (weight-gradient slabs + d_feature planes) -> encode backward (table-gradient
//             records + d/dx planes) -> table_grad_reduce2 (per-owner LDS reduction) -> slab reduce (both: lnr_table_reduce.hip)
// plus the MFMA layout self-test.
#include "lnr_density_api.h"
#include <vector>
#include <cstdio>
#include <mutex>
#include <unordered_map>

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// Host-side note per workspace (keyed by its address): which layout last used it, whether the 64-bit overflow accumulators of that layout
// are known to be all-zero, and the call counter ("epoch") the kernels stamp a level's status word with when they add to its accumulators.
// The accumulators are zeroed once per layout change instead of once per backward (59 MB at the default size), and the reduce reads and
// re-zeroes only the levels that were stamped in THIS call (table_grad_reduce2_kernel).  What breaks the note - another network or batch
// size on the same workspace (its planes and regions lie elsewhere), lnr_density_workspace_init, an error between the first and the last
// launch of a backward - marks the accumulators unknown, and the next backward clears them.  The caller's side of the contract
// (include/loner_hip.h): between two density calls the workspace belongs to the library.
// ------------------------------------------------------------------------------------------------
namespace {
struct WsNote { uint64_t layout; uint32_t epoch; bool ovf_zero; };
std::mutex g_ws_mutex;
std::unordered_map<const void*, WsNote> g_ws_notes;

uint64_t layout_signature(const LnrNetSpec* spec, int64_t cap) {
    uint64_t h = 1469598103934665603ull;                        // FNV-1a over the spec and the point capacity
    auto mix = [&](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
    mix(spec, sizeof(LnrNetSpec));
    mix(&cap, sizeof(cap));
    return h;
}
// a density call with this layout touches the workspace: a different layout than the note's leaves the accumulators unknown
// (bounded: a caller that never releases its workspaces cannot grow the map without limit - dropping every note is always safe, the
// next backward on each workspace then clears its accumulators once)
void ws_bound_locked() { if (g_ws_notes.size() > 64) g_ws_notes.clear(); }
void ws_touch(const void* ws, uint64_t layout) {
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    ws_bound_locked();
    auto it = g_ws_notes.find(ws);
    if (it == g_ws_notes.end()) g_ws_notes[ws] = WsNote{layout, 0u, false};
    else if (it->second.layout != layout) { it->second.layout = layout; it->second.ovf_zero = false; }
}
// start of a backward that writes table gradients: -> {epoch of this call, must the accumulators be cleared first}; they count as unknown
// until ws_backward_done
void ws_backward_begin(const void* ws, uint64_t layout, int* epoch, bool* clear) {
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    ws_bound_locked();
    WsNote& n = g_ws_notes[ws];
    if (n.layout != layout) { n.layout = layout; n.ovf_zero = false; }
    *clear = !n.ovf_zero;
    n.ovf_zero = false;
    n.epoch = n.epoch >= 0x7FFFFFF0u ? 1u : n.epoch + 1u;
    if (n.epoch == 1u) *clear = true;                          // (first call, or the counter wrapped: stale stamps must go too)
    *epoch = (int)n.epoch;
}
void ws_backward_done(const void* ws) {
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    auto it = g_ws_notes.find(ws);
    if (it != g_ws_notes.end()) it->second.ovf_zero = true;
}
void ws_forget(const void* ws) {
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    g_ws_notes.erase(ws);
}
}  // namespace

// ------------------------------------------------------------------------------------------------
// workspace layout: [feat enc_dim x m_pad][dfeat enc_dim x m_pad][dxl groups x 3 x m_pad][slabs][counts][regions]
// ------------------------------------------------------------------------------------------------
struct Layout {
    int64_t m_pad;
    int n_groups, bpg, maxo, shift, nown, n_split;
    RegionPlan plan;
    size_t off_status, off_feat, off_wide, off_dfeat, off_dxl, off_dpts, off_rayacc, off_slabs, off_ovf, off_counts, off_regions, total;
};

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Region capacities (RegionPlan, lnr_density_api.h): level l sends n_points*8 corner updates (F/2 pair records each, 1 when
// F == 1; half as many x-pair records) to the `span` owners its table covers, from bpg workgroups.  Each level's regions hold
// that expectation + 25 % + 24 records; anything beyond it (skewed data) goes to the level's 64-bit overflow accumulators, so
// this is a performance knob only.
static Layout make_layout(const LnrNetSpec* spec, int64_t n_points, const DensityRoute& route) {
    Layout L;
    L.m_pad = (n_points + 63) / 64 * 64;
    if (L.m_pad < 64) L.m_pad = 64;
    // Plane skew: the MLP kernels read / write all 32 feature (d_feature) planes of the same samples at once, and the bench window's
    // planes are 2^21 samples = 8 MiB apart - a power-of-two stride puts the 32 concurrent streams on the same HBM channel / cache set
    // bits.  A plane stride that is a multiple of 64 KiB gets 17 x 256 bytes on top (LNR_PLANE_SKEW floats; 0 switches it off: A/B).
#ifndef LNR_PLANE_SKEW
#define LNR_PLANE_SKEW 1088
#endif
    if (LNR_PLANE_SKEW > 0 && (L.m_pad * (int64_t)sizeof(float)) % 65536 == 0) L.m_pad += LNR_PLANE_SKEW;
    const bool hash = spec->encoding == LNR_ENC_HASHGRID;
    L.n_groups = hash ? spec->n_levels : 1;
    L.shift = LNR_SLICE_SHIFT;
    const int64_t n_table = spec->n_params - spec->n_mlp_params;
    L.nown = (int)((n_table + (1 << L.shift) - 1) >> L.shift);
    int64_t bpg = (n_points + LNR_ENC_BWD_BLOCK * LNR_BATCHES_PER_WG - 1) / (LNR_ENC_BWD_BLOCK * LNR_BATCHES_PER_WG);   // batches per encode-backward workgroup
    if (bpg < 1) bpg = 1;
    if (bpg > LNR_ENC_MAX_BPG) bpg = LNR_ENC_MAX_BPG;
    bpg = (bpg + 3) & ~(int64_t)3;       // the wave-private partition runs 4 waves (= 4 chunks) per workgroup
    L.bpg = (int)bpg;
    L.maxo = 1;
    size_t ovf_total = 0;
    uint64_t region_total = 0;
    for (int l = 0; l < LNR_MAX_LEVELS; ++l) { L.plan.off[l] = 0; L.plan.bytes[l] = 0; L.plan.xp[l] = 0; L.plan.split[l] = 1; }
    L.n_split = 0;
    if (hash) {
        const int F = spec->n_features;
        for (int pass = 0; pass < 2; ++pass) {                              // pass 1 only if the plan exceeds the budget: scaled down
            if (pass == 1 && region_total <= LNR_REGION_BUDGET) break;
            const double shrink = pass == 0 ? 1.0 : (double)LNR_REGION_BUDGET / (double)region_total;
            region_total = 0; ovf_total = 0; L.maxo = 1; L.n_split = 0;
            for (int l = 0; l < spec->n_levels; ++l) {
                ovf_total += (size_t)spec->level_size[l] * F;
                const int span = lnr_level_span(spec, l, L.shift);
                if (span > L.maxo) L.maxo = span;
                // expected records per (owner, chunk): 8 corner updates per point (F/2 pair records each), spread over the level's owners
                const bool xp = lnr_level_can_use_xpairs(*spec, l, LNR_XPAIR_SCALE_MIN);
                L.plan.xp[l] = xp ? 1 : 0;
                double r = (double)n_points * 8.0 * (F >= 2 ? F / 2.0 : 1.0) / (double)span / (double)L.bpg;
                if (xp) r *= 0.5;                                           // one record per x-neighbour pair
                else if (spec->level_scale[l] < LNR_COMBINE_SCALE_MAX) r *= LNR_COMBINE_FILL;   // run-length combined along the rays
                // twice the expectation + 64 records, in 256-byte units: a record beyond the capacity costs four (two) 64-bit global atomics,
                // so the capacity is generous (sweep in DESIGN.md 2; the reduce does not care how full a region is)
                const double recs = (r * (xp ? LNR_REGION_HEADROOM_XP : LNR_REGION_HEADROOM) + LNR_REGION_SLACK) * shrink;
                uint64_t bytes = (uint64_t)(recs * (xp ? 12.0 : 8.0));
                bytes = (bytes + 255u) & ~(uint64_t)255u;
                // spatially coherent (dense-indexed) levels: several reduce workgroups per owner (table_grad_reduce_split_kernel)
                int parts = spec->level_hashed[l] == 0 ? LNR_REDUCE_SPLIT : 1;
                while (parts > 1 && L.bpg / parts < 16) parts >>= 1;      // at least one region per wave
                L.plan.split[l] = (uint8_t)(parts < 1 ? 1 : parts);
                if (parts > 1) L.n_split += span * parts;
                L.plan.off[l] = region_total;
                L.plan.bytes[l] = (uint32_t)bytes;
                region_total += (uint64_t)span * (uint64_t)L.bpg * bytes;
            }
        }
    }
    const int64_t blocks = (int64_t)L.n_groups * L.bpg;
    size_t off = 0;
    L.off_status = off; off += LNR_WORKSPACE_STATUS_BYTES;          // status words (include/loner_hip.h), same place for every n_points
    // (fp16 mode + frequency encoding: the MLP kernels evaluate the encoding and its input gradient themselves - no planes at all)
    const size_t plane_set = route.fused_enc ? 0 : (size_t)spec->enc_dim * L.m_pad * sizeof(float);
    L.off_feat = off; off += align256(plane_set);
    L.off_wide = off; off += align256(route.wide_bytes);     // chunk planes of the 256 x 2..3 route (0 bytes for every other network); the forward uses them too
    L.off_dfeat = off; off += align256(plane_set);
    L.off_dxl = off; off += align256(plane_set == 0 ? 0 : (size_t)L.n_groups * 3 * L.m_pad * sizeof(float));
    L.off_dpts = off; off += align256((size_t)3 * L.m_pad * sizeof(float));      // d_pts scratch of the general d_rays route
    L.off_rayacc = off; off += align256(((size_t)(L.m_pad / 64) * 7 + 2) * sizeof(long long));   // per-ray sums of the d_rays route (n_samples >= 64 there) + a non-finite word per ray
    L.off_slabs = off; off += align256((size_t)LNR_BWD_MAX_BLOCKS * spec->n_mlp_params * sizeof(float));
    L.off_ovf = off; off += align256(ovf_total * sizeof(long long));
    L.off_counts = off; off += align256(hash ? (size_t)blocks * L.maxo * sizeof(int) : 0);
    L.off_regions = off; off += (size_t)region_total;
    L.total = off;
    return L;
}

// flag LNR_BWD_REPORT_REGIONS: how full the record regions ran (diagnostic for sizing RegionPlan; synchronises the stream)
static void report_regions(const LnrNetSpec* spec, const Layout& L, const RegionPlan& plan, const int* counts, const int* ovf_flag, int epoch, const float* dfeat,
                           int64_t n_points, hipStream_t st) {
    std::vector<int> h((size_t)spec->n_levels * L.maxo * L.bpg);
    int used[LNR_MAX_LEVELS] = {};          // ovf_flag[l] == epoch: this call sent records of level l to the overflow accumulators
    if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(h.data(), counts, h.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(used, ovf_flag, sizeof(used), hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int l = 0; l < spec->n_levels; ++l) {
        const int rec = plan.xp[l] ? 12 : 8, cap = (int)(plan.bytes[l] / rec);
        long long sum = 0, over = 0; int mx = 0;
        const int span = lnr_level_span(spec, l, L.shift);
        for (int o = 0; o < span; ++o)
            for (int c = 0; c < L.bpg; ++c) {
                const int v = h[((size_t)l * L.maxo + o) * L.bpg + c];
                sum += v; if (v > mx) mx = v; if (v > cap) over += v - cap;
            }
        if (dfeat != nullptr && n_points > 0) {                 // how many samples carry a gradient into this level at all
            std::vector<float> plane((size_t)n_points);
            if (hipMemcpy(plane.data(), dfeat + (size_t)l * spec->n_features * L.m_pad, plane.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess) {
                long long nz = 0, runs = 0;
                for (int64_t i = 0; i < n_points; ++i) { nz += plane[i] != 0.0f; runs += (plane[i] != 0.0f) && (i == 0 || plane[i - 1] == 0.0f); }
                fprintf(stderr, "[lnr regions] level %2d: %lld of %lld samples have d_feature != 0, in %lld runs\n", l, nz, (long long)n_points, runs);
            }
        }
        fprintf(stderr, "[lnr regions] level %2d: %d-B records, capacity %d, mean %.1f, max %d, overflowed %lld of %lld, overflow accumulators %s, %d reduce workgroups per owner\n",
                l, rec, cap, (double)sum / ((double)span * L.bpg), mx, over, sum, used[l] == epoch ? "used" : "unused", (int)plan.split[l]);
    }
}

static int check_spec(const LnrNetSpec* spec, const char* who) {
    LNR_REQUIRE(spec != nullptr, "%s: null spec", who);
    LNR_REQUIRE(spec->in_dim > 0 && spec->n_mlp_params > 0, "%s: spec not finalized (call lnr_net_spec_finalize)", who);
    const int ht = spec->n_neurons / 16;
    if (!(ht == 1 || ht == 2 || ht == 4 || ht == 8 || ht == 16) || spec->n_neurons % 16) {
        lnr_set_error("%s: n_neurons=%d not supported (need 16, 32, 64, 128 or 256)", who, spec->n_neurons);
        return LNR_ERR_UNSUPPORTED;
    }
    return LNR_OK;
}

// workgroups of an MLP launch: `waves` tiles of `tile` samples each, at most max_blocks (the kernels loop over the rest)
static int mlp_blocks(int64_t n_points, int tile, int waves, int64_t max_blocks) {
    const int64_t tiles = (n_points + tile - 1) / tile;
    const int64_t blocks = (tiles + waves - 1) / waves;
    return (int)(blocks > max_blocks ? max_blocks : (blocks < 1 ? 1 : blocks));
}

static size_t fwd_lds(const LnrNetSpec* s, int w_lds) { return ((w_lds ? (size_t)lnr_w_lds_floats(s->n_neurons, s->in_dim, s->n_hidden, true) : 0) + 4) * sizeof(float); }
static size_t bwd_lds(const LnrNetSpec* s, int w_lds, int waves, int dw64) {
    const size_t H = s->n_neurons;
    const size_t scratch = H * 16 + (s->n_hidden > 1 ? (size_t)(s->n_hidden + 1) * H * 16 : 0);
    return ((w_lds ? 1 : 0) * (size_t)s->n_mlp_params + (dw64 ? 2 : 1) * (size_t)s->n_mlp_params + (size_t)waves * scratch) * sizeof(float);
}

// THE dispatch of the density MLP (DensityRoute, lnr_density_api.h): which kernel family runs a network and with which launch
// shape.  256 x 2..3 goes layer by layer; fp16 mode takes its own kernels or nothing (it says so instead of falling back); in
// fp32 the reference's default shape class (32 encoded features -> <= 64 ReLU neurons -> 1) takes the bf16x3 / register-resident
// kernels, and everything else prefers weights in LDS and 4 waves per workgroup and falls back to fewer waves, then to weights
// read from global memory (L2), until the workgroup fits the 160 KB LDS of a CDNA4 CU.
static DensityRoute lnr_route(const LnrNetSpec* spec, int64_t n_points, bool backward) {
    DensityRoute r{};
    r.waves = 4;
    const bool f16 = spec->precision == LNR_PREC_F16;
    const int64_t max_blocks = backward ? LNR_BWD_MAX_BLOCKS : LNR_DENSITY_MAX_BLOCKS;
    auto blocks = [&](int tile, int waves, int64_t cap) { r.tile = tile; return mlp_blocks(n_points, tile, waves, cap); };
    auto done = [&](int kind, int grid) {
        if (f16 && kind >= LNR_ROUTE_BF3) return DensityRoute{};          // an fp16 network the fp16 kernels do not cover: unsupported, no fall-back to fp32
        r.kind = kind; r.grid = grid;
        r.n_slabs = kind == LNR_ROUTE_WIDE ? 1 : grid;                     // one slab per workgroup; 256 x n folds its partial slabs into slab 0 itself
        return r;
    };
    if (lnr_wide_class(spec)) {          // the layer-by-layer route sizes its own launches (lnr_density_wide.hip)
        r.w_lds = 0;
        r.wide_bytes = lnr_wide_workspace(spec, n_points);
        return done(LNR_ROUTE_WIDE, 1);
    }
    if (f16 && lnr_f16_supported(spec)) {          // 32-sample tiles
        if (lnr_f16_fast_class(spec)) return done(LNR_ROUTE_F16_FAST, blocks(32, 4, max_blocks));
        const bool compile_time_act = spec->activation == LNR_ACT_RELU || spec->activation == LNR_ACT_SINE;
        r.f16_part = compile_time_act ? 0 : (backward && spec->n_neurons > 64 ? 2 : 1);
        r.fused_enc = lnr_f16_fused_freq(spec);
        // backward: one workgroup per CU (LDS), persistent over the steps
        return done(r.fused_enc ? LNR_ROUTE_F16_FREQ : LNR_ROUTE_F16_GEN, blocks(32, 4, backward ? 256 : max_blocks));
    }
    // (the register-resident kernels address up to 32 padded planes with 32-bit byte offsets: m_pad < 2^25, see lnr_bf3_class)
    if (spec->activation == LNR_ACT_RELU && spec->n_hidden == 1 && spec->in_dim == 32 && spec->enc_dim == 32 && spec->n_neurons <= 64 &&
        n_points <= (1ll << 25) - 2048) {
        r.w_lds = 1;
        r.lds = backward ? (2 * (size_t)spec->n_mlp_params + 4 * (size_t)spec->n_neurons * 20) * sizeof(float)
                         : (size_t)spec->n_mlp_params * sizeof(float);
        if (lnr_bf3_class(spec, n_points)) return done(LNR_ROUTE_BF3, blocks(32, 4, max_blocks));
        return done(LNR_ROUTE_FAST32, blocks(16, 4, max_blocks));
    }
    // backward of a general network: the register-accumulating kernel (lnr_density_regs.h) for up to three hidden layers and 128 padded
    // inputs (256 neurons: one hidden layer) - four waves, their dZ / layer-input images in LDS, the weights too when they fit
    // (from 64 neurons up: below that the whole gradient is small enough for the LDS-accumulating kernel to win - 32 Tanh x 2: 1.5 against 2.7 ms)
    if (backward && spec->n_neurons >= 64 && spec->n_hidden <= 3 && spec->in_dim <= 128 && !(spec->n_neurons == 256 && spec->n_hidden > 1)) {
        const size_t scratch = (size_t)4 * (spec->n_hidden > 1 ? 2 : 1) * spec->n_neurons * 20 * sizeof(float);       // LNR_TDZ_STRIDE rows
        const size_t weights = (size_t)lnr_w_lds_floats(spec->n_neurons, spec->in_dim, spec->n_hidden, true) * sizeof(float);       // (padded rows)
        if (scratch <= (size_t)LNR_LDS_LIMIT) {
            // weights in LDS: all of them, else the hidden matrices + output rows (read twice per step), else none
            const size_t hidden = (size_t)lnr_w_lds_floats(spec->n_neurons, spec->in_dim, spec->n_hidden, false) * sizeof(float);
            r.w_lds = scratch + weights <= (size_t)LNR_LDS_LIMIT ? 1 : (spec->n_hidden > 1 && scratch + hidden <= (size_t)LNR_LDS_LIMIT ? 2 : 0);
            r.lds = scratch + (r.w_lds == 1 ? weights : (r.w_lds == 2 ? hidden : 0));
            return done(LNR_ROUTE_REGS, blocks(16, 4, 256));            // one workgroup per CU (one wave per SIMD)
        }
    }
    // {weights in LDS, waves, 64-bit fixed-point weight-gradient accumulators}.  LDS-resident weights matter most (without
    // them every MFMA operand is a global load), then the integer accumulators (LDS float atomics are ~16x slower), then waves.
    static const int opts[12][3] = {{1, 4, 1}, {1, 2, 1}, {1, 1, 1}, {1, 4, 0}, {1, 2, 0}, {1, 1, 0},
                                    {0, 4, 1}, {0, 2, 1}, {0, 1, 1}, {0, 4, 0}, {0, 2, 0}, {0, 1, 0}};
    for (int o = 0; o < 12; ++o) {
        const int w_lds = opts[o][0], waves = opts[o][1], dw64 = opts[o][2];
        if (!backward && (waves != 4 || dw64)) continue;           // forward scratch does not depend on these
        const size_t lds = backward ? bwd_lds(spec, w_lds, waves, dw64) : fwd_lds(spec, w_lds);
        if (lds > (size_t)LNR_LDS_LIMIT) continue;
        r.w_lds = w_lds; r.waves = waves; r.lds = lds; r.dw64 = backward ? dw64 : 0;
        return done(LNR_ROUTE_LDS, blocks(16, waves, max_blocks));
    }
    DensityRoute none{};
    none.lds_misfit = 1;
    return none;
}

// LNR_ROUTE_UNSUPPORTED as the density calls report it: a legal network no kernel covers must say so, not fall back
static int route_unsupported(const LnrNetSpec* spec, const DensityRoute& route, const char* who) {
    if (route.lds_misfit)
        lnr_set_error("%s: network (n_neurons=%d, n_hidden_layers=%d, in_dim=%d: %d MLP weights) does not fit the 160 KB LDS of a CU "
                      "even with one wave per workgroup; not supported by the fp32 kernels", who, spec->n_neurons, spec->n_hidden,
                      spec->in_dim, spec->n_mlp_params);
    else
        lnr_set_error("%s: precision fp16 covers networks with an even number of encoded features per level, 16/32/64/128/256 neurons, "
                      "at most 3 hidden layers and - below 256 neurons - at most 128 (padded) inputs whose weights fit the LDS; use precision "
                      "fp32 for this network", who);
    return LNR_ERR_UNSUPPORTED;
}

extern "C" int lnr_density_route(const LnrNetSpec* spec, int64_t n_points, int32_t backward, LnrDensityRoute* out) {
    int rc = check_spec(spec, "lnr_density_route");
    if (rc) return rc;
    LNR_REQUIRE(out != nullptr && n_points >= 0, "lnr_density_route: bad argument");
    const DensityRoute r = lnr_route(spec, n_points, backward != 0);
    *out = LnrDensityRoute{r.kind, r.w_lds, r.waves, r.dw64, r.f16_part, r.kind == LNR_ROUTE_UNSUPPORTED ? 0 : r.grid, r.tile};
    return LNR_OK;
}

// the fp32 kernels on feature planes: one translation unit per width (forward, LDS-accumulating backward) / per (width, depth)
// (mlp_backward_regs_kernel)
static int mlp_fwd_ht(const MlpArgs& a) {
    switch (a.spec->n_neurons / 16) {
        case 1: return lnr_mlp_fwd_ht1(a);
        case 2: return lnr_mlp_fwd_ht2(a);
        case 4: return lnr_mlp_fwd_ht4(a);
        case 8: return lnr_mlp_fwd_ht8(a);
        default: return lnr_mlp_fwd_ht16(a);
    }
}
static int mlp_bwd_ht(const MlpArgs& a) {
    switch (a.spec->n_neurons / 16) {
        case 1: return lnr_mlp_bwd_ht1(a);
        case 2: return lnr_mlp_bwd_ht2(a);
        case 4: return lnr_mlp_bwd_ht4(a);
        case 8: return lnr_mlp_bwd_ht8(a);
        default: return lnr_mlp_bwd_ht16(a);
    }
}
static int mlp_bwd_regs(const MlpArgs& a) {
#define LNR_REGS_CASE(HT, NH) case (HT) * 4 + (NH): return lnr_mlp_bwd_regs_ht##HT##_nh##NH(a)
    switch ((a.spec->n_neurons / 16) * 4 + a.spec->n_hidden) {
        LNR_REGS_CASE(4, 1); LNR_REGS_CASE(4, 2); LNR_REGS_CASE(4, 3);
        LNR_REGS_CASE(8, 1); LNR_REGS_CASE(8, 2); LNR_REGS_CASE(8, 3);
        LNR_REGS_CASE(16, 1);
        default: lnr_set_error("lnr_density_backward: no register-accumulating kernel for %d neurons x %d hidden layers", a.spec->n_neurons, a.spec->n_hidden); return LNR_ERR_UNSUPPORTED;
    }
#undef LNR_REGS_CASE
}

static int make_src(PointSrc* s, MlpPoints* mp, const float* pts, int64_t n_points, const float* rays, const float* z,
                    int32_t n_rays, int32_t n_samples, const int32_t* n_rays_dev, const char* who) {
    if (pts != nullptr) {
        LNR_REQUIRE(n_points >= 0, "%s: negative n_points", who);
        *s = PointSrc{pts, nullptr, nullptr, 1, n_points, 0, nullptr};
        *mp = MlpPoints{n_points, nullptr, 0, 1, nullptr};
    } else {
        LNR_REQUIRE(rays != nullptr && z != nullptr, "%s: need either pts or (rays, z)", who);
        LNR_REQUIRE(n_rays >= 0 && n_samples > 0, "%s: bad n_rays/n_samples", who);
        *s = PointSrc{nullptr, rays, z, n_samples, 0, n_rays, n_rays_dev};
        *mp = MlpPoints{(int64_t)n_rays * n_samples, n_rays_dev, n_rays, n_samples, nullptr};
    }
    return LNR_OK;
}

// The head of lnr_density_forward, lnr_density_backward and lnr_density_fold_weight_grads (`who`): everything that happens before
// the first launch, in one order, so that a bad call fails with the same status and text whichever entry point it reaches.
struct CallHead { PointSrc src; MlpPoints mp; int64_t cap; DensityRoute route; Layout L; };
enum { HEAD_FORWARD, HEAD_BACKWARD, HEAD_FOLD };
// route and layout for h->cap points, then the checks that need them: the 32-bit plane offsets, the workspace size, the route
static int head_plan(const LnrNetSpec* spec, int kind, size_t workspace_bytes, const char* who, CallHead* h) {
    h->route = lnr_route(spec, h->cap, kind != HEAD_FORWARD);          // (the fold: the route of the backward whose slabs these are)
    h->L = make_layout(spec, h->cap, h->route);
    const size_t need = kind == HEAD_FORWARD ? h->L.off_dfeat : h->L.total;
    if (kind == HEAD_FOLD) LNR_REQUIRE(workspace_bytes >= need, "%s: workspace too small", who);
    else {
        // (the limit is on the PADDED plane stride - the sample count rounded up to 64, plus the skew: ADVICE r5)
        LNR_REQUIRE(h->L.m_pad * (spec->n_features > 4 ? spec->n_features : 4) < (1ll << 30),
                    "%s: too many points per call for 32-bit plane offsets (padded n_points * max(n_features, 4) must be < 2^30)", who);
        if (workspace_bytes < need) {
            lnr_set_error("%s: workspace %zu < %zu (%s)", who, workspace_bytes, need, kind == HEAD_FORWARD ? "lnr_density_workspace_forward" : "lnr_density_workspace");
            return LNR_ERR_WORKSPACE;
        }
    }
    return h->route.kind == LNR_ROUTE_UNSUPPORTED ? route_unsupported(spec, h->route, who) : LNR_OK;
}
// forward and backward: the spec, the points (h->cap == 0 with LNR_OK: an empty batch - nothing to do, nothing was checked), the entry
// point's own argument check (bad_args: what is wrong with them, or NULL), then head_plan
static int call_head(const LnrNetSpec* spec, int kind, const char* who, const float* pts, int64_t n_points, const float* rays, const float* z, int32_t n_rays,
                     int32_t n_samples, const int32_t* n_rays_dev, const char* bad_args, size_t workspace_bytes, CallHead* h) {
    h->cap = 0;
    int rc = check_spec(spec, who);
    if (rc || (n_points == 0 && (pts != nullptr || n_rays == 0))) return rc;
    rc = make_src(&h->src, &h->mp, pts, n_points, rays, z, n_rays, n_samples, n_rays_dev, who);
    if (rc || h->mp.n_points == 0) return rc;
    LNR_REQUIRE(bad_args == nullptr, "%s: %s", who, bad_args);
    h->cap = h->mp.n_points;
    return head_plan(spec, kind, workspace_bytes, who, h);
}

extern "C" size_t lnr_density_workspace(const LnrNetSpec* spec, int64_t n_points) {
    if (!spec || n_points < 0) return 0;
    return make_layout(spec, n_points, lnr_route(spec, n_points, true)).total;
}

extern "C" size_t lnr_density_workspace_forward(const LnrNetSpec* spec, int64_t n_points) {
    if (!spec || n_points < 0) return 0;
    return make_layout(spec, n_points, lnr_route(spec, n_points, false)).off_dfeat;          // status words + feature planes: all the forward touches
}

extern "C" int lnr_density_workspace_init(void* workspace, size_t workspace_bytes, void* stream) {
    LNR_REQUIRE(workspace != nullptr && workspace_bytes >= LNR_WORKSPACE_STATUS_BYTES, "lnr_density_workspace_init: workspace too small");
    ws_forget(workspace);
    if (hipMemsetAsync(workspace, 0, LNR_WORKSPACE_STATUS_BYTES, (hipStream_t)stream) != hipSuccess) {
        lnr_set_error("lnr_density_workspace_init: hipMemsetAsync failed");
        return LNR_ERR_LAUNCH;
    }
    return LNR_OK;
}

extern "C" int lnr_density_workspace_release(void* workspace) {
    LNR_REQUIRE(workspace != nullptr, "lnr_density_workspace_release: null workspace");
    ws_forget(workspace);
    return LNR_OK;
}

extern "C" int lnr_density_forward(const LnrNetSpec* spec, const float* params, const float* pts, int64_t n_points,
                                   const float* rays, const float* z, int32_t n_rays, int32_t n_samples,
                                   const int32_t* n_rays_dev, float* sigma, void* workspace, size_t workspace_bytes, void* stream) {
    CallHead h;
    int rc = call_head(spec, HEAD_FORWARD, "lnr_density_forward", pts, n_points, rays, z, n_rays, n_samples, n_rays_dev,
                       params && sigma && workspace ? nullptr : "null params/sigma/workspace", workspace_bytes, &h);
    if (rc || h.cap == 0) return rc;
    const PointSrc& src = h.src; MlpPoints& mp = h.mp; const int64_t cap = h.cap; const DensityRoute& route = h.route; const Layout& L = h.L;
    hipStream_t st = (hipStream_t)stream;
    ws_touch(workspace, layout_signature(spec, cap));
    float* feat = (float*)((char*)workspace + L.off_feat);
    mp.clip_flag = reinterpret_cast<int32_t*>((char*)workspace + L.off_status) + LNR_STATUS_CLIPPED;
    if (!route.fused_enc) {
        LnrProfScope prof("encode_forward", st);
        rc = lnr_encode_forward(spec, params, &src, cap, feat, L.m_pad, spec->precision == LNR_PREC_F16, st);
    }
    if (rc) return rc;
    LNR_CHECK_LAUNCH("lnr_density_forward(encode)");
    LnrProfScope prof_mlp("mlp_forward", st);
    const MlpArgs a{spec, &route, params, feat, L.m_pad, &mp, sigma, nullptr, nullptr, nullptr, 0, 0, &src, nullptr, (char*)workspace + L.off_wide, st};
    const char* what;
    switch (route.kind) {
        case LNR_ROUTE_WIDE: rc = lnr_mlp_fwd_wide(a); what = "lnr_density_forward(mlp 256 x n)"; break;
        case LNR_ROUTE_F16_FAST: case LNR_ROUTE_F16_FREQ: case LNR_ROUTE_F16_GEN: rc = lnr_mlp_fwd_f16(a); what = "lnr_density_forward(mlp f16)"; break;
        case LNR_ROUTE_BF3: rc = lnr_mlp_fwd_bf3(a); what = "lnr_density_forward(mlp bf16x3)"; break;
        default: rc = mlp_fwd_ht(a); what = "lnr_density_forward(mlp)"; break;          // LNR_ROUTE_FAST32, LNR_ROUTE_LDS
    }
    if (rc) return rc;
    LNR_CHECK_LAUNCH(what);
    return LNR_OK;
}

extern "C" int lnr_density_backward(const LnrNetSpec* spec, const float* params, const float* pts, int64_t n_points,
                                    const float* rays, const float* z, int32_t n_rays, int32_t n_samples,
                                    const int32_t* n_rays_dev, const float* d_sigma, float* grad_params, float* d_pts, float* d_rays,
                                    int32_t reuse_features, int32_t flags, void* workspace, size_t workspace_bytes, void* input_grad_event,
                                    void* stream) {
    hipStream_t st = (hipStream_t)stream;
    // the input gradient (d_pts / d_rays) is complete where this is called; what follows only finishes grad_params.  A caller that
    // continues with the input gradient on another stream (pose gradient, pose step, the next batch's rays and samples) waits for this
    // event instead of for the whole call.  An empty batch has nothing to compute, but the event is part of the contract of every
    // successful call: an unrecorded event would let that stream run against the PREVIOUS call's record
    auto input_grad_done = [&]() -> int {
        if (input_grad_event != nullptr && hipEventRecord((hipEvent_t)input_grad_event, st) != hipSuccess) {
            lnr_set_error("lnr_density_backward: hipEventRecord failed");
            return LNR_ERR_LAUNCH;
        }
        return LNR_OK;
    };
    CallHead h;
    int rc = call_head(spec, HEAD_BACKWARD, "lnr_density_backward", pts, n_points, rays, z, n_rays, n_samples, n_rays_dev,
                       !(params && d_sigma && workspace) ? "null argument"
                       : !(grad_params || d_pts || d_rays) ? "nothing to compute (no grad_params, d_pts or d_rays)" : nullptr, workspace_bytes, &h);
    if (rc) return rc;
    if (h.cap == 0) return input_grad_done();
    const PointSrc& src = h.src; const MlpPoints& mp = h.mp; const int64_t cap = h.cap; const DensityRoute& route = h.route; const Layout& L = h.L;
    char* ws = (char*)workspace;
    float* feat = (float*)(ws + L.off_feat);
    float* dfeat = (float*)(ws + L.off_dfeat);
    float* dxl = (float*)(ws + L.off_dxl);
    float* slabs = (float*)(ws + L.off_slabs);
    long long* ovf = (long long*)(ws + L.off_ovf);
    int* counts = (int*)(ws + L.off_counts);
    void* regions = (void*)(ws + L.off_regions);
    const bool hash = spec->encoding == LNR_ENC_HASHGRID;
    // test hook: LNR_BWD_TABLE_ATOMICS sends every record down the global-atomic fallback path (same result, ~20x slower);
    // the tests use it as an independent implementation of the record partition
    RegionPlan rplan = L.plan;
    if (flags & LNR_BWD_TABLE_ATOMICS)                       // no room anywhere: every record takes the overflow path
        for (int l = 0; l < LNR_MAX_LEVELS; ++l) rplan.bytes[l] = 0;
    const bool want_grad = grad_params != nullptr;

    const bool fused_freq = route.fused_enc;          // encoding and its input gradient inside the MLP backward kernel
    if (!reuse_features && !fused_freq) {
        LnrProfScope prof("encode_forward", st);
        rc = lnr_encode_forward(spec, params, &src, cap, feat, L.m_pad, spec->precision == LNR_PREC_F16, st);
        if (rc) return rc;
        LNR_CHECK_LAUNCH("lnr_density_backward(encode)");
    }
    // d_rays (rays form only): the input gradient goes straight into the ray records.  When a wave's 64 samples lie on one
    // ray (n_samples % 64 == 0) and there is a table to walk, the encode kernels accumulate it themselves; otherwise it
    // takes the general route (d/dx planes -> d_pts scratch in the workspace -> lnr_points_grad_to_rays).
    LNR_REQUIRE(!(d_rays && pts), "lnr_density_backward: d_rays needs the rays form");
    LNR_REQUIRE(!(d_rays && d_pts), "lnr_density_backward: pass d_pts or d_rays, not both");
    const bool ray_accum = d_rays != nullptr && hash && (n_samples % 64 == 0);
    float* d_pts_eff = d_pts;
    if (d_rays && !ray_accum) d_pts_eff = (float*)(ws + L.off_dpts);
    const int want_dfeat = ((hash && want_grad) || d_pts_eff != nullptr || ray_accum) ? 1 : 0;
    {
    LnrProfScope prof("mlp_backward", st);
    const MlpArgs a{spec, &route, params, feat, L.m_pad, &mp, nullptr, d_sigma, dfeat, slabs, want_dfeat, want_grad ? 1 : 0, &src, d_pts_eff, ws + L.off_wide, st};
    switch (route.kind) {
        case LNR_ROUTE_WIDE: rc = lnr_mlp_bwd_wide(a); break;
        case LNR_ROUTE_F16_FAST: case LNR_ROUTE_F16_FREQ: case LNR_ROUTE_F16_GEN: rc = lnr_mlp_bwd_f16(a); break;
        case LNR_ROUTE_BF3: rc = lnr_mlp_bwd_bf3(a); break;
        case LNR_ROUTE_REGS: rc = mlp_bwd_regs(a); break;
        default: rc = mlp_bwd_ht(a); break;          // LNR_ROUTE_FAST32, LNR_ROUTE_LDS
    }
    }
    if (rc) return rc;
    LNR_CHECK_LAUNCH("lnr_density_backward(mlp)");
    float* grad_table = want_grad ? grad_params + spec->n_mlp_params : nullptr;
    // the overflow accumulators: all-zero between calls (WsNote above); cleared here only when that is not known
    int* ovf_flag = reinterpret_cast<int32_t*>(ws + L.off_status) + LNR_STATUS_OVF_LEVEL0;
    int epoch = 0;
    const bool uses_ovf = hash && want_grad;
    if (uses_ovf) {
        bool clear = false;
        ws_backward_begin(workspace, layout_signature(spec, cap), &epoch, &clear);
        if (clear && (hipMemsetAsync(ovf, 0, L.off_counts - L.off_ovf, st) != hipSuccess ||
                      hipMemsetAsync(ovf_flag, 0, LNR_MAX_LEVELS * sizeof(int32_t), st) != hipSuccess)) {
            lnr_set_error("lnr_density_backward: hipMemsetAsync failed");
            return LNR_ERR_LAUNCH;
        }
    } else {
        ws_touch(workspace, layout_signature(spec, cap));
    }
    // the weight-gradient fold rides in the table reduce's launch whenever both run in this call
    const bool fold_in_reduce = want_grad && hash && L.nown > 0 && !(flags & LNR_BWD_DEFER_WEIGHT_FOLD);
    const TableGradSink sink{grad_table, want_grad ? regions : nullptr, rplan, counts, L.bpg, L.maxo, L.shift, ovf, ovf_flag, epoch};
    const SlabFold fold{slabs, route.n_slabs, spec->n_mlp_params, grad_params};
    const int overwrite = (flags & LNR_BWD_OVERWRITE_GRAD) ? 1 : 0;
    if (want_dfeat && !fused_freq) {
        const InputGradOut out{dxl, d_pts_eff, ray_accum ? d_rays : nullptr, (long long*)(ws + L.off_rayacc)};
        rc = lnr_encode_backward(spec, params, &src, cap, dfeat, L.m_pad, sink, out, st);
        if (rc) return rc;
        LNR_CHECK_LAUNCH("lnr_density_backward(encode backward)");
    }
    if (d_rays && !ray_accum) {
        rc = lnr_points_grad_to_rays(d_pts_eff, z, n_rays, n_rays_dev, n_samples, d_rays, stream);
        if (rc) return rc;
    }
    rc = input_grad_done();
    if (rc || !want_grad) return rc;       // frozen parameters: no table reduce, no weight-gradient fold
    if (want_dfeat) {
        if (hash && (flags & LNR_BWD_REPORT_REGIONS)) {           // diagnostic, call-time flag: synchronises the stream
            int64_t live = cap;
            int32_t nr = 0;
            if (n_rays_dev && hipStreamSynchronize(st) == hipSuccess && hipMemcpy(&nr, n_rays_dev, sizeof(nr), hipMemcpyDeviceToHost) == hipSuccess) live = (int64_t)nr * n_samples;
            report_regions(spec, L, rplan, counts, ovf_flag, epoch, dfeat, live, st);
        }
    }
    if (hash && L.nown > 0) {          // also with cap_rec == 0 (all-atomic test path): it folds in the overflow accumulators
        rc = lnr_launch_table_reduce(spec, sink, L.nown, (flags & LNR_BWD_TABLE_ATOMICS) ? 0 : L.n_split, fold_in_reduce ? fold : SlabFold{}, overwrite, st);
        if (rc) return rc;
        LNR_CHECK_LAUNCH("lnr_density_backward(table reduce)");
        ws_backward_done(workspace);                  // the reduce has put every accumulator it read back to zero
#ifdef LNR_PHASE_TIMING
        lnr_table_reduce_print_phases(st);
#endif
    }
    // (folding the slabs right after the MLP backward instead was measured: +15 us in front of the encode backward, nothing gained)
    if ((flags & LNR_BWD_DEFER_WEIGHT_FOLD) || fold_in_reduce) return LNR_OK;      // the caller folds them (lnr_density_fold_weight_grads) / done above
    lnr_launch_slab_fold(fold, overwrite, st);
    LNR_CHECK_LAUNCH("lnr_density_backward(reduce)");
    return LNR_OK;
}

extern "C" int lnr_density_fold_weight_grads(const LnrNetSpec* spec, int64_t n_points, float* grad_params, void* workspace,
                                             size_t workspace_bytes, int32_t flags, void* stream) {
    int rc = check_spec(spec, "lnr_density_fold_weight_grads");
    if (rc) return rc;
    LNR_REQUIRE(grad_params && workspace && n_points > 0, "lnr_density_fold_weight_grads: bad argument");
    CallHead h;
    h.cap = n_points;
    rc = head_plan(spec, HEAD_FOLD, workspace_bytes, "lnr_density_fold_weight_grads", &h);
    if (rc) return rc;
    lnr_launch_slab_fold(SlabFold{(const float*)((const char*)workspace + h.L.off_slabs), h.route.n_slabs, spec->n_mlp_params, grad_params},
                         (flags & LNR_BWD_OVERWRITE_GRAD) ? 1 : 0, (hipStream_t)stream);
    LNR_CHECK_LAUNCH("lnr_density_fold_weight_grads");
    return LNR_OK;
}

// ------------------------------------------------------------------------------------------------
// MFMA layout self-test: D = A(16x4) * B(4x16) with asymmetric operands, checked against the
// layout the kernels assume (A: lane->A[l&15][l>>4]; B: lane->B[l>>4][l&15]; D: reg r ->
// D[4*(l>>4)+r][l&15]).
// ------------------------------------------------------------------------------------------------
__global__ void selftest_mfma_kernel(float* out) {
    const int lane = threadIdx.x;
    const int i = lane & 15, k = lane >> 4;
    const float a = (float)(i * 7 + k * 3 + 1) * 0.25f;          // A[i][k]
    const float b = (float)((lane & 15) * 5 - k * 11 + 2) * 0.5f; // B[k][j], j = lane&15
    f32x4 d = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, d, 0, 0, 0);
    float err = 0.0f;
    const int j = lane & 15;
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * (lane >> 4) + r;
        float ref = 0.0f;
        for (int kk = 0; kk < 4; ++kk) ref += ((float)(row * 7 + kk * 3 + 1) * 0.25f) * ((float)(j * 5 - kk * 11 + 2) * 0.5f);
        err = fmaxf(err, fabsf(ref - d[r]));
    }
    err = wave_max(err);
    if (lane == 0) out[0] = err;
}

extern "C" int lnr_selftest_mfma(float* out, void* stream) {
    LNR_REQUIRE(out != nullptr, "lnr_selftest_mfma: null out");
    hipLaunchKernelGGL(selftest_mfma_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out);
    lnr_selftest_mfma_f16(out, (hipStream_t)stream);
    lnr_selftest_mfma_bf3(out, (hipStream_t)stream);
    LNR_CHECK_LAUNCH("lnr_selftest_mfma");
    return LNR_OK;
}
