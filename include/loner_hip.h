/*
 * loner_hip.h -- C ABI of libloner_hip.so, the MI355X (gfx950) implementation of the
 * LONER mapping-thread hot path.
 *
 * The reference (umautobots/LONER) is pure Python: its "native" layer on this path is
 * torch ops plus the tinycudann CUDA extension, reached through Python classes.  It has
 * no FFI of its own, so every entry point below cites the reference *function* it
 * replaces (paths relative to the reference root).  The Python classes that mirror the
 * reference's interface (loner_amd/models/..., loner_amd/mapping/...) bind these symbols
 * with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *   - tensors are dense, row-major, float32 unless stated; the caller owns all buffers;
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*);
 *   - return value 0 = success, negative = LnrStatus error (nothing was enqueued);
 *   - the library keeps no global state and is re-entrant per stream;
 *   - `n_rays_dev` (nullable): if non-null the kernels read the live ray count from
 *     device memory (<= the `n_rays` capacity given by value) so that a window whose
 *     ray count depends on data (rays dropped by the cube test) needs no host sync.
 *
 * Ray record (13 floats): [origin(3) dir(3) viewdir(3) 0 0 near far]  (ray_utils.py:307-310)
 */
#ifndef LONER_HIP_H
#define LONER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LNR_RAY_STRIDE 13
#define LNR_LOSS_RAYS_PER_BLOCK 4
#define LNR_LOSS_MAX_SAMPLES 1024   /* lnr_los_loss_fused refuses more samples per ray (LNR_ERR_UNSUPPORTED) */
#define LNR_MAX_LEVELS 32

typedef enum LnrStatus {
    LNR_OK = 0,
    LNR_ERR_INVALID_ARG = -1,
    LNR_ERR_UNSUPPORTED = -2,   /* legal config the kernels do not cover (message via lnr_last_error) */
    LNR_ERR_LAUNCH = -3,        /* hipGetLastError() != hipSuccess after a launch */
    LNR_ERR_WORKSPACE = -4      /* workspace too small */
} LnrStatus;

typedef enum LnrEncoding { LNR_ENC_HASHGRID = 0, LNR_ENC_FREQUENCY = 1 } LnrEncoding;

/* Arithmetic of the density network.  The reference runs tinycudann in half precision (fp16 parameters copy, fp16 encoded
 * features, FullyFusedMLP on tensor cores: cfg/nerf_config/default_nerf_hash.yaml:20-31, src/models/nerf_tcnn.py:35-38).
 *   LNR_PREC_F32: everything in fp32; stricter than the reference, the default.  Matrix products of the reference's default shape
 *                 class (32 encoded features -> <= 64 ReLU neurons -> 1) run on the bf16 matrix pipe with every fp32 operand split
 *                 into three bf16 terms (x = x0 + x1 + x2 exactly) and the six largest partial products accumulated in fp32:
 *                 error per product below 2^-24 relative (the order of fp32's own rounding; exact for operands of <= 16 significant
 *                 bits), ~2.5x the speed of the fp32 MFMA.  Every other network: v_mfma_f32_16x16x4_f32 (exact fp32 fma chains).
 *   LNR_PREC_F32_CHAIN: fp32 with exact fma chains (v_mfma_f32_16x16x4_f32) for every network, the default class included.
 *   LNR_PREC_F16: the reference's storage types - encoded features and MLP weights rounded to fp16, matrix products on
 *                 v_mfma_f32_16x16x32_f16 with fp32 accumulation (the reference accumulates in fp16), fp32 master
 *                 parameters and fp32 gradients (the reference: fp16 atomics with a loss scale of 128). */
typedef enum LnrPrecision { LNR_PREC_F32 = 0, LNR_PREC_F16 = 1, LNR_PREC_F32_CHAIN = 2 } LnrPrecision;

/* Grid position of the hash-grid lookup, pos = x*scale + 0.5:  LNR_POS_FMA rounds once (tiny-cuda-nn's fmaf, the
 * default), LNR_POS_MUL_ADD rounds the product and the sum separately (what un-contracted code would do).  The two
 * differ by one fp32 ulp of pos = 1/32 cell on the finest default level. */
typedef enum LnrPosRounding { LNR_POS_FMA = 0, LNR_POS_MUL_ADD = 1 } LnrPosRounding;

/* Failure guard.  The reference checks, in EVERY iteration, the loss for NaN (inside compute_loss, optimizer.py:590) and - after
 * backward, before optimizer.step() - every pose gradient and pose tensor for non-finite values (optimizer.py:368-374); an
 * exception leaves the step of that iteration unreached.  Without a host sync per iteration the same contract is kept on the
 * device: `poison_dev` (nullable everywhere) is an int32[2] word {code, tag}, zeroed by the caller at the start of a phase.
 * lnr_los_loss_fused and lnr_pose_backward set it (first event wins; tag = the caller's iteration index) and lnr_adam_step /
 * lnr_occ_grid_apply do nothing once it is non-zero, so parameters, poses and the occupancy grid stay at the values they had
 * when the failing iteration began; the host reads the word once per phase and raises the reference's error. */
#define LNR_POISON_NAN_LOSS 1    /* AssertionError("NaN Loss Encountered") */
#define LNR_POISON_POSE_GRAD 2   /* RuntimeError("Fatal: Encountered invalid gradient in pose.") */
#define LNR_POISON_POSE 3        /* RuntimeError("Fatal: Encountered invalid pose tensor.") */

/* lnr_density_backward flags */
#define LNR_BWD_TABLE_ATOMICS 1   /* test hook: every table-gradient record goes to the 64-bit overflow accumulators (atomics) */
#define LNR_BWD_DEFER_WEIGHT_FOLD 16 /* leave the per-workgroup weight-gradient slabs in the workspace: the caller adds them to grad_params
                                       with lnr_density_fold_weight_grads (same points capacity) - e.g. on another stream, beside the
                                       table-gradient reduce, instead of behind it */
#define LNR_BWD_REPORT_REGIONS 2  /* diagnostic: print to stderr how full the record regions ran (synchronises the stream) */
#define LNR_BWD_OVERWRITE_GRAD 32 /* grad_params RECEIVES this call's gradient instead of accumulating it: the table-gradient reduce writes
                                       every float of its slice (zeros included) without reading it, the weight-gradient fold stores
                                       instead of adding.  A training loop that steps after every backward then needs neither the 30 MB
                                       read here nor the optimiser's zeroing of the gradient (lnr_adam_step zero_grad = 0): 60 MB of HBM
                                       traffic per iteration.  With LNR_BWD_DEFER_WEIGHT_FOLD pass the same flag to
                                       lnr_density_fold_weight_grads. */

typedef enum LnrActivation {
    LNR_ACT_NONE = 0, LNR_ACT_RELU = 1, LNR_ACT_SINE = 2, LNR_ACT_LEAKY_RELU = 3,
    LNR_ACT_EXPONENTIAL = 4, LNR_ACT_SIGMOID = 5, LNR_ACT_SQUAREPLUS = 6,
    LNR_ACT_SOFTPLUS = 7, LNR_ACT_TANH = 8
} LnrActivation;

/* Density network = input encoding + bias-free MLP; the config schema is tinycudann's as
 * used by src/models/nerf_tcnn.py:29-38 (cfg/nerf_config/default_nerf_hash.yaml keys
 * pos_encoding_sigma / sigma_network).  Fill the first block, call lnr_net_spec_finalize. */
typedef struct LnrNetSpec {
    /* -- configuration -- */
    int32_t encoding;          /* LnrEncoding */
    int32_t n_levels;          /* HashGrid */
    int32_t n_features;        /* HashGrid: features per level, 1 | 2 | 4 | 8 */
    int32_t log2_table;        /* HashGrid: log2_hashmap_size */
    int32_t base_res;          /* HashGrid: base_resolution */
    float   per_level_scale;   /* HashGrid */
    int32_t n_frequencies;     /* Frequency */
    int32_t activation;        /* LnrActivation of the hidden layers */
    int32_t n_neurons;         /* hidden width, multiple of 16, <= 256 */
    int32_t n_hidden;          /* hidden layers, >= 1 */
    int32_t precision;         /* LnrPrecision (0 = fp32) */
    int32_t pos_rounding;      /* LnrPosRounding (0 = fma) */
    /* -- derived by lnr_net_spec_finalize -- */
    int32_t enc_dim;           /* encoding outputs */
    int32_t in_dim;            /* enc_dim rounded up to 16 (padding inputs are the constant 1) */
    int32_t n_mlp_params;      /* H*in_dim + (n_hidden-1)*H*H + 16*H */
    int64_t n_params;          /* MLP matrices first ([out][in] row-major), then encoding tables */
    float    level_scale[LNR_MAX_LEVELS];
    uint32_t level_res[LNR_MAX_LEVELS];
    uint32_t level_size[LNR_MAX_LEVELS];    /* entries */
    uint32_t level_offset[LNR_MAX_LEVELS];  /* entries, from the start of the encoding block */
    uint32_t level_hashed[LNR_MAX_LEVELS];
} LnrNetSpec;

/* Loss configuration = model_config.loss (cfg/model_config/default_model_config.yaml:42-63). */
typedef struct LnrLossConfig {
    int32_t selection;     /* 0 L1_JS, 1 L2_JS, 2 L1_LOS, 3 L2_LOS  (optimizer.py:493-534,568-574) */
    float min_js, max_js, js_alpha;
    float los_lambda;      /* already decayed by the caller if decay_los_lambda (optimizer.py:448-452) */
    float depth_lambda;
    float min_eps;         /* min_depth_eps */
    float fixed_eps;       /* LOS variants: the (decayed) depth_eps for this iteration */
} LnrLossConfig;

const char* lnr_last_error(void);          /* host; thread-local text for the last negative status */
int  lnr_version(void);

/* Optional per-kernel timing of the entry points that launch several kernels (density forward / backward): when
 * enabled, HIP events are recorded on the caller's stream around each internal launch.  lnr_profile_read waits for the
 * recorded events, returns the number of distinct kernels (names [n][name_stride] chars, summed milliseconds, calls)
 * and clears the log.  Diagnostics only; off by default. */
int lnr_profile_enable(int32_t on);
int lnr_profile_read(char* names, int32_t name_stride, float* total_ms, int32_t* calls, int32_t capacity);

/* ---- density network ------------------------------------------------------------------------- */
int lnr_net_spec_finalize(LnrNetSpec* spec /*host, in/out*/);

/* Scratch both density calls need, sized for up to n_points points per call: feature planes [enc_dim][n_points],
 * their gradient, per-level d/dx planes, per-workgroup weight-gradient slabs and the record regions of the
 * table-gradient partition.  The content between calls only matters for `reuse_features` below.
 * Limits: n_points * max(n_features_per_level, 4) < 2^30 per call, encoding table < 2^30 floats (32-bit byte offsets). */
size_t lnr_density_workspace(const LnrNetSpec* spec /*host*/, int64_t n_points);
/* The part of it lnr_density_forward alone needs (status words + feature planes): rendering / inference callers
 * (Model.forward(testing=True), analysis/compute_l1_depth.py:42-64) never pay for the backward's record regions. */
size_t lnr_density_workspace_forward(const LnrNetSpec* spec /*host*/, int64_t n_points);

/* Which MLP kernels lnr_density_forward (backward = 0) / lnr_density_backward (backward = 1) launch for this network at up to
 * n_points points per call, from the same function the launch path reads.  Host only: touches no device, needs no workspace.
 *   LNR_ROUTE_UNSUPPORTED  no kernel: the density calls return LNR_ERR_UNSUPPORTED
 *   LNR_ROUTE_WIDE         256 neurons x 2..3 hidden layers (and 256 x 1 in fp16 mode where the fused kernels do not fit), both
 *                          precisions: layer by layer through chunk planes in the workspace
 *   LNR_ROUTE_F16_FAST     fp16 mode, the reference's sigma network (16 levels x 2 features -> <= 64 ReLU neurons -> 1)
 *   LNR_ROUTE_F16_FREQ     fp16 mode, frequency encoding evaluated inside the general fp16 kernels (no feature planes)
 *   LNR_ROUTE_F16_GEN      fp16 mode, general kernels on half2 pair planes
 *   LNR_ROUTE_BF3          LNR_PREC_F32, the default shape class on the bf16 matrix pipe with three-term operand splits
 *   LNR_ROUTE_FAST32       the default shape class on the register-resident fp32 kernels (LNR_PREC_F32_CHAIN, frequency encodings)
 *   LNR_ROUTE_REGS         fp32 backward that accumulates the weight gradient in registers; w_lds: 1 all weights, 2 the hidden
 *                          matrices, 0 none in LDS
 *   LNR_ROUTE_LDS          general fp32 kernels; w_lds (weights in LDS), waves per workgroup and - backward - dw64 (64-bit
 *                          fixed-point weight-gradient accumulators) name the tier that fits the LDS
 * f16_part: the object of the general fp16 kernels that holds the kernel (0: compile-time ReLU / Sine; run-time activations:
 * forward 1, backward 1 up to 64 neurons and 2 from 128); 0 for every other route.
 * grid, tile: the launch shape of the MLP kernels - workgroups (of four waves on every route but LNR_ROUTE_LDS, which has `waves`) and
 * samples a wave takes per step of its loop (32 or 16); wave w of workgroup b runs tiles b * waves + w, + grid * waves, ...  Both are 0
 * for LNR_ROUTE_UNSUPPORTED, tile is 0 for LNR_ROUTE_WIDE (it sizes its own launches). */
typedef enum LnrRouteKind {
    LNR_ROUTE_UNSUPPORTED = 0, LNR_ROUTE_WIDE = 1, LNR_ROUTE_F16_FAST = 2, LNR_ROUTE_F16_FREQ = 3, LNR_ROUTE_F16_GEN = 4,
    LNR_ROUTE_BF3 = 5, LNR_ROUTE_FAST32 = 6, LNR_ROUTE_REGS = 7, LNR_ROUTE_LDS = 8
} LnrRouteKind;
typedef struct LnrDensityRoute { int32_t kind, w_lds, waves, dw64, f16_part, grid, tile; } LnrDensityRoute;
int lnr_density_route(const LnrNetSpec* spec /*host*/, int64_t n_points, int32_t backward, LnrDensityRoute* out /*host*/);

/* The first LNR_WORKSPACE_STATUS_BYTES of a workspace are int32 status words the kernels write and the caller may read (with
 * the device in sync) and reset; lnr_density_workspace_init zeroes them - call it once after allocating a workspace.
 *   [LNR_STATUS_CLIPPED]  number of density outputs lnr_density_forward clipped since the last reset: non-finite values - and, with
 *                         LNR_PREC_F16, values beyond +-65504, which the reference's fp16 network returns as +-inf - are replaced
 *                         by the extremes of the network's dtype, NaN by 0, as DecoupledNeRF.forward does with nan_to_num
 *                         (nerf_tcnn.py:70-78); the caller prints the reference's "Clipping infinite outputs" warning once. */
#define LNR_WORKSPACE_STATUS_BYTES 256
#define LNR_STATUS_CLIPPED 0
#define LNR_STATUS_OVF_LEVEL0 16      /* [16 .. 16 + LNR_MAX_LEVELS): internal - the call stamp of the last lnr_density_backward that used a level's
                                          64-bit overflow accumulators (those are kept all-zero between calls instead of cleared per call).
                                          Between two density calls on a workspace its content belongs to the library: a caller that writes
                                          into it - or hands it to another network / batch size - is fine (that is detected by layout), one
                                          that scribbles over it from outside must call lnr_density_workspace_init again. */
/* REQUIRED once for every allocation that is used as a workspace - also for a new allocation that happens to get the address of a
 * released one: the library keeps a small host-side note per workspace ADDRESS (layout signature, call stamp, "overflow accumulators
 * known zero"), which lnr_density_workspace_init resets.  Without it a recycled address would be believed to hold zeroed accumulators.
 * lnr_density_workspace_release drops the note when a workspace is freed (optional but tidy: the notes are bounded - beyond 64 of them
 * every note is dropped, which only costs the next backward on each workspace one clear).  One workspace serves one stream at a time:
 * forward and backward of a call pair, and successive calls, are ordered by the stream they are issued on. */
int lnr_density_workspace_init(void* workspace, size_t workspace_bytes, void* stream);
int lnr_density_workspace_release(void* workspace);

/* sigma = MLP(enc((xyz+1)/2))[0]           replaces tinycudann forward at nerf_tcnn.py:63-72
 * Points are given either explicitly (pts != NULL, [n_points,3] in the world cube [-1,1]) or
 * implicitly as rays [n_rays,13] + z [n_rays,n_samples] (xyz = o + d*z, rendering_tcnn.py:241).
 * Two launches: level-major encoding into the workspace's feature planes, then the MLP on those planes. */
int lnr_density_forward(const LnrNetSpec* spec /*host*/, const float* params,
                        const float* pts, int64_t n_points,
                        const float* rays, const float* z, int32_t n_rays, int32_t n_samples,
                        const int32_t* n_rays_dev,
                        float* sigma /*[n_points] or [n_rays*n_samples]*/,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the above                     replaces tinycudann backward (loss.backward(), optimizer.py:366)
 * grad_params [n_params] is ACCUMULATED into (caller zeroes it; lnr_adam_step can re-zero it); NULL = parameters frozen
 * (tracking phase, optimizer.py:239-259): only the input gradient is computed, no table-gradient records, no reduce.
 * d_pts (nullable) [*,3] receives dL/dxyz per point (needed only when poses are optimised).
 * d_rays (nullable, rays form only, instead of d_pts) [n_rays,13]: dL/dxyz is reduced over the samples of each ray and
 * ADDED to the ray-record gradient (origin cols 0:3 += sum dL/dxyz, direction cols 3:6 += sum z dL/dxyz) - what
 * lnr_points_grad_to_rays does with d_pts, without materialising d_pts (64-bit fixed-point sums: reproducible).
 * reuse_features != 0: the workspace still holds the feature planes lnr_density_forward wrote for the SAME
 * spec, params and points (tinycudann keeps its forward activations the same way); 0 re-encodes first. */
int lnr_density_backward(const LnrNetSpec* spec /*host*/, const float* params,
                         const float* pts, int64_t n_points,
                         const float* rays, const float* z, int32_t n_rays, int32_t n_samples,
                         const int32_t* n_rays_dev,
                         const float* d_sigma, float* grad_params, float* d_pts, float* d_rays,
                         int32_t reuse_features, int32_t flags, void* workspace, size_t workspace_bytes,
                         void* input_grad_event /* hipEvent_t, nullable: recorded on `stream` as soon as d_pts / d_rays are complete,
                                                   before the table-gradient reduce - the pose tail and the next batch's ray build and
                                                   sampling can then run on another stream beside the rest of this call */,
                         void* stream);

/* grad_params[0 : n_mlp_params] += (flags & LNR_BWD_OVERWRITE_GRAD: =) the weight-gradient slabs a lnr_density_backward call with
 * LNR_BWD_DEFER_WEIGHT_FOLD left in `workspace` (n_points: the n_points / n_rays * n_samples of that call).  Fixed summation order:
 * reproducible. */
int lnr_density_fold_weight_grads(const LnrNetSpec* spec /*host*/, int64_t n_points, float* grad_params,
                                  void* workspace, size_t workspace_bytes, int32_t flags, void* stream);

/* ---- rays ------------------------------------------------------------------------------------- */
/* LidarRayDirections.build_lidar_rays (ray_utils.py:269-322) + get_far_val (:31-60) for one
 * keyframe: gather, rotate, normalise, clip to the cube.  Writes ALL n_index candidates plus a
 * keep flag (the `far > near + 1/scale` test, :318-322).  transform: 12 floats = rows of [R|t]. */
int lnr_build_lidar_rays(const float* directions /*[3,n_points]*/, const float* distances /*[n_points]*/,
                         int64_t n_points, const int64_t* index /*[n_index]*/, int32_t n_index,
                         const float* transform /*[12]*/, float range_min, float range_max,
                         float scale, const float* shift /*host [3]*/,
                         float* rays /*[n_index,13]*/, float* depths /*[n_index]*/,
                         uint8_t* keep /*[n_index]*/, void* stream);

/* The same for a whole keyframe window in one launch (optimizer.py:285-340): segment s covers candidates
 * [seg_start[s], seg_start[s+1]) of keyframe pose row seg_pose[s]; distances[s] == NULL means the constant
 * const_distance[s] (sky rays, sensors.py:162-167).  index (device, concatenated) may be NULL: the indices are
 * then drawn in-kernel (the torch.randint of optimizer.py:288,301) and returned in index_out.  All per-segment
 * arrays are HOST arrays of length n_seg (seg_start: n_seg+1); transforms [n_poses,12] is on the device. */
int lnr_build_window_rays(const float* const* directions, const float* const* distances, const float* const_distance,
                          const int64_t* n_points, const int32_t* seg_start, const int32_t* seg_pose, int32_t n_seg,
                          const int64_t* index, int64_t* index_out, uint64_t seed, const float* transforms,
                          float range_min, float range_max, float scale, const float* shift /*host [3]*/,
                          float* rays, float* depths, uint8_t* keep, void* stream);

/* CameraRayDirections.build_rays (ray_utils.py:175-213) with get_far_val(no_nan=True) (:31-60) for one camera pose: one thread per
 * ray.  directions [n_pixels,3] are the camera-frame directions of get_ray_directions (:62-125), row-major over the image; index
 * (device int64 [n_rays], NULL: the pixels 0 .. n_rays-1 in order) names the pixel of each ray; transform: 12 floats = rows of the
 * camera-to-world [R|t], which is read, never written (the reference shifts its argument in place).  Record, every operation rounded
 * on its own in fp32: origin (t + shift) / scale (add, then divide); direction (R dir) / |R dir| with the products summed left to
 * right; view direction = -direction; columns 9, 10 = pixel x = index % width and y = index / width; near = range_min / scale; far =
 * the cube exit distance of lnr_build_lidar_rays (direction + 1e-15).  Unlike LiDAR rays, far is not capped by the sensor range and
 * no ray is dropped.  An index outside [0, n_pixels) gives a record of NaNs.  directions, index, transform and rays are device
 * pointers (the kernel reads the pose on the device); shift is a host array. */
int lnr_build_camera_rays(const float* directions /*device [n_pixels,3]*/, int64_t n_pixels, const int64_t* index /*device [n_rays] or NULL*/,
                          int32_t n_rays, int32_t width, const float* transform /*device [12]*/, float range_min, float scale,
                          const float* shift /*host [3]*/, float* rays /*[n_rays,13]*/, void* stream);

/* tensor_to_transform (pose_utils.py:288-302) for n poses: pose6 [n,6] = [t, axis-angle] -> transforms [n,12]
 * (rows of [R|t]); and its backward d_transforms [n,12] -> d_pose6 [n,6] (mask nullable: 0 = fixed pose;
 * accumulate != 0 adds to d_pose6). */
int lnr_pose_forward(const float* pose6, int32_t n, float* transforms, void* stream);
int lnr_pose_backward(const float* pose6, const float* d_transforms, const uint8_t* mask, int32_t n, float* d_pose6,
                      int32_t accumulate, int32_t* poison_dev, int32_t poison_tag, void* stream);

/* Order-preserving compaction of candidate rays by `keep` (the boolean indexing at
 * ray_utils.py:322 and the vstack at optimizer.py:333-338 for a whole window).
 * seg_start [n_seg+1] (host) delimits the keyframes inside the candidate arrays;
 * out_seg_start [n_seg+1] (device) receives the compacted segment starts; n_out_dev the total. */
int lnr_compact_rays(const float* rays_in, const float* depths_in, const uint8_t* keep, const int64_t* src_index,
                     int32_t n_in, const int32_t* seg_start /*host*/, int32_t n_seg,
                     float* rays_out, float* depths_out, int64_t* src_index_out,
                     int32_t* out_seg_start, int32_t* n_out_dev, void* stream);

/* lnr_compact_rays followed, in the same launch, by what the loss needs next from the compacted batch: counts_dev [2] = the normalisers
 * lnr_count_opaque computes ({#rays, #opaque rays}, optimizer.py:460-463,488-489; far[0] = the batch's own first ray), OR record = the
 * rank's front record as lnr_shard_front_pack writes it (seg_order [n_seg] host, cap depth slots >= n_in).  Exactly one of the two. */
int lnr_compact_rays_front(const float* rays_in, const float* depths_in, const uint8_t* keep, const int64_t* src_index,
                           int32_t n_in, const int32_t* seg_start /*host*/, int32_t n_seg,
                           float* rays_out, float* depths_out, int64_t* src_index_out,
                           int32_t* out_seg_start, int32_t* n_out_dev,
                           int32_t* counts_dev /*[2] or NULL*/, const int32_t* seg_order /*[n_seg] host or NULL*/, int32_t cap,
                           float* record /*[LNR_FRONT_HEADER + cap] or NULL*/, void* stream);

/* Sharded windows (one process per GPU, keyframes round-robin): the reference's `depth > far[0]` test (optimizer.py:460-461) uses the
 * FIRST ray of the whole batch = the first kept ray of the first keyframe, in window order, that kept any.  Each rank reports its
 * candidate as one 64-bit key = (seg_order of its first segment with a kept ray) << 32 | bits of that ray's far; INT64_MAX when it kept
 * none.  A MIN all-reduce over the ranks then leaves the batch's first ray's key everywhere (low word = far[0] as float bits).
 * rays / out_seg_start: the outputs of lnr_compact_rays; seg_order [n_seg] (host): ascending position of each segment in the window. */
int lnr_first_ray_key(const float* rays, const int32_t* out_seg_start /*[n_seg+1] device*/, const int32_t* seg_order /*[n_seg] host*/,
                      int32_t n_seg, int64_t* key_out /*[1] device*/, void* stream);

/* The sharded loop's one small collective per iteration (loner_amd/mapping/sharding.py; SURVEY 8e collectives (2) + the far[0] quirk).
 * far[0] of the whole batch and the global normalisers #rays / #opaque rays (optimizer.py:460-463,488-489,569-578) - the second of
 * which depends on far[0] - come out of ONE all-gather of per-rank "front records" instead of a key exchange followed by a count
 * exchange.  A record is LNR_FRONT_HEADER + cap float32 words: [0..1] the rank's first-ray key as lnr_first_ray_key defines it (int64
 * bits), [2] its live-ray count (int32 bits), [3] 0, [4..] the ground-truth depths of its kept rays (zeros beyond the count).
 * lnr_shard_front_pack writes a rank's record from the outputs of lnr_compact_rays (n_seg = 0: a rank without keyframes - the key is
 * INT64_MAX, the count 0, every pointer but `record` may be NULL).  lnr_shard_front_reduce reads the `world` gathered records
 * (consecutive, `stride` = LNR_FRONT_HEADER + cap words each) and writes counts_dev = {sum of the live counts, number of depths d over
 * all ranks with d > 0 and not d > far[0]} - the values lnr_count_opaque computes for an unsharded batch - and far0_dev = far[0] (NaN
 * bits when no rank kept a ray), for lnr_los_loss_fused / lnr_occ_grid_step. */
#define LNR_FRONT_HEADER 4
int lnr_shard_front_pack(const float* rays, const int32_t* out_seg_start /*[n_seg+1] device*/, const int32_t* seg_order /*[n_seg] host*/,
                         int32_t n_seg, const float* depths, int32_t n_rays, const int32_t* n_rays_dev, int32_t cap,
                         float* record /*[LNR_FRONT_HEADER + cap] device*/, void* stream);
int lnr_shard_front_reduce(const float* records /*[world][stride] device*/, int32_t world, int32_t stride,
                           int32_t* counts_dev /*[2]*/, float* far0_dev /*[1]*/, void* stream);

/* ---- the sharded loop's collectives: RCCL on the caller's stream (csrc/lnr_comm.hip) -------------------------------------------
 * The reference has no multi-GPU mapping (its only fan-out is independent trials, examples/run_loner.py:339-424); SURVEY.md 8e
 * defines the keyframe-sharded window these calls serve.  One communicator per rank and process: rank 0 makes an id
 * (lnr_comm_unique_id), hands its LNR_COMM_ID_BYTES bytes to the other ranks by any means (the Python layer: the torch.distributed
 * store), every rank calls lnr_comm_init on its HIP device (collective: returns when all have).  A collective is ONE enqueue on
 * `stream` - ordered with the kernels before and after it on that stream, no host synchronisation, capturable into a hipGraph.
 * librccl.so.1 is loaded on first use (dlopen); lnr_comm_available() = 0 when it is not there. */
#define LNR_COMM_ID_BYTES 128
typedef enum LnrCommDtype { LNR_COMM_F32 = 0, LNR_COMM_BF16 = 1, LNR_COMM_I64 = 2, LNR_COMM_I32 = 3, LNR_COMM_U8 = 4 } LnrCommDtype;
typedef enum LnrCommOp { LNR_COMM_SUM = 0, LNR_COMM_MIN = 1, LNR_COMM_MAX = 2 } LnrCommOp;
int lnr_comm_available(void);
int lnr_comm_unique_id(void* id /*[LNR_COMM_ID_BYTES] host*/, size_t id_bytes);
int lnr_comm_init(const void* id, size_t id_bytes, int32_t rank, int32_t world, void** comm_out);
int lnr_comm_destroy(void* comm);
/* in place; the gradient all-reduce (optimizer.py:366's loss.backward() summed over the shards), the occupancy pseudo-gradient (I64), the failure word (MIN) */
int lnr_comm_all_reduce(void* comm, void* buf, size_t count, int32_t dtype /*LnrCommDtype*/, int32_t op /*LnrCommOp*/, void* stream);
/* recv [recv_count] = sum over ranks of send[rank * recv_count ...]: a rank's chunk of the flat gradient */
int lnr_comm_reduce_scatter(void* comm, const void* send, void* recv, size_t recv_count, int32_t dtype, void* stream);
/* recv [world * bytes_per_rank]; send may be the rank's own slot of recv (in place): front records, stepped parameter chunks */
int lnr_comm_all_gather(void* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
int lnr_comm_broadcast(void* comm, void* buf, size_t bytes, int32_t root, void* stream);

/* Backward of lnr_build_lidar_rays for a window: dL/drays -> dL/d[R|t] per keyframe
 * (the autograd tail ray_utils.py:281-305 <- keyframe.py:80-88).  d_transform [n_seg,12]. */
int lnr_lidar_rays_backward(const float* d_rays /*[n,13]*/, const float* rays /*[n,13]*/,
                            const int64_t* src_index /*[n]*/, const int32_t* seg_start /*device [n_seg+1]*/,
                            int32_t n_seg, const float* const* directions /*host array of n_seg device ptrs*/,
                            const int64_t* n_points /*host [n_seg]*/, const float* transforms /*[n_seg,12]*/,
                            float scale, float* d_transform /*[n_seg,12]*/, void* stream);

/* ---- samplers ---------------------------------------------------------------------------------- */
/* OccupancyGridModel.interpolate (model_tcnn.py:122-131): trilinear lookup, zero padding. */
int lnr_occ_interpolate(const float* grid /*[V,V,V] z,y,x*/, int32_t V, const float* pts /*[n,3]*/,
                        int64_t n, float* out /*[n]*/, void* stream);

/* OccGridRaySampler.get_samples (ray_sampling.py:53-92) incl. sample_pdf (rendering_tcnn.py:18-67).
 * steps: torch.linspace(0,1,n_samples/2) as a device table.  u_jitter/u_pdf [n_rays,n_samples/2]:
 * the two torch.rand draws; either may be NULL, then a counter-based generator keyed by
 * (seed, ray, sample) is used.  dbg_inds/dbg_probs/dbg_cdf (nullable) expose the searchsorted
 * indices, point_probs and cdf for stage-wise parity tests. */
int lnr_sample_rays_occ(const float* rays, int32_t n_rays, const int32_t* n_rays_dev,
                        const float* grid, int32_t V, int32_t n_samples, float perturb,
                        const float* steps, const float* u_jitter, const float* u_pdf, uint64_t seed,
                        float* z_out /*[n_rays,n_samples] sorted*/,
                        int64_t* dbg_inds, float* dbg_probs, float* dbg_cdf, void* stream);

/* UniformRaySampler.get_samples (ray_sampling.py:22-43). steps: linspace(0,1,n_samples). */
int lnr_sample_rays_uniform(const float* rays, int32_t n_rays, const int32_t* n_rays_dev,
                            int32_t n_samples, float perturb, const float* steps,
                            const float* u_jitter, uint64_t seed, float* z_out, void* stream);

/* The random numbers the kernels draw when the caller passes no random tensors, as tensors (diagnostics: distribution tests, and
 * the proof that a seeded call equals the same call with these draws handed in).  The reference draws, per forward,
 * torch.rand [n_rays, n_samples/2] twice (ray_sampling.py:72, rendering_tcnn.py:48) and torch.randn [n_rays, n_samples] once
 * (rendering_tcnn.py:104); per keyframe torch.randint (optimizer.py:288).
 *   which = LNR_DRAW_JITTER / LNR_DRAW_PDF: the uniforms in [0,1) that lnr_sample_rays_* use for element [ray][j] under `seed`;
 *   which = LNR_DRAW_NOISE: the N(0,1) values that lnr_render_* / lnr_los_loss_fused add (x noise_std) to sigma [ray][i] under `seed`;
 *   which = LNR_DRAW_RAY_INDEX + segment: the uniforms behind the ray indices lnr_build_window_rays draws for that segment
 *           (out [n_rays * n_per_ray] in draw order: index = min(floor(u * n_points), n_points - 1)). */
#define LNR_DRAW_JITTER 0
#define LNR_DRAW_PDF 1
#define LNR_DRAW_NOISE 2
#define LNR_DRAW_RAY_INDEX 16
int lnr_rng_draws(int32_t which, uint64_t seed, int32_t n_rays, int32_t n_per_ray, float* out /*[n_rays,n_per_ray]*/, void* stream);

/* ---- volume rendering ---------------------------------------------------------------------------- */
/* raw2outputs(sigma_only=True, far, ret_var=True) (rendering_tcnn.py:71-147).
 * noise [n_rays,n_samples] = randn*raw_noise_std (rendering_tcnn.py:104) or NULL with
 * noise_std>0 for the in-kernel generator (noise_std==0: no noise).  Outputs nullable. */
int lnr_render_forward(const float* sigma, const float* z, const float* rays, int32_t n_rays,
                       const int32_t* n_rays_dev, int32_t n_samples,
                       const float* noise, float noise_std, uint64_t seed,
                       float* depth, float* weights, float* opacity, float* variance, void* stream);

/* lnr_render_forward without the [n_rays,n_samples] weights, plus the ray's peak: what the depth renderer reads from
 * weights_fine / samples_fine (analysis/renderer.py:195-198: samples_fine[argmax(weights_fine)]).  depth, opacity and variance are
 * lnr_render_forward's bit for bit (same arithmetic, same noise draws).  peak_index (int32) is the sample of maximal weight with
 * torch.argmax's rules - on equal weights the lowest index, a NaN weight counts as maximal and the lowest NaN wins - and peak_z is
 * z[ray][peak_index], copied, not computed.  Outputs nullable. */
int lnr_render_forward_peak(const float* sigma, const float* z, const float* rays, int32_t n_rays,
                            const int32_t* n_rays_dev, int32_t n_samples,
                            const float* noise, float noise_std, uint64_t seed,
                            float* depth, float* opacity, float* variance, float* peak_z, int32_t* peak_index, void* stream);

/* save_depth (analysis/render_utils.py:116-127) per element, values [n] fp32 -> rgba [n,4] uint8 (4-byte aligned):
 *   v = values * multiplier (fp32; the world cube's scale for raw depths, 1 for metres); NaN -> (0,0,0,0), matplotlib's "bad" colour;
 *   v >= (float) max_depth -> (0,0,0,255), the reference's mask; otherwise c = clip(v, (float) min_depth, (float) max_depth),
 *   x = clip((c - (float) min_depth) / (float)(max_depth - min_depth), 0, 1) (the span subtracted in fp64 and rounded once, as Python
 *   does before torch sees it; subtract and divide rounded on their own in fp32), k = min(floor(256 x), 255) - matplotlib's index
 *   rule - and the pixel is (table[3k], table[3k+1], table[3k+2], 255).  table: device uint8 [256,3], the colour map already
 *   truncated to uint8 ((lut * 255).astype(uint8), the reference's last step). */
int lnr_depth_colormap(const float* values, int64_t n, float multiplier, double min_depth, double max_depth,
                       const uint8_t* table /*[256,3]*/, uint8_t* rgba /*[n,4]*/, void* stream);

/* Backward of lnr_render_forward for arbitrary upstream gradients (nullable each):
 * g_depth[n], g_weights[n,S], g_opacity[n], g_variance[n]  ->  d_sigma [n,S] and the direct
 * ray-record contribution d_rays [n,13] (cols 3:6 through |dir|, col 12 = far); d_rays is
 * OVERWRITTEN.  Points' contribution to cols 0:6 is added by lnr_points_grad_to_rays. */
int lnr_render_backward(const float* sigma, const float* z, const float* rays, int32_t n_rays,
                        const int32_t* n_rays_dev, int32_t n_samples,
                        const float* noise, float noise_std, uint64_t seed,
                        const float* g_depth, const float* g_weights, const float* g_opacity,
                        const float* g_variance, float* d_sigma, float* d_rays, void* stream);

/* xyz = o + d*z  =>  d_rays[:,0:3] += sum_s d_pts ; d_rays[:,3:6] += sum_s z*d_pts
 * (rendering_tcnn.py:241 backward). */
int lnr_points_grad_to_rays(const float* d_pts /*[n,S,3]*/, const float* z, int32_t n_rays,
                            const int32_t* n_rays_dev, int32_t n_samples, float* d_rays, void* stream);

/* ---- meshing (analysis/mesher.py:103-225) ---------------------------------------------------------- */
/* The lattice of Mesher.get_grid_uniform: n[a] nodes per axis (x, y, z), the np.linspace axes as doubles on the device, the fp32
 * bounds of the reference's bound check (a 0-dim fp64 tensor does not promote fp32 points: the bound is rounded to fp32 and compared
 * in fp32) and, for the bucket search, the first node and 1 / spacing of each axis (a guess only: the bucket is then corrected
 * against the axis values themselves). */
typedef struct LnrMeshGrid {
    int32_t n[3];
    float lo[3], hi[3];
    double first[3], inv_step[3];
    const double* axis[3];
} LnrMeshGrid;

/* Compositing (the arithmetic and noise draws of lnr_render_forward: the same weights, depth and variance bit for bit) fused with the reference's weight volume (mesher.py:143-180),
 * without writing weights, depths or points.  A ray counts when depth < depth_max (the rendered depth in world-cube units against
 * ray_range[1] - 0.25 in metres: the reference's comparison, kept) and, with use_var != 0, variance < var_max.  Each of its samples
 * with w > 0 is placed at o + d z (fp32 multiply, then fp32 add), kept when lo <= p <= hi on every axis (fp32), bucketed per axis as
 * torch.bucketize against the fp64 axis (smallest i with (double) p <= axis[i]) and lands at flat index x_b nz + y_b nx nz + z_b (the
 * reference's [y][x][z] order; indices >= nx ny nz are dropped, smaller ones - also those of bucket n on an axis - are kept).
 * volume [ny*nx*nz] fp32 receives the max of the weights (integer max on the bit patterns: weights are >= 0); the caller zeroes it.
 * counters (nullable, uint64 [2]) += {samples that reached the volume, atomics issued}. */
int lnr_render_mesh_accumulate(const float* sigma, const float* z, const float* rays, int32_t n_rays, const int32_t* n_rays_dev,
                               int32_t n_samples, const float* noise, float noise_std, uint64_t seed, const LnrMeshGrid* grid,
                               float depth_max, int32_t use_var, float var_max, float* volume, uint64_t* counters, void* stream);

/* Marching cubes over volume [nx][ny][nz] fp32 (all >= 2, nx ny nz < 2^31).  A node is inside when v > level.  A vertex lies on
 * every lattice edge whose ends differ, owned by the edge's lower node, at t = (level - va) / (vb - va) from it (va at the lower
 * node); its coordinate along the edge is ((float) index + t) * spacing + origin, the others (float) index * spacing + origin, each
 * operation rounded on its own in fp32.  Vertex ids follow node order, then axis (x, y, z); triangles follow cell order (a cell is
 * named by its lower node), then the case table's order.  The case table (256 x LNR_MC_TABLE_WIDTH int8, edge ids, -1 after the
 * last triangle; edge e = 4 a + q lies along axis a from the q-th corner with bit a clear, corners numbered x + 2 y + 4 z) is
 * generated from one rule: on a face with its two inside corners diagonal they are separated.  Triangles face lower values.
 * Two calls: the count pass (per-block vertex and triangle counts, then their exclusive scan; totals_dev uint64 [2] = {V, F}),
 * then, with the totals read back, the emit pass: verts [V,3] fp32, tris [F,3] int32 (V < 2^30).  lnr_mc_workspace: bytes of the
 * workspace both calls share. */
#define LNR_MC_TABLE_WIDTH 16
size_t lnr_mc_workspace(int32_t nx, int32_t ny, int32_t nz);
int lnr_mc_count(const float* volume, int32_t nx, int32_t ny, int32_t nz, float level, void* workspace, size_t workspace_bytes,
                 uint64_t* totals_dev, void* stream);
int lnr_mc_emit(const float* volume, int32_t nx, int32_t ny, int32_t nz, float level, const float* spacing /*host [3]*/,
                const float* origin /*host [3]*/, void* workspace, size_t workspace_bytes, int64_t n_verts, int64_t n_tris,
                float* verts, int32_t* tris, void* stream);
/* host only: the case table, out [256 * LNR_MC_TABLE_WIDTH] */
int lnr_mc_case_table(int8_t* out);
/* The same pair over the observed part of a volume: valid uint8 [nx][ny][nz], a node counts as valid when its byte is not 0.  A
 * lattice edge carries a vertex only when both its ends are valid and differ; a cell emits its case's triangles only when all eight
 * corners are valid (the rule of scikit-image's `mask`).  Vertex and triangle order, the arithmetic, the workspace and the two-call
 * protocol are those above; with every node valid the outputs are the unmasked pair's byte for byte.  A vertex on an edge whose
 * four cells all lost a corner is emitted and used by no triangle (lnr_mesh_select drops such vertices), so V > 0 with F = 0 is
 * possible: tris may then be NULL. */
int lnr_mc_count_masked(const float* volume, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz, float level, void* workspace,
                        size_t workspace_bytes, uint64_t* totals_dev, void* stream);
int lnr_mc_emit_masked(const float* volume, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz, float level,
                       const float* spacing /*host [3]*/, const float* origin /*host [3]*/, void* workspace, size_t workspace_bytes,
                       int64_t n_verts, int64_t n_tris, float* verts, int32_t* tris, void* stream);

/* ---- point clouds (analysis/renderer_lidar.py:71-91, :296-349; analysis/evaluate_lidar_map.py:16-98) ----------------------- */
/* Points are fp64 [n,3] (x y z per point), n <= 2^31 - 4096 per call (LNR_ERR_INVALID_ARG beyond).  Every fp64 expression rounds
 * operation by operation (no fma), divides and square roots are IEEE.  Calls that sort take a caller-owned workspace of
 * lnr_cloud_workspace(n) bytes (about 36 n: keys, indices and scan space for n points; 0 = n out of range). */
size_t lnr_cloud_workspace(int64_t n_points);

/* Scan points of one rendered pose (renderer_lidar.py:83-91).  Ray i (i < n_rays) was rendered with depth[i] and variance[i]
 * (Model.forward(testing=True, return_variance=True)) along scan direction ray_index[i] (directions: the scan's [3, n_directions]
 * fp32 sensor-frame directions).  With d = fp32(depth * scale) and v = fp32(variance * scale) it is kept when v < var_max and
 * d < depth_max (fp32 compares: NaN is dropped); its point is fp32(dir_a * d) per axis, widened to fp64.  points [n_rays,3]
 * receives the kept points in ray order, n_points_dev (int32 [1]) their count; the count stays on the device. */
int lnr_lidar_scan_points(const float* depth, const float* variance, const int64_t* ray_index, int64_t n_rays,
                          const float* directions, int64_t n_directions, float scale, float var_max, float depth_max,
                          void* workspace, size_t workspace_bytes, double* points, int32_t* n_points_dev, void* stream);

/* open3d's legacy PointCloud::VoxelDownSample (as called by renderer_lidar.py:342,348 and evaluate_lidar_map.py:20-21), with a
 * defined order.  n_points_dev (nullable): the live count (<= n_points) is read on the device.  voxel_size finite and > 0.
 * lo = min - 0.5 v and hi = max + 0.5 v per axis; v * INT_MAX < max_a(hi_a - lo_a) is open3d's "voxel_size is too small".  A point's
 * voxel is floor((p_a - lo_a) / v) per axis; the key packs the three indices with ceil(log2(voxels on the axis)) bits each (x highest,
 * z lowest), at most 64 bits in all.  Each occupied voxel gives one point, the fp64 sum of its points in input order divided by
 * (double) count; out [n_points,3] receives them in ascending (i_x, i_y, i_z) order.
 * info_dev int64 [8], written by the call: {status, points out, non-finite input points, key bits, edge (fp64 bits), voxels on x, y, z};
 * status bit 1: non-finite input (nothing is written), 2: voxel_size too small, 4: key wider than 64 bits.  One host read of info_dev
 * gives the outcome and the output count. */
int lnr_voxel_down_sample(const double* points, int64_t n_points, const int32_t* n_points_dev, double voxel_size,
                          void* workspace, size_t workspace_bytes, double* out, int64_t* info_dev, void* stream);

/* open3d's PointCloud::Transform with an affine T (renderer_lidar.py:304,341): transform host [12] fp64, the top three rows of T
 * (row-major); dst_i = ((T_i0 x + T_i1 y) + T_i2 z) + T_i3 for each row i.  dst may equal src (in place) or be the tail of a merged
 * cloud (the append of merge_o3d_pc, renderer_lidar.py:61-67). */
int lnr_cloud_append_transformed(const double* src, int64_t n_points, const double* transform, double* dst, void* stream);

/* The search structure of compute_point_cloud_distance (evaluate_lidar_map.py:59-60: open3d's KDTreeFlann over the target cloud):
 * a grid of cubic cells over the targets, origin at their minimum, the targets sorted by cell.  cell_edge <= 0: the default
 * edge cbrt(e_x e_y e_z / n) with every extent e_a raised to at least 2^-10 of the largest (1 when all targets coincide).  The edge
 * is doubled until the key fits 63 bits; the distances do not depend on it.  grid: lnr_nn_grid_bytes(n) bytes, kept by the caller
 * for any number of lnr_nn_distance calls.  info_dev int64 [8] as lnr_voxel_down_sample's ({status, occupied cells, non-finite
 * targets, key bits, edge, cells on x, y, z}); status bit 1: a non-finite target (the grid is unusable). */
size_t lnr_nn_grid_bytes(int64_t n_targets);
int lnr_nn_grid_build(const double* targets, int64_t n_targets, double cell_edge, void* workspace, size_t workspace_bytes,
                      void* grid, size_t grid_bytes, int64_t* info_dev, void* stream);

/* PointCloud::ComputePointCloudDistance: for every query the distance to its nearest target, exactly.  d2 = (dx*dx + dy*dy) + dz*dz
 * (d = q - t per axis), minimised over all targets; distance = sqrt(d2) (correctly rounded); sq_distance (nullable) receives d2.  With
 * no target every distance is 0 (open3d: SearchKNN finds nothing).  A query visits Chebyshev shells of cells around its own and stops
 * once its best d2 lies below a rounding-safe lower bound on every unvisited cell; queries still open after 5 shells take an exact
 * pass over all targets.  A non-finite query gets NaN.  workspace: lnr_cloud_workspace(n_queries) bytes.
 * counters_dev int64 [4], written by the call: {queries that took the exact pass, non-finite queries, shells visited, 0}. */
int lnr_nn_distance(const void* grid, int64_t n_targets, const double* queries, int64_t n_queries, double* distance,
                    double* sq_distance, void* workspace, size_t workspace_bytes, int64_t* counters_dev, void* stream);

/* ---- normals and point-to-plane ICP (analysis/evaluate_lidar_map.py:23-53) ----------------------------------------------------- */
#define LNR_KNN_MAX 32          /* the largest knn of lnr_cloud_normals */
#define LNR_ICP_RESULT 64       /* fp64 entries of lnr_icp_point_to_plane's result */

/* open3d's PointCloud::EstimateNormals(KDTreeSearchParamKNN(knn)) (evaluate_lidar_map.py:36-37) over the points a grid was built from
 * (lnr_nn_grid_build, any cell edge: the results do not depend on it).  Neighbours of point i: the min(knn, n) smallest
 * (d2, input index) pairs over all points, i itself included, d2 as lnr_nn_distance's (the lower input index wins a tie), found by the
 * same shell walk with the k-th best in the stop rule and the same exact pass for points still open after 5 shells.  Covariance (fp64,
 * no fma): with m >= 3 neighbours, the cumulants sum_x .. sum_zz summed in neighbour order, each divided by (double) m, then
 * C_ab = m_ab - m_a m_b; with fewer, the identity.  Normal: the unit eigenvector of C's smallest eigenvalue by open3d's FastEigen3x3
 * (C scaled by its largest entry, trigonometric roots, eigenvectors from cross products of rows); its sign is free.  C with zero
 * off-diagonals gives (1,0,0) if C00 < C11 and C00 < C22, else (0,1,0) if C11 < C00 and C11 < C22, else (0,0,1); an all-zero C gives
 * (0,0,1).  normals [n,3] and covariances [n,3,3] (nullable, row-major) in input order.  workspace: lnr_cloud_workspace(n) bytes.
 * counters_dev int64 [4], written by the call: {points that took the exact pass, 1 if the grid is unusable (a non-finite point, or
 * another n), shells visited, 0}. */
int lnr_cloud_normals(const void* grid, int64_t n_points, int32_t knn, double* normals, double* covariances, void* workspace,
                      size_t workspace_bytes, int64_t* counters_dev, void* stream);

/* GetRegistrationResultAndCorrespondences' search (open3d KDTreeFlann::SearchHybrid(r, 1)): for every query the target with the
 * smallest (d2, index) among those with d2 < r*r (strict), found on the grid within ceil(r / edge) + 1 shells.  index int32 [n]
 * (the target's input index, -1 for none) and sq_distance [n] (d2; +inf for none, NaN for a non-finite query).  counters_dev int64
 * [4]: {0, non-finite queries, 0, 0}. */
int lnr_icp_correspondences(const void* grid, int64_t n_targets, const double* queries, int64_t n_queries, double max_distance,
                            int32_t* index, double* sq_distance, int64_t* counters_dev, void* stream);

/* open3d's RegistrationICP with TransformationEstimationPointToPlane (evaluate_lidar_map.py:44-48).  grid: over the n_targets targets,
 * target_normals [n_targets,3] in their input order; source [n_source,3]; init host [16] (row-major 4x4, bottom row 0 0 0 1).
 * The source is copied and transformed by init (lnr_cloud_append_transformed's rounding); correspondences are taken once
 * (lnr_icp_correspondences' rule), then up to max_iteration rounds: the update, transformation = update @ transformation (each entry
 * ((a0 b0 + a1 b1) + a2 b2) + a3 b3), the copy transformed by update, correspondences again; the loop stops after a round with
 * |d fitness| < relative_fitness and |d rmse| < relative_rmse.  fitness = n_corr / n_source and inlier_rmse = sqrt(sum d2 / n_corr),
 * both 0 without a correspondence.  The update: per correspondence (s, t, n) r = (s - t).n and J = [s x n, n]; JTJ = sum J J^T and
 * JTr = sum J r over the correspondences in source order per thread, per-block partials and one workgroup's fold, all in a fixed order
 * (bit-identical from run to run); x = LDLT(JTJ).solve(-JTr) as Eigen's (pivoting on the largest remaining |diagonal|, a zero
 * component where |D_i| <= DBL_MIN); update = [Rz(x2) Ry(x1) Rx(x0) | x3..x5]; no correspondence gives the identity.  Every round is
 * enqueued without a host read; rounds after convergence return at once.  workspace: lnr_icp_workspace(n_source) bytes.
 * result_dev fp64 [LNR_ICP_RESULT]: [0:16] transformation, [16] fitness, [17] inlier_rmse, [18:39] the last solved JTJ (upper
 * triangle, row by row), [39:45] its JTr, [45] its sum of d2, [46:52] its x.  info_dev int64 [8]: {status, correspondences, rounds
 * run, non-finite source points, correspondences whose target normal is non-finite, correspondences of the last solved system,
 * converged or stopped, 0 (lnr_icp_generalized: correspondences skipped)}; status bit 1: a non-finite source point, 2: the grid is unusable (a non-finite target, or another
 * n_targets), 4: a non-finite target normal, 8: a non-finite update (the transformation keeps its last finite value). */
size_t lnr_icp_workspace(int64_t n_source);
int lnr_icp_point_to_plane(const void* grid, int64_t n_targets, const double* target_normals, const double* source, int64_t n_source,
                           double max_distance, const double* init, double relative_fitness, double relative_rmse, int32_t max_iteration,
                           void* workspace, size_t workspace_bytes, double* result_dev, int64_t* info_dev, void* stream);

/* ---- robust kernels and generalized ICP (open3d's RobustKernel family and registration_generalized_icp; Segal et al., ------------
 *      "Generalized-ICP", RSS 2009) ---------------------------------------------------------------------------------------------- */
/* Robust kernels: the weight w(m) of a residual of magnitude m >= 0 with the scale k (finite and > 0 unless the kernel is L2), fp64:
 *   LNR_ROBUST_L2      w = 1 (no weight is evaluated: the terms are summed as they are)
 *   LNR_ROBUST_HUBER   w = k / max(m, k)
 *   LNR_ROBUST_CAUCHY  q = m / k, w = 1 / (1 + q q)
 *   LNR_ROBUST_TUKEY   q = m / k, u = 1 - q q, w = u u for m <= k, else 0
 * A weighted sum adds w * term, the term formed first. */
#define LNR_ROBUST_L2 0
#define LNR_ROBUST_HUBER 1
#define LNR_ROBUST_CAUCHY 2
#define LNR_ROBUST_TUKEY 3

/* lnr_icp_point_to_plane with the weight w(|r|) on every correspondence's JTJ and JTr terms (the 21 products J_a J_b and the 6
 * products J_a r); fitness, inlier_rmse and the count are not weighted.  With LNR_ROBUST_L2 it runs lnr_icp_point_to_plane's own
 * kernels and returns its bytes.  Everything else, the result and the info words included, is lnr_icp_point_to_plane's. */
int lnr_icp_point_to_plane_robust(const void* grid, int64_t n_targets, const double* target_normals, const double* source,
                                  int64_t n_source, double max_distance, const double* init, double relative_fitness,
                                  double relative_rmse, int32_t max_iteration, int32_t kernel, double kernel_k, void* workspace,
                                  size_t workspace_bytes, double* result_dev, int64_t* info_dev, void* stream);

/* The covariance of a point on a plane with the unit normal n: C_ab = delta_ab - ((1 - epsilon) n_a) n_b for a <= b, mirrored below
 * the diagonal; open3d's Rx diag(epsilon, 1, 1) Rx^T written without the rotation, so it does not depend on the sign of n.  A
 * non-finite normal gives a covariance with non-finite entries.  normals [n,3] -> covariances [n,3,3]; epsilon finite and > 0. */
int lnr_cloud_plane_covariances(const double* normals, int64_t n, double epsilon, double* covariances, void* stream);

/* open3d's RegistrationGeneralizedICP (plane to plane).  Correspondences, fitness, inlier_rmse, the convergence test, the LDLT solve,
 * the update and its composition, the fixed-order sums, the workspace, result_dev and info_dev are lnr_icp_point_to_plane's; only the
 * system differs.  target_covariances [n_targets,3,3] in the targets' input order and source_covariances [n_source,3,3] as the
 * caller has them for the untransformed source; of each only the upper triangle is read.  Per correspondence (s, t) of a round, with
 * R the rotation block of the accumulated transformation (init before the first round; the source's covariances are rotated from
 * their given values every round, so rounding does not compound), fp64 without fma:
 *   B = R C_s, B_ab = (R_a0 S_0b + R_a1 S_1b) + R_a2 S_2b;   M_ab = T_ab + ((B_a0 R_b0 + B_a1 R_b1) + B_a2 R_b2) for a <= b
 *   cofactors c00 = m11 m22 - m12 m12, c01 = m02 m12 - m01 m22, c02 = m01 m12 - m02 m11, c11 = m00 m22 - m02 m02,
 *   c12 = m01 m02 - m00 m12, c22 = m00 m11 - m01 m01;  det = (m00 c00 + m01 c01) + m02 c02;  W_ab = c_ab / det
 *   d = s - t;  (W d)_a = (W_a0 d0 + W_a1 d1) + W_a2 d2;  m = sqrt(max((d0 (Wd)_0 + d1 (Wd)_1) + d2 (Wd)_2, 0)), the Mahalanobis residual
 *   J = [-[s]x | I] (3x6);  G = W [-[s]x], row a of G = s x (row a of W);  H = [s]x G, column b of H = s x (column b of G)
 *   JTJ += w(m) [H G^T; G W] (its upper triangle, row by row: H_aa.. H_a2, G_0a, G_1a, G_2a for a < 3, then W's)
 *   JTr += w(m) [s x (W d); W d]
 * These are open3d's normal equations without the matrix square root of M^-1 (J^T sqrt(W) sqrt(W) J = J^T W J: with L2 the same
 * least-squares problem).  Stated difference: the robust weight is taken once per correspondence on m, not once per whitened row, so
 * it does not depend on the frame.  A correspondence whose M has a non-finite entry or whose det is not > 0 is skipped and counted:
 * status bit 16, and info_dev[7] holds the count (0 from the point-to-plane entry points); like the other data bits it ends the
 * call with the transformation at its last value. */
int lnr_icp_generalized(const void* grid, int64_t n_targets, const double* target_covariances, const double* source,
                        const double* source_covariances, int64_t n_source, double max_distance, const double* init,
                        double relative_fitness, double relative_rmse, int32_t max_iteration, int32_t kernel, double kernel_k,
                        void* workspace, size_t workspace_bytes, double* result_dev, int64_t* info_dev, void* stream);

/* ---- global registration (open3d's compute_fpfh_feature, registration_ransac_based_on_feature_matching and ----------------------
 *      registration_ransac_based_on_correspondence; Rusu et al., "Fast Point Feature Histograms (FPFH) for 3D Registration", ICRA 2009)
 * A starting pose for the ICP entry points above, from two clouds alone.  Everything is fp64 without fma and rounds operation by
 * operation; dot(a, b) = (a0 b0 + a1 b1) + a2 b2, cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), |a| = sqrt(dot(a, a)),
 * d2 as lnr_nn_distance's.  Two runs give the same bytes: no float atomics, no hand-over between workgroups inside a launch. */
#define LNR_ORIENT_LOCATION 0
#define LNR_ORIENT_DIRECTION 1
#define LNR_FPFH_DIM 33
#define LNR_FEATURE_DIM_MAX 64
#define LNR_RANSAC_CHUNK 2048
#define LNR_STREAM_RANSAC 0x524E534300000000ull   /* "RNSC" in the top word of the Philox counter's high half */

/* open3d's OrientNormalsTowardsCameraLocation / OrientNormalsToAlignWithDirection, in place on normals [n,3].  reference host [3],
 * finite.  LNR_ORIENT_LOCATION: with v_a = reference_a - p_i,a per axis, n_i is negated (each component) when dot(v, n_i) < 0;
 * LNR_ORIENT_DIRECTION (points may be null): when dot(n_i, reference) < 0.  A zero or NaN dot product leaves the normal (open3d
 * replaces a zero normal by the direction; this entry does not).  A normal with a non-finite component is left as it is and counted.
 * counters_dev int64 [4], written by the call: {non-finite normals, normals flipped, 0, 0}. */
int lnr_cloud_orient_normals(const double* points, int64_t n_points, double* normals, int32_t mode, const double* reference,
                             int64_t* counters_dev, void* stream);

/* The 20 literals of the FPFH angle bins: out[2 (b - 1)] = cos(theta_b), out[2 (b - 1) + 1] = sin(theta_b) with
 * theta_b = -pi + 2 pi b / 11 for b = 1..10.  Host only. */
int lnr_fpfh_bin_edges(double* out);

/* open3d's ComputeFPFHFeature with KDTreeSearchParamHybrid(radius, max_nn) over the points a grid was built from (lnr_nn_grid_build),
 * normals [n,3] in their input order; max_nn in [2, LNR_KNN_MAX] (open3d's default of 100 is out of range by intent: the neighbour
 * list stays in registers), radius finite and > 0.  features fp64 [n, LNR_FPFH_DIM], row i = point i.
 * Neighbours of i: of the min(max_nn, n) smallest (d2, input index) pairs of lnr_cloud_normals' search (the same shell walk, the same
 * exact pass after 5 shells) those with d2 < radius * radius (strict, the product rounded once), less the entry whose index is i;
 * m is their count, their order the list's.  (With more than max_nn exact duplicates before i the list does not hold i and m can
 * reach max_nn.)
 * Pair feature of (p1, n1) = point i and (p2, n2) = a neighbour: d = p2 - p1 per axis, f3 = |d|; a1 = dot(n1, d) / f3,
 * a2 = dot(n2, d) / f3; if |a1| < |a2| the two normals are swapped, d is negated and f2 = -a2, else f2 = a1; v = cross(d, n1), each
 * component divided by |v|; w = cross(n1, v); f1 = dot(v, n2); y = dot(w, n2), x = dot(n1, n2).  If f3 = 0 or |v| = 0, or either
 * normal has a non-finite component, the pair counts as f1 = f2 = 0 and x = y = 0.
 * Bins, 11 per feature: f1 and f2 go to floor(11 * ((f + 1) * 0.5)) clamped to [0, 10] (NaN: 0).  The angle atan2(y, x) is binned
 * without libm, with (c_b, s_b) of lnr_fpfh_bin_edges: x = y = 0 gives 5; y < 0 gives the count of b in 1..5 with
 * y * c_b - x * s_b >= 0; otherwise 5 + the count of b in 6..10 with y * c_b - x * s_b >= 0.  (This is floor(11 (atan2(y, x) + pi) /
 * (2 pi)) clamped to 10 wherever the angle is not within rounding of an edge.)
 * SPFH of i, open3d's row order: rows 0..10 the angle, 11..21 f1, 22..32 f2; each bin is (double) count * (100.0 / (double) m), all
 * zero when m = 0.  Stated difference: open3d adds 100 / m once per neighbour.
 * FPFH of i: acc_j and sum_b start at 0.0; over the neighbours k in list order with d2_k != 0 and then j = 0..32,
 * val = spfh_k,j / d2_k, acc_j = acc_j + val, sum_{j / 11} = sum_{j / 11} + val; feature_j = acc_j * (100.0 / sum_{j / 11}) + spfh_i,j,
 * and acc_j + spfh_i,j where the sum is 0.  An exact duplicate counts in m and is skipped in the weighting.
 * A point whose own normal is not finite is counted; its pairs, and every pair that reads such a normal, are the zero pair above, so
 * every feature stays finite.  workspace: lnr_cloud_fpfh_workspace(n) bytes (about 660 n; 0 = n out of range).
 * counters_dev int64 [4], written by the call: {points that took the exact pass, 1 if the grid is unusable (a non-finite point, or
 * another n: features is not written), shells visited, points whose own normal is not finite}. */
size_t lnr_cloud_fpfh_workspace(int64_t n_points);
int lnr_cloud_fpfh(const void* grid, int64_t n_points, const double* normals, double radius, int32_t max_nn, double* features,
                   void* workspace, size_t workspace_bytes, int64_t* counters_dev, void* stream);

/* The nearest target of every query in feature space, brute force and exact (the KDTreeFlann over features of
 * registration_ransac_based_on_feature_matching).  targets [n_targets, dim] and queries [n_queries, dim], dim in
 * [1, LNR_FEATURE_DIM_MAX].  d2 = the sum over j = 0..dim-1, left to right from 0.0, of (q_j - t_j) * (q_j - t_j); the answer is the
 * target with the smallest (d2, index), the lower index winning a tie; a NaN d2 never wins.  index int32 [n_queries] (-1 for none)
 * and sq_distance [n_queries] (+inf for none).  The targets are split into slices over the second grid dimension and a second launch
 * takes the minimum of the slices' pairs; the order is total, so the result does not depend on the split.  split: 0 for the
 * library's rule (about 512 workgroups), else the number of slices wanted, at most 512 (both are capped by the 64-row tiles there
 * are).  workspace: lnr_feature_nearest_workspace(n_queries) bytes (0 = out of range). */
size_t lnr_feature_nearest_workspace(int64_t n_queries);
int lnr_feature_nearest(const double* targets, int64_t n_targets, const double* queries, int64_t n_queries, int32_t dim, int32_t split,
                        int32_t* index, double* sq_distance, void* workspace, size_t workspace_bytes, void* stream);

/* open3d's RegistrationRANSACBasedOnCorrespondence with a fixed number of hypotheses.  source [n_source,3], target [n_target,3],
 * corr int32 [m,2] (source index, target index), n_hypotheses H in [1, 2^22], max_distance d finite and > 0, edge_similarity e in
 * [0, 1] (0 switches the edge checker off).  Stated differences from open3d: H is a fixed count, there is no confidence-based early
 * stop, so the work and the answer depend on the arguments only; a hypothesis' pose comes from the two triangle frames, not from a
 * Kabsch fit of the sample; there is no final refit on the inliers.
 * Hypothesis h = 0..H-1: (x0, x1, x2, _) = philox4x32_10 with counter low 64 bits h, high 64 bits LNR_STREAM_RANSAC, key seed;
 * i_k = ((uint64) x_k * m) >> 32; sample k is correspondence i_k, (s_k, t_k) its source and target point.  In this order: two equal
 * indices reject the hypothesis (repeated index); with e != 0, for (k, j) = (0,1), (1,2), (2,0), ls = sqrt(d2(s_k, s_j)) and
 * lt = sqrt(d2(t_k, t_j)) (differences k minus j), rejected unless ls >= e * lt and lt >= e * ls (edge checker); the frame of
 * (a, b, c) = the three points in draw order is e1 = (b - a) / |b - a| per component, nrm = cross(e1, c - a), e3 = nrm / |nrm|,
 * e2 = cross(e3, e1), and a non-finite entry in the source's or the target's frame rejects the hypothesis (frame).  Otherwise
 * R_ab = (et1_a es1_b + et2_a es2_b) + et3_a es3_b, the centroids are ((a + b) + c) / 3.0 per axis, and
 * t_a = ct_a - ((R_a0 cs_0 + R_a1 cs_1) + R_a2 cs_2).
 * Score: every correspondence i = 0..m-1 in order, p = R s_i + t with lnr_cloud_append_transformed's rounding, d2 = d2(p, t_i)
 * (differences p minus t), an inlier when d2 < d * d.  The inlier d2 are summed left to right from 0.0 within each chunk of
 * LNR_RANSAC_CHUNK correspondences and the chunk sums are added in chunk order; counts are integers.
 * Best: the largest count, then the smallest sum, then the smallest h.
 * result_dev fp64 [18]: [0:16] the 4x4 transformation (row-major), [16] fitness = count / m, [17] inlier_rmse = sqrt(sum / count),
 * both 0 for a count of 0.  info_dev int64 [8]: {status, best h (-1 for none), its count, surviving hypotheses, rejected: repeated
 * index, rejected: edge checker, rejected: frame, m}.  status bit 1: m < 3 (no hypothesis is formed: every counter is 0), 2: no
 * hypothesis survived, 4: a correspondence index out of range (such a pair is never an inlier and spoils every frame it is in);
 * with bit 1 or 2 the transformation is the identity and the count 0.
 * workspace: lnr_ransac_workspace(m, H) bytes (48 m + 9 H + 12 H ceil(m / LNR_RANSAC_CHUNK), about; 0 = out of range). */
size_t lnr_ransac_workspace(int64_t n_correspondences, int64_t n_hypotheses);
int lnr_ransac_correspondence(const double* source, int64_t n_source, const double* target, int64_t n_target, const int32_t* corr,
                              int64_t n_correspondences, int64_t n_hypotheses, uint64_t seed, double max_distance,
                              double edge_similarity, void* workspace, size_t workspace_bytes, double* result_dev, int64_t* info_dev,
                              void* stream);

/* ---- segmentation (open3d's PointCloud::RemoveRadiusOutliers, ClusterDBSCAN and SegmentPlane; Ester et al., "A Density-Based -----
 *      Algorithm for Discovering Clusters", KDD 1996; Fischler and Bolles, "Random Sample Consensus", CACM 1981) ----------------------
 * Taking a cloud apart.  Everything is fp64 without fma and rounds operation by operation; dot, cross and |a| are the global
 * registration block's, d2(p, q) = (dx dx + dy dy) + dz dz with d = p - q per axis (lnr_nn_distance's; it is symmetric bit for bit).
 * Integer atomics only, no hand-over or waiting between workgroups inside a launch, every loop bounded by the call's arguments: two
 * runs give the same bytes. */
#define LNR_STREAM_PLANE 0x504C414E00000000ull    /* "PLAN" in the top word of the Philox counter's high half */

/* For every point i of the cloud a grid was built from (lnr_nn_grid_build), counts[i] (uint32, input order) = the number of points j,
 * i included, with d2(p_i, p_j) < radius * radius (strict, the product rounded once: lnr_icp_correspondences' rule).  radius finite
 * and > 0.  The walk covers at most ceil(radius / edge) + 1 shells of cells, as lnr_icp_correspondences' does (the one past
 * ceil(radius / edge) covers the rounding of the two cell assignments), and ends sooner once the shells' lower bound reaches
 * radius^2; the counts do not depend on the grid's edge.  PointCloud.remove_radius_outlier keeps point i when counts[i] > nb_points
 * (open3d's rule, whose count includes i).  counters_dev int64 [4], written by the call: {0, 1 if the grid is unusable (a non-finite
 * point, or another n: counts is not written), shells walked, 0}. */
int lnr_cloud_radius_count(const void* grid, int64_t n_points, double radius, uint32_t* counts, int64_t* counters_dev, void* stream);

/* open3d's ClusterDBSCAN over the points a grid was built from; eps finite and > 0, min_points >= 1.  With count_i as
 * lnr_cloud_radius_count's at radius eps: point i is a core when count_i >= min_points; two cores are adjacent when
 * d2 < eps * eps; a cluster is a connected component of cores; clusters are numbered 0, 1, ... by ascending smallest core index; a
 * core gets its cluster's number, a non-core with at least one core within d2 < eps * eps (a border point) the smallest number among
 * those cores' clusters, every other point (noise) -1.  These are the labels of open3d's sequential algorithm (indices in ascending
 * order, a breadth-first walk from every unvisited core, a noise point re-labelled by the first cluster that reaches it); they
 * depend on the order of the input only through the numbering.  labels int32 [n] in input order.
 * info_dev int64 [8], written by the call: {status, clusters, cores, border points, noise points, 0, 0, 0}; status bit 1: the grid
 * holds a non-finite point, 2: the grid is unusable (that, or built for another n); with a bit set every label is -1 and the counts
 * are 0.  workspace: lnr_cloud_dbscan_workspace(n) bytes (about 17 n; 0 = n out of range). */
size_t lnr_cloud_dbscan_workspace(int64_t n_points);
int lnr_cloud_dbscan(const void* grid, int64_t n_points, double eps, int32_t min_points, int32_t* labels, void* workspace,
                     size_t workspace_bytes, int64_t* info_dev, void* stream);

/* open3d's SegmentPlane with ransac_n = 3 and a fixed number of hypotheses.  points [n,3], distance_threshold t finite and > 0,
 * n_hypotheses H in [1, 2^22].  Stated differences from open3d: the sample size is always 3; H is a fixed count, there is no
 * probability-based stop; the draws are counter-based, so the result depends on the arguments only.
 * Hypothesis h = 0..H-1: (x0, x1, x2, _) = philox4x32_10 with counter low 64 bits h, high 64 bits LNR_STREAM_PLANE, key seed;
 * i_k = ((uint64) x_k * n) >> 32.  Two equal indices reject the hypothesis (repeated).  With a, b, c the three points in draw order:
 * nrm = cross(b - a, c - a) (differences per axis), L = |nrm|, nv = nrm / L per component, d = -dot(nv, a); L == 0, or a non-finite
 * L, nv component or d, rejects it (degenerate).
 * Score: for every point i = 0..n-1 in order e = dot(nv, p_i) + d, an inlier when |e| < t (strict; a NaN is never an inlier); e * e
 * of the inliers is summed left to right from 0.0 within each chunk of LNR_RANSAC_CHUNK points and the chunk sums are added in chunk
 * order (lnr_ransac_correspondence's rule); counts are integers.
 * Best: the largest count, then the smallest sum, then the smallest h.  inlier uint8 [n]: the best hypothesis's mask (open3d's
 * returned inliers precede its refit too).
 * Refit (refine != 0 and at least 3 inliers; otherwise the returned model is the hypothesis's): with q_i = p_i - a per axis, a the
 * best hypothesis's first sample point, the 9 cumulants (qx, qy, qz, qx qx, qx qy, qx qz, qy qy, qy qz, qz qz) are summed over the
 * points in lnr_cloud_outlier_threshold's order (thread j of block b adds its terms i = 256 b + j, + 256 B, ... in turn from 0.0,
 * B = min(ceil(n / 256), 2048); a block sums its threads by the xor butterfly of each wave and the four waves left to right; one
 * workgroup folds the B partials the same way), a point that is no inlier adding 0.0; each sum is divided by (double) count and the
 * covariance formed as lnr_cloud_normals forms it (C_xx = m_xx - m_x m_x, ...); the normal is FastEigen3x3's unit eigenvector of the
 * smallest eigenvalue with lnr_cloud_normals' degenerate-case rules, negated per component when its dot product with nv is negative;
 * the centroid is a + (m_x, m_y, m_z) per axis and d = -dot(normal, centroid).
 * plane_dev fp64 [8]: [0:4] the returned model (a, b, c, d), [4:8] the best hypothesis's own model.  info_dev int64 [8]: {status,
 * best h (-1 for none), its count, surviving hypotheses, rejected: repeated, rejected: degenerate, non-finite points, n}; status bit
 * 1: n < 3 (no hypothesis is formed), 2: no hypothesis survived; with either the plane is zeros and the mask empty.
 * workspace: lnr_plane_workspace(n, H) bytes (H + 12 H ceil(n / LNR_RANSAC_CHUNK) + 256 Ki, about; 0 = out of range). */
size_t lnr_plane_workspace(int64_t n_points, int64_t n_hypotheses);
int lnr_cloud_segment_plane(const double* points, int64_t n_points, double distance_threshold, int64_t n_hypotheses, uint64_t seed,
                            int32_t refine, double* plane_dev, uint8_t* inlier, void* workspace, size_t workspace_bytes,
                            int64_t* info_dev, void* stream);

/* ---- mesh sampling, outlier filter, trajectory transform (analysis/compute_metrics/maps/mesh_to_pcd.py; ------------------------
 *      examples/fusion_portable/create_lidar_map.py, mask_gt_with_trajectory.py) ------------------------------------------------- */
/* open3d's TriangleMesh::SamplePointsUniformly (mesh_to_pcd.py:22) with a defined order and counter-based draws.  vertices fp64
 * [n_vertices,3], triangles int32 [n_triangles,3], n_triangles and n_points within the cloud limit.
 * Area: with u = v0 - v1 and w = v0 - v2, c = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x) and
 * A_t = 0.5 * sqrt((c_x c_x + c_y c_y) + c_z c_z).
 * Cumulative area C_t, a 64-ary tree of fp64 additions: prefix(a)[t] for t in chunk c = t / 64 is the left-to-right sum
 * ((a[64c] + a[64c+1]) + ...) + a[t] for c = 0, and prefix(T)[c-1] + (that sum) otherwise, where T[c] is the left-to-right sum of the
 * whole chunk c (the last chunk may be short) and prefix(T) is formed by the same rule; C = prefix(A), S = C_{F-1}.
 * Ownership (open3d's stratified rule): n_t = min(n_points, max over u <= t of round((C_u / S) * (double) n_points)), round half away
 * from zero; triangle t owns the points n_{t-1} <= i < n_t, n_{-1} = 0.  (The running max only matters where C steps down by an ulp
 * between two chunks; n_{F-1} = n_points.)  A triangle of zero area owns nothing.
 * Point i: (x, y, z, w) = philox4x32_10 with counter low 64 bits i, high 64 bits 0x4D45534800000000 ("MESH" in the top word; no
 * other draw of the library has a non-zero top word), key seed; r1 = (double)(((uint64) x << 32 | y) >> 11) * 2^-53 and r2 likewise
 * from z, w; s = sqrt(r1), a = 1 - s, b = s * (1 - r2), c = s * r2; p = (a v0 + b v1) + c v2 per axis.
 * points [n_points,3] and triangle_index int32 [n_points] (nullable) depend on (mesh, n_points, seed) only.
 * workspace: lnr_mesh_sample_workspace(n_triangles) bytes (0 = out of range).  info_dev int64 [8], written by the call: {status, points
 * written, triangles with a non-finite vertex or an index out of range, S (fp64 bits), 0, 0, 0, 0}; status bit 1: a triangle uses a
 * non-finite vertex, 2: a vertex index is outside [0, n_vertices), 4: S is not finite; with any bit set nothing is written.  S = 0 or
 * n_triangles = 0 writes nothing and reports 0 points. */
size_t lnr_mesh_sample_workspace(int64_t n_triangles);
int lnr_mesh_sample_points(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, int64_t n_points,
                           uint64_t seed, void* workspace, size_t workspace_bytes, double* points, int32_t* triangle_index,
                           int64_t* info_dev, void* stream);

/* The workspace of the three entries below: lnr_cloud_tools_workspace(n_points) bytes (about 4 n; 0 = n out of range). */
size_t lnr_cloud_tools_workspace(int64_t n_points);

/* The first half of open3d's PointCloud::RemoveStatisticalOutliers (create_lidar_map.py:134) over the points a grid was built from:
 * the neighbours of point i are lnr_cloud_normals' (the m = min(nb_neighbors, n) smallest (d2, input index) pairs, i itself included,
 * by the same shell walk and the same exact pass after 5 shells); mean_distance_i = (((sqrt(d2_0) + sqrt(d2_1)) + ...) in list order,
 * starting from 0.0) / (double) m.  mean_distance [n] in input order; nb_neighbors in [1, LNR_KNN_MAX].  counters_dev int64 [4] as
 * lnr_cloud_normals'. */
int lnr_cloud_knn_mean_distance(const void* grid, int64_t n_points, int32_t nb_neighbors, double* mean_distance, void* workspace,
                                size_t workspace_bytes, int64_t* counters_dev, void* stream);

/* The second half: result_dev fp64 [4] = {mean, std, threshold, valid}.  valid = n_points when the grid is usable for them (else 0);
 * mean = (sum of mean_distance_i over mean_distance_i > 0) / valid; std = sqrt((sum of (mean_distance_i - mean)^2 over the same i) /
 * (valid - 1)); threshold = mean + std_ratio * std.  Either sum is taken in a fixed order: thread j of block b adds its terms i = 256 b
 * + j, + 256 B, ... (B = min(ceil(n / 256), 2048) blocks) in turn, a block sums its threads by the xor butterfly of each wave and the
 * four waves left to right, and one workgroup folds the B partials the same way.  A point is kept when mean_distance_i > 0 and
 * mean_distance_i < threshold (the caller's compare).  valid = 1 gives 0 / 0: a NaN threshold keeps nothing, as open3d's does. */
int lnr_cloud_outlier_threshold(const void* grid, const double* mean_distance, int64_t n_points, double std_ratio, void* workspace,
                                size_t workspace_bytes, double* result_dev, void* stream);

/* process_cloud of create_lidar_map.py (:77-111): every point of a scan moved by the trajectory's pose at the point's own time.
 * points [n,3] (sensor frame) and timestamps [n] (absolute, fp64); the trajectory is n_poses >= 2 device arrays: traj_times [K]
 * strictly increasing (the caller checks), traj_positions [K,3], traj_rotations [K,9] (row-major) and traj_rotvecs [K-1,3], the
 * rotation vectors log(R_k^T R_{k+1}).  A point with a non-finite coordinate or time is dropped and counted; else it is dropped as
 * below range unless sqrt((x x + y y) + z z) > min_range; else as outside the trajectory when tau < T_0 or tau > T_{K-1}.  Otherwise k is
 * the last index with T_k <= tau, at most K - 2; alpha = (tau - T_k) / (T_{k+1} - T_k); trans_a = P_k,a + alpha * (P_{k+1},a - P_k,a);
 * w = alpha * w_k per axis, theta = sqrt((w_x w_x + w_y w_y) + w_z w_z); R = R_k when theta < 1e-9, else with e = w / theta,
 * s = sin(theta), v = 1 - cos(theta) the matrix E = I + s K + v K^2 as lnr_motion_compensate writes it (E_00 = 1 - v * (e_y e_y +
 * e_z e_z), E_01 = (v * e_x) * e_y - s * e_z, ...) and R_ab = (R_k,a0 E_0b + R_k,a1 E_1b) + R_k,a2 E_2b; out_a = ((R_a0 x + R_a1 y)
 * + R_a2 z) + trans_a.  scipy's Slerp and interp1d give the same pose up to rounding; the fp64 value above is the definition.
 * out [n,3] receives the kept points in input order.  info_dev int64 [8], written by the call: {status, kept, below range, outside the
 * trajectory, non-finite, 0, 0, 0}; status bit 1: a non-finite point or time.  One host read of info_dev gives the count. */
int lnr_cloud_trajectory_transform(const double* points, const double* timestamps, int64_t n_points, const double* traj_times,
                                   const double* traj_positions, const double* traj_rotations, const double* traj_rotvecs,
                                   int64_t n_poses, double min_range, void* workspace, size_t workspace_bytes, double* out,
                                   int64_t* info_dev, void* stream);

/* ---- mesh tools (what a user of open3d's TriangleMesh calls between Mesher.get_mesh and a score or a viewer) -------------------- */
/* vertices fp64 [n_vertices,3], triangles int32 [n_triangles,3]; n_vertices <= 2^31 - 1 and 3 n_triangles <= 2^31 - 4096 (the sort's
 * limit).  Every fp64 expression rounds operation by operation (no fma), square roots and divides are IEEE; no float is added by an
 * atomic, so every output is a function of the mesh and two runs give the same bits.  Each entry writes info_dev int64 [4] =
 * {status, a, b, 0} (a and b as stated per entry); status bit 1: a vertex index lies outside [0, n_vertices), 2: a cluster id lies
 * outside [0, n_clusters).  With a bit set the other outputs are not to be used; no such index is dereferenced.
 * workspace: lnr_mesh_tools_workspace(n_vertices, n_triangles) bytes (about 88 per triangle and 4 per vertex; 0 = out of range).
 * Only lnr_mesh_select uses the per-vertex part: the other entries also take the size for n_vertices = 0. */
size_t lnr_mesh_tools_workspace(int64_t n_vertices, int64_t n_triangles);

/* open3d's TriangleMesh::ClusterConnectedTriangles.  Two triangles are adjacent when they share an edge: the unordered pair (min, max)
 * of two consecutive corners (0-1, 1-2, 2-0), also when the two are equal.  An edge of three or more triangles links them all; a shared
 * vertex links nothing.  Clusters are the connected components, numbered by ascending smallest triangle index (open3d's breadth-first
 * walk opens a cluster at the first unvisited triangle).  triangle_clusters int32 [n_triangles]; cluster_n_triangles int32
 * [n_triangles], of which the first C entries are the clusters' triangle counts and the rest 0; info a = C.  Only the triangles are
 * read: no vertex array is needed. */
int lnr_mesh_connected_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* workspace,
                                 size_t workspace_bytes, int32_t* triangle_clusters, int32_t* cluster_n_triangles, int64_t* info_dev,
                                 void* stream);

/* The third output of ClusterConnectedTriangles: cluster_area fp64 [n_clusters], for any labelling triangle_clusters int32
 * [n_triangles] with values in [0, n_clusters).  A_t is lnr_mesh_sample_points' area.  The order of the sum: the areas of cluster c's
 * triangles in ascending triangle index form a list; while the list is longer than one, every group of 64 consecutive entries (the last
 * may be shorter) is replaced by its left-to-right sum ((a_0 + a_1) + a_2) + ...; the entry left is cluster_area[c].  A cluster
 * without a triangle has area 0. */
int lnr_mesh_cluster_area(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                          const int32_t* triangle_clusters, int64_t n_clusters, void* workspace, size_t workspace_bytes,
                          double* cluster_area, int64_t* info_dev, void* stream);

/* The compaction behind open3d's RemoveTrianglesByMask, RemoveVerticesByMask, RemoveUnreferencedVertices, RemoveDegenerateTriangles and
 * Crop.  triangle_keep uint8 [n_triangles] and vertex_keep uint8 [n_vertices] (either nullable: keep all; non-zero keeps).  A triangle
 * survives when it is kept, its corners are in range and all three are kept vertices.  A vertex survives when it is kept and, with
 * drop_unreferenced != 0, a surviving triangle uses it.  Survivors keep their relative order: a new index is the number of survivors
 * before.  triangles_out int32 [n_triangles,3] receives the surviving triangles with their corners re-indexed, vertex_map int32
 * [n_vertices] every vertex's new index or -1; info a = surviving vertices, b = surviving triangles. */
int lnr_mesh_select(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const uint8_t* triangle_keep,
                    const uint8_t* vertex_keep, int32_t drop_unreferenced, void* workspace, size_t workspace_bytes, int32_t* triangles_out,
                    int32_t* vertex_map, int64_t* info_dev, void* stream);

/* open3d's TriangleMesh::ComputeVertexNormals as TriangleMesh.compute_vertex_normals (analysis/mesher.py) computes it, bit for bit.
 * Face normal of triangle t: with a = v1 - v0 and b = v2 - v0, f_t = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x).
 * Vertex i: s = 0.0, then s = s + f_t for every corner (k, t) with triangles[t][k] = i in ascending (k, t) order (numpy's three
 * np.add.at passes); norm = sqrt((s_x s_x + s_y s_y) + s_z s_z); normals[i] = s / norm, or s / 1.0 where norm > 0 does not hold.  A
 * vertex without a triangle gets zeros.  normals fp64 [n_vertices,3]. */
int lnr_mesh_vertex_normals(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, void* workspace,
                            size_t workspace_bytes, double* normals, int64_t* info_dev, void* stream);

/* ---- mesh simplification and smoothing (open3d's SimplifyVertexClustering, RemoveDuplicatedTriangles and FilterSmooth*) ---------- */
/* The conventions of "mesh tools": vertices fp64 [n_vertices,3], triangles int32 [n_triangles,3]; every fp64 expression rounds
 * operation by operation (no fma), square roots and divides are IEEE; no float is added by an atomic, so every output is a function of
 * the inputs only and two runs give the same bits.  Each entry writes info_dev int64 [4] = {status, a, b, 0} (a and b as stated per
 * entry).  An index out of range sets a status bit and is never dereferenced; with a bit set the other outputs are not to be used.
 * Where open3d leaves an order unspecified (it iterates unordered_sets), the order stated here is the definition.
 * Limits: n_vertices <= 2^31 - 1 (lnr_mesh_vertex_clusters: 2^31 - 4096, the sort's limit) and 6 n_triangles <= 2^31 - 4096.
 * workspace: lnr_mesh_filters_workspace(n_vertices, n_triangles) bytes (about 28 per vertex or 168 per triangle, whichever is more;
 * 0 = out of range).  lnr_mesh_vertex_clusters uses the per-vertex part only (n_triangles = 0 suffices), lnr_mesh_unique_triangles and
 * lnr_mesh_vertex_adjacency the per-triangle part only (n_vertices = 0 suffices); lnr_mesh_smooth takes none. */
size_t lnr_mesh_filters_workspace(int64_t n_vertices, int64_t n_triangles);

/* The vertex half of open3d's TriangleMesh::SimplifyVertexClustering(voxel_size, Average).  voxel_size finite and > 0.  lo_a = min_a -
 * 0.5 v over the vertices; a vertex's voxel is floor((p_a - lo_a) / v) per axis; the key, the "voxel_size is too small" rule and the
 * "key wider than 64 bits" rule are lnr_voxel_down_sample's.  Clusters are numbered by first occurrence (open3d's rule): cluster c is
 * the c-th distinct voxel met when walking the vertices in index order.  vertex_cluster int32 [n_vertices]; cluster_vertices fp64
 * [n_vertices,3], of which the first m rows are used: row c is the sum of the cluster's vertices in ascending vertex index, started
 * at 0.0, divided by (double) count.  info a = m, b = the number of non-finite vertices; status bit 1: a non-finite vertex (nothing
 * else is valid), 2: voxel_size too small, 4: key wider than 64 bits. */
int lnr_mesh_vertex_clusters(const double* vertices, int64_t n_vertices, double voxel_size, void* workspace, size_t workspace_bytes,
                             int32_t* vertex_cluster, double* cluster_vertices, int64_t* info_dev, void* stream);

/* open3d's TriangleMesh::RemoveDuplicatedTriangles as a mask, and the triangle half of SimplifyVertexClustering.  vertex_map int32
 * [n_vertices] (nullable: the identity, and n_mapped = n_vertices) with values in [0, n_mapped), n_mapped <= 2^31 - 1.  The three
 * corners are mapped to (t0, t1, t2) and rotated cyclically by open3d's rule: with t0 <= t1, (t0, t1, t2) when t0 <= t2, else
 * (t2, t0, t1); otherwise (t1, t2, t0) when t1 <= t2, else (t2, t0, t1).  The orientation is kept: a triangle and its mirror image
 * are different classes.  canonical int32 [n_triangles,3] receives the rotated triple.  triangle_keep uint8 [n_triangles] is 1 for
 * the triangle with the lowest index among those with the same canonical triple and 0 for the others; with drop_degenerate != 0 it is
 * 1 only where, in addition, the three mapped indices are pairwise different.  Correct for every index below 2^31 - 1 (the triple is
 * ordered by two stable sorts, not packed into one key).  info a = the number of ones in triangle_keep, b = the triangles whose mapped
 * indices are not pairwise different (whatever drop_degenerate is); status bit 1: a corner lies outside [0, n_vertices) or a mapped
 * value outside [0, n_mapped). */
int lnr_mesh_unique_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* vertex_map,
                              int64_t n_mapped, int32_t drop_degenerate, void* workspace, size_t workspace_bytes, int32_t* canonical,
                              uint8_t* triangle_keep, int64_t* info_dev, void* stream);

/* The adjacency list open3d's FilterSmooth* build, as a CSR: j is a neighbour of i when some triangle has both as consecutive corners
 * (0-1, 1-2, 2-0, either direction).  A pair (i, i) from a repeated index is left out, on purpose: open3d makes such a vertex its own
 * neighbour, which pins it with weight 1e12.  row_start int32 [n_vertices + 1] and neighbours int32 [6 n_triangles], of which
 * row_start[n_vertices] entries are used: row i is neighbours[row_start[i] .. row_start[i + 1]), each distinct neighbour once, ascending.
 * info a = row_start[n_vertices]; status bit 1: a corner lies outside [0, n_vertices) (that triangle contributes nothing). */
int lnr_mesh_vertex_adjacency(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* workspace, size_t workspace_bytes,
                              int32_t* row_start, int32_t* neighbours, int64_t* info_dev, void* stream);

/* n_steps >= 0 smoothing steps over vertices [n_vertices,3] with the adjacency (row_start [n_vertices + 1], neighbours
 * [n_neighbours]) of lnr_mesh_vertex_adjacency and scratch fp64 [n_vertices,3].  The steps ping-pong between the two arrays on the
 * device with no host synchronisation, and the result always ends in vertices; n_steps = 0 leaves its bytes untouched.  Every step
 * reads the positions p of the step before.  Step s (from 0) uses the factor f = lambda when s is even, mu when s is odd; both finite.
 * kind 0 (open3d's FilterSmoothSimple; f unused): S = p_i, then S = S + p_j for the neighbours j of i in ascending order;
 * out = S / (double)(1 + n_i).
 * kind 1 (FilterSmoothLaplacian, weights by inverse distance; Taubin is 2 k steps with lambda > 0 > mu): W = 0.0 and S = 0.0, then
 * per neighbour j in ascending order, with d = p_i - p_j: dist = sqrt((d_x d_x + d_y d_y) + d_z d_z), w = 1 / (dist + 1e-12),
 * W = W + w, S_a = S_a + w * p_j,a; then out_a = p_i,a + f * (S_a / W - p_i,a).
 * A vertex without neighbours keeps its position in both kinds (open3d divides 0 by 0 there).  info a = b = 0; status bit 1: a row
 * outside 0 <= row_start[i] <= row_start[i + 1] <= n_neighbours or a neighbour outside [0, n_vertices); that vertex stays where it is. */
int lnr_mesh_smooth(double* vertices, double* scratch, int64_t n_vertices, const int32_t* row_start, const int32_t* neighbours,
                    int64_t n_neighbours, int32_t kind, int32_t n_steps, double lambda, double mu, int64_t* info_dev, void* stream);

/* ---- ray casting (open3d's t.geometry.RaycastingScene, and the rays of a LiDAR that moves while it sweeps) ------------------------ */
/* The conventions of "mesh tools": vertices fp64 [n_vertices,3], triangles int32 [n_triangles,3], n_vertices <= 2^31 - 1 and
 * n_triangles <= 2^31 - 4096 (the sort's limit); every fp64 expression rounds operation by operation (no fma), square roots and divides
 * are IEEE; no float is added by an atomic, so every output is a function of the inputs only and two runs give the same bits.  Each
 * entry writes info_dev int64 [LNR_RAYCAST_INFO]; an index out of range sets a status bit and is never dereferenced; no entry reads
 * anything back to the host.
 *
 * The hit of a ray (o, d) on a triangle (A, B, C) is the watertight rule of Woop, Benthin and Wald (2013) in fp64:
 *   kz = the axis of largest |d|, the lowest axis on ties; kx = (kz + 1) % 3, ky = (kx + 1) % 3, the two swapped when d[kz] < 0;
 *   Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz];
 *   with A, B, C taken relative to o (A = A - o per axis): Ax = A[kx] - Sx * A[kz], Ay = A[ky] - Sy * A[kz], likewise for B and C;
 *   U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
 *   a miss when (U < 0 || V < 0 || W < 0) && (U > 0 || V > 0 || W > 0), or when det = (U + V) + W is 0;
 *   t = ((U * (Sz * A[kz]) + V * (Sz * B[kz])) + W * (Sz * C[kz])) / det, accepted when t_min <= t <= t_max; no back-face culling;
 *   the barycentrics are (u, v) = (U / det, V / det): the hit point is u A + v B + (1 - u - v) C (open3d's pair weighs B and C).
 * The result of a ray is the accepted hit with the smallest t, the smallest triangle index among equal t; a miss is t = +inf, id -1,
 * uv 0.  A ray with a non-finite component or a direction of all zeros is a miss and is counted; a triangle with a non-finite vertex
 * is left out and counted.  This is the whole definition: the tree only decides which triangles a ray is tested against, and its box
 * test is padded (by 2^-36 of the largest slab distance of the box, and the same share of the box's offset on an axis the ray does not
 * move along) so that it keeps every box whose triangle the rule above accepts; a node is dropped only when its padded entry distance
 * is strictly greater than the best t so far.
 *
 * The closest point q of a triangle (A, B, C) to a point p is the region walk of Ericson, Real-Time Collision Detection, 5.1.5, in
 * fp64, every operation rounded on its own, with dot(x, y) = (x0 * y0 + x1 * y1) + x2 * y2 and vectors handled per axis:
 *   ab = B - A, ac = C - A, ap = p - A, d1 = dot(ab, ap), d2 = dot(ac, ap);       d1 <= 0 && d2 <= 0: q = A;
 *   bp = p - B, d3 = dot(ab, bp), d4 = dot(ac, bp);                               d3 >= 0 && d4 <= d3: q = B;
 *   vc = d1 * d4 - d3 * d2;             vc <= 0 && d1 >= 0 && d3 <= 0: v = d1 / (d1 - d3), q = A + v * ab;
 *   cp = p - C, d5 = dot(ab, cp), d6 = dot(ac, cp);                               d6 >= 0 && d5 <= d6: q = C;
 *   vb = d5 * d2 - d1 * d6;             vb <= 0 && d2 >= 0 && d6 <= 0: w = d2 / (d2 - d6), q = A + w * ac;
 *   va = d3 * d6 - d5 * d4;             va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0: w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),
 *                                                                                  q = B + w * (C - B);
 *   otherwise den = 1 / ((va + vb) + vc), v = vb * den, w = vc * den, q = (A + ab * v) + ac * w.
 * The first branch that applies wins.  The squared distance is dot(p - q, p - q).  The barycentrics follow the ray's convention, (u, v)
 * weigh A and B: with v_B and w_C the weights of B and C in the branch taken - (0, 0) at A, (1, 0) at B, (0, 1) at C, (v, 0) on AB,
 * (0, w) on AC, (1 - w, w) on BC, (v, w) inside - v_out = v_B and u_out = (1.0 - v_B) - w_C.
 * The answer of a query p: a triangle is a candidate when its squared distance is <= max_distance_sq (a NaN, which a triangle
 * collapsed to a point or a line can produce through 0 / 0, never is); the answer is the candidate with the smallest squared
 * distance, the smallest triangle index among equal ones; with no candidate the squared distance is +inf, the id -1, the point and
 * the uv zeros.  A query with a non-finite coordinate gets that answer too and is counted; the triangles the build left out are no
 * candidates.  The tree's bound of a box [lo, hi]: per axis g = max(lo - p, p - hi, 0) reduced by 2^-36 max(|lo|, |hi|, |p|) and
 * clamped at 0, bound = (g0 * g0 + g1 * g1) + g2 * g2; a node is dropped only when its bound is strictly greater than the best
 * squared distance so far or than max_distance_sq, so equal distances still reach the lower index.
 *
 * The crossing count of a ray is the number of triangles the watertight rule above accepts with t_min <= t <= t_max, with the same
 * exclusions (a ray that is not finite or has a zero direction counts 0 and is counted).  A point is inside a closed mesh when the
 * count along LNR_OCCUPANCY_DIRECTIONS[0] from it, over [0, +inf], is odd; with three samples, when at least two of the three
 * directions give an odd count.  The directions are fixed, not drawn: the answer is a function of the mesh and the point.  The
 * limit: a ray through an edge or a corner shared by several triangles is accepted by each of them, so one direction can miscount;
 * the majority vote exists for this case. */
#define LNR_OCCUPANCY_DIRECTIONS {{1.0, 0.4142135623730951, 0.7320508075688772}, {-0.6180339887498949, 1.0, 0.3027756377319946}, \
                                  {0.2360679774997897, -0.7071067811865476, 1.0}}
#define LNR_RAYCAST_INFO 8
#define LNR_BVH_STACK 96            /* words of traversal stack per ray; a tree is at most 63 + 31 levels deep (code bits + tie bits) */

/* An opaque device BVH over (vertices, triangles): lnr_bvh_bytes(n_triangles) bytes (about 190 per triangle), built with a workspace
 * of lnr_bvh_workspace(n_triangles) bytes (about 26 per triangle); either is 0 when n_triangles is out of range.  The build: the
 * 63-bit Morton code of every usable triangle's box centre over the box of those centres (an axis without extent contributes 0), the
 * stable (uint64, uint32) radix sort, Karras' (2012) radix tree with the sorted position breaking ties between equal codes, and the
 * boxes fitted in LNR_BVH_STACK launches: a node takes its children's boxes only when an earlier launch wrote them.  A triangle with
 * a non-finite vertex or an index outside [0, n_vertices) is left out of the tree.  The buffer holds copies of the corners: the mesh
 * may be freed.  info_dev: {status, triangles in the tree, triangles with a non-finite vertex, triangles with an index out of range,
 * depth (the longest root-to-leaf path in edges; always < LNR_BVH_STACK), nodes, 0, 0}; status bit 1: an index out of range, 2: the
 * tree is deeper than the stack (cannot happen with 63-bit codes and 2^31 triangles; checked all the same).  With a bit set
 * lnr_cast_rays reports misses only and repeats the bit. */
size_t lnr_bvh_workspace(int64_t n_triangles);
size_t lnr_bvh_bytes(int64_t n_triangles);
int lnr_bvh_build(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, void* workspace,
                  size_t workspace_bytes, void* bvh, size_t bvh_bytes, int64_t* info_dev, void* stream);

/* open3d's RaycastingScene::CastRays with a window.  bvh from lnr_bvh_build with the same n_triangles; rays fp64 [n_rays,6] = (ox, oy,
 * oz, dx, dy, dz), the direction of any length (t is in units of it); t_min, t_max not NaN.  t_hit fp64 [n_rays], primitive_ids int32
 * [n_rays] (the index into the triangles given to the build), primitive_uvs fp64 [n_rays,2] (nullable).  One ray per lane, the near
 * child first; a ray stops after 2 x nodes visits (a damaged tree ends the kernel).  info_dev: {status, hits, rays that are not finite
 * or have a zero direction, node visits over all rays, rays stopped by the visit cap, triangles the build left out, depth, 0};
 * status bits 1 and 2 as the build's, 4: the visit cap was reached, 8: a stack column was full (its entry was dropped, never written
 * out of bounds). */
int lnr_cast_rays(const void* bvh, int64_t n_triangles, const double* rays, int64_t n_rays, double t_min, double t_max, double* t_hit,
                  int32_t* primitive_ids, double* primitive_uvs, int64_t* info_dev, void* stream);

/* open3d's RaycastingScene::ComputeClosestPoints with a reach: the closest point of the mesh to every query, by the rule above.
 * points fp64 [n_points,3]; max_distance_sq not NaN (+inf: no limit).  dist_sq fp64 [n_points], primitive_ids int32 [n_points],
 * closest fp64 [n_points,3] (nullable), primitive_uvs fp64 [n_points,2] (nullable).  One query per lane, the child with the smaller
 * bound first, at most 2 x nodes visits per query.  info_dev: {status, queries answered (id >= 0), queries with a non-finite
 * coordinate, node visits over all queries, queries stopped by the visit cap, triangles the build left out, depth, 0}; the status
 * bits are lnr_cast_rays'. */
int lnr_closest_points(const void* bvh, int64_t n_triangles, const double* points, int64_t n_points, double max_distance_sq,
                       double* dist_sq, int32_t* primitive_ids, double* closest, double* primitive_uvs, int64_t* info_dev, void* stream);

/* open3d's RaycastingScene::CountIntersections with a window: counts int32 [n_rays], the crossing count stated above; rays, t_min and
 * t_max as lnr_cast_rays takes them.  Every box whose padded slab meets the window is visited.  info_dev: {status, rays with a count
 * above 0, rays that are not finite or have a zero direction, node visits, rays stopped by the visit cap, triangles the build left
 * out, depth, 0}; the status bits are lnr_cast_rays'. */
int lnr_count_intersections(const void* bvh, int64_t n_triangles, const double* rays, int64_t n_rays, double t_min, double t_max,
                            int32_t* counts, int64_t* info_dev, void* stream);

/* The rays of a sensor that moves while it sweeps: the inverse of lnr_cloud_trajectory_transform.  directions fp32 [3,n_rays] in the
 * sensor frame (a scan's layout), timestamps fp64 [n_rays] (absolute), the trajectory arrays as lnr_cloud_trajectory_transform takes
 * them.  The pose at tau is that entry's, word for word: k the last index with T_k <= tau, at most K - 2; alpha = (tau - T_k) /
 * (T_{k+1} - T_k); trans_a = P_k,a + alpha * (P_{k+1},a - P_k,a); w = alpha * w_k per axis, theta = sqrt((w_x w_x + w_y w_y) + w_z
 * w_z); R = R_k when theta < 1e-9, else R_k E with E and the product as stated there.  Only the sine and cosine in E are pinned down
 * further, so that a restatement gives the same bits on any host (a library's sine is good to an ulp, and which ulp differs between
 * libraries; these are within 2 ulps): k = floor(theta * 0.6366197723675814 + 0.5), r = (theta - k * 1.5707963267948966) - k *
 * 6.123233995736766e-17, z = r * r; p_s = p_c = 1.0, then for j = 10 down to 1: p_s = 1.0 - (z * p_s) / (2j (2j + 1)) and p_c = 1.0 -
 * (z * p_c) / ((2j - 1) 2j); S = r * p_s, C = p_c; (sin, cos) = (S, C), (C, -S), (-S, -C), (-C, S) for k mod 4 = 0, 1, 2, 3.
 * rays fp64 [n_rays,6]: origin = trans, direction_a
 * = (R_a0 x + R_a1 y) + R_a2 z with (x, y, z) the direction widened to fp64.  A ray whose time lies outside [T_0, T_{K-1}] or whose
 * direction or time is not finite is six NaNs (lnr_cast_rays then reports a miss) and is counted.  info_dev: {status, rays written,
 * outside the trajectory, non-finite, 0, 0, 0, 0}; status bit 1: a non-finite direction or time. */
int lnr_trajectory_rays(const float* directions, const double* timestamps, int64_t n_rays, const double* traj_times,
                        const double* traj_positions, const double* traj_rotations, const double* traj_rotvecs, int64_t n_poses,
                        double* rays, int64_t* info_dev, void* stream);

/* ---- TSDF fusion (no counterpart in the reference; open3d's UniformTSDFVolume for range rays) --------------------------------- */
/* A dense volume of nx ny nz lattice nodes (each >= 2, the product < 2^31), z fastest: the layout the marching cubes above read.  Node
 * (i, j, k) lies at origin_a + (double) index_a * v per axis (origin: host fp64 [3], v = voxel_size; one multiply, one add); its voxel
 * is the cube of edge v centred on it.  Per node the caller owns, and zeroes, sum (int64) and count (uint32).  Every fp64 expression
 * here rounds operation by operation (no fma), and divides are IEEE.
 *
 * lnr_tsdf_integrate adds rays to the volume: rays fp64 [n_rays,6] = (o, d) as lnr_trajectory_rays writes them (d of unit length:
 * t below is metres along it), ranges fp64 [n_rays] (r), trunc > 0 and front >= trunc (+inf: free space is carved from the origin
 * on), n_rays < 2^32 - 256.  A ray is left out and counted as invalid when a component of o or d is not finite, d is zero, r is not
 * finite or r <= 0, or a grid-frame value below is not finite.  The grid frame puts voxel i of an axis on [i, i + 1):
 *   go_a = (o_a - origin_a) / v + 0.5,   gd_a = d_a / v.
 * The segment is t0 = max(0, r - front), t1 = r + trunc, clipped to the box [0, n_a] by slabs: per axis, with gd_a == 0 the ray misses
 * unless 0 <= go_a < n_a; otherwise ta = (0 - go_a) / gd_a, tb = (n_a - go_a) / gd_a, t0 = max(t0, min(ta, tb)), t1 = min(t1,
 * max(ta, tb)).  The ray misses the box, and is counted so, unless t0 < t1.
 * The walk is that of Amanatides and Woo (1987).  It enters at the grid coordinate e_a = go_a + t0 * gd_a, in voxel c_a = floor(e_a)
 * clamped to [0, n_a - 1].  Per axis step_a = sign(gd_a), tDelta_a = 1 / |gd_a| and tMax_a = ((c_a + (1 if gd_a > 0 else 0)) - go_a)
 * / gd_a, the t of the voxel's face ahead; an axis with gd_a == 0 has tMax_a = +inf and never steps.  Then, repeatedly: the voxel c
 * is visited; a is the axis of the smallest tMax, a tie going to x before y before z (a = x when tMax_x <= tMax_y and tMax_x <=
 * tMax_z, else y when tMax_y <= tMax_z, else z); the walk stops unless tMax_a < t1, and stops when c_a + step_a leaves [0, n_a - 1];
 * otherwise c_a += step_a and tMax_a += tDelta_a.
 * A visited voxel with node p gets s = r - (((p_x - o_x) * d_x + (p_y - o_y) * d_y) + (p_z - o_z) * d_z).  Nothing is written unless
 * s >= -trunc; otherwise q = llrint(min(s / trunc, 1) * 1048576) (ties to even), sum[node] += q and count[node] += 1, both integer
 * atomics whose result is not used: a volume does not depend on the order of waves, rays or calls, and is the same on every run.  A
 * ray updates a node at most once.  info_dev int64 [8], written by the call: {status (0), rays that updated at least one node,
 * invalid rays, rays that miss the box, node updates, 0, 0, 0}.
 *
 * lnr_tsdf_field reads the volume (min_count >= 1): field fp32 [nx][ny][nz] = (float) (-(double) sum / ((double) count * 1048576.0))
 * where count > 0 and 0 elsewhere; valid uint8 = 1 where count >= min_count, else 0.  The sign is flipped: field > 0 behind the
 * surface, which the marching cubes above call inside, so that their triangles face the sensor's side. */
int lnr_tsdf_integrate(const double* rays, const double* ranges, int64_t n_rays, int32_t nx, int32_t ny, int32_t nz,
                       const double* origin /*host [3]*/, double voxel_size, double trunc, double front, int64_t* sum, uint32_t* count,
                       int64_t* info_dev, void* stream);
int lnr_tsdf_field(const int64_t* sum, const uint32_t* count, int32_t nx, int32_t ny, int32_t nz, uint32_t min_count, float* field,
                   uint8_t* valid, void* stream);

/* ---- sparse TSDF (open3d's ScalableTSDFVolume / VoxelBlockGrid for range rays) ------------------------------------------------ */
/* A sparse volume IS the dense volume of lnr_tsdf_integrate over a lattice of nx ny nz nodes, of which only the blocks a ray wrote to
 * are stored: each axis has 2 <= n <= 2^21 nodes and there is no limit on the product.  Origin, voxel_size, trunc, front and the grid
 * frame, the slab clip against [0, n_a], the walk with its tie rule, s and q, and the invalid and miss classes are those of "TSDF
 * fusion" above, word for word and with the same operation-by-operation fp64 arithmetic.  So for every lattice a dense volume can
 * hold, every node of the sparse volume has the dense volume's sum and count, bit for bit.
 *
 * Blocks.  A block is 8 x 8 x 8 nodes; the block of node (i, j, k) is (i >> 3, j >> 3, k >> 3) and its key bx << 36 | by << 18 | bz:
 * 18 bits per axis, at most 54.  A block exists if and only if some ray wrote one of its nodes (s >= -trunc at a visited voxel); a
 * block that was only visited does not exist.  Nodes of a block with an index >= n_a on some axis are never written and never valid.
 *
 * Directory.  keys uint64 [B], ascending and unique, with a parallel slot uint32 [B]: block slot owns sum int64 [512] and count uint32
 * [512] in the caller's pool arrays [capacity][8][8][8], z fastest, zeroed by the caller.  An existing block keeps its slot for life.
 * The blocks a call creates take the slots B_old, B_old + 1, ... in ascending key order.  A lookup is a binary search over keys.
 * Hence the pool is a function of the sequence of the calls' ray sets, and the volume in directory order (ascending key) is a function
 * of the set of all rays, whatever their order, their split into calls, or the run.
 *
 * One integration is four calls on one stream, with rays, ranges, the lattice and the parameters as lnr_tsdf_integrate takes them, the
 * same in each.  The host reads a count after the first and after the second, because the pool is the caller's and grows there:
 *   lnr_tsdf_sparse_touch      walks the rays without writing.  A ray has a candidate at every written voxel whose block is not the
 *                              block of the voxel it wrote before and is not in the directory (keys [n_blocks]).  ray_offsets uint32
 *                              [n_rays + 1] gets the exclusive scan of the rays' candidate counts, counts_dev int64 [2] = {candidates, 0}.
 *   lnr_tsdf_sparse_insert     (n_candidates >= 1: the count read back) walks the rays that have a candidate again, sorts the candidate
 *                              keys (stable LSD radix, as many 8-bit passes as the lattice's highest key needs) and keeps the distinct
 *                              ones in the workspace; counts_dev[1] = their number, B_new.
 *   lnr_tsdf_sparse_merge      (n_new >= 1: B_new read back; the workspace of the insert, untouched, and the same n_candidates) sorts
 *                              the pairs (keys, slot) [n_blocks] and (new key r, n_blocks + r) into keys_out, slot_out [n_blocks + n_new],
 *                              which may be keys and slot themselves.
 *   lnr_tsdf_sparse_integrate  (keys, slot [n_blocks]: the directory after the merge, n_new of its blocks new; capacity >= n_blocks
 *                              blocks in sum and count) runs the walk and per written voxel resolves block to slot - a ray searches
 *                              only when the block changes - and issues the two atomics of the dense call.  A written voxel whose
 *                              block the search does not find, or finds with a slot >= capacity, writes nothing and is counted.
 *                              info_dev int64 [8], written by the call: {status (0), rays that updated at least one node, invalid rays,
 *                              rays that miss the box, node updates, new blocks, blocks, lost updates}; lost updates is 0 whenever the
 *                              four calls saw the same rays.
 * With no candidate, insert and merge are skipped.  lnr_tsdf_sparse_workspace: the bytes that serve a touch of n_rays rays and an
 * insert and merge that sort n_sort = n_blocks + n_candidates pairs (either may be 0); 0 for a count out of range (n_rays < 2^32 - 256,
 * n_sort <= 2^31 - 4096).
 *
 * lnr_tsdf_sparse_field writes field fp32 and valid uint8 [n_blocks][8][8][8] in directory order, gathered through slot, with
 * lnr_tsdf_field's expression and min_count rule (1 <= n_blocks < 2^22). */
size_t lnr_tsdf_sparse_workspace(int64_t n_rays, int64_t n_sort);
int lnr_tsdf_sparse_touch(const double* rays, const double* ranges, int64_t n_rays, int32_t nx, int32_t ny, int32_t nz,
                          const double* origin /*host [3]*/, double voxel_size, double trunc, double front, const uint64_t* keys,
                          int64_t n_blocks, uint32_t* ray_offsets, void* workspace, size_t workspace_bytes, int64_t* counts_dev,
                          void* stream);
int lnr_tsdf_sparse_insert(const double* rays, const double* ranges, int64_t n_rays, int32_t nx, int32_t ny, int32_t nz,
                           const double* origin /*host [3]*/, double voxel_size, double trunc, double front, const uint64_t* keys,
                           int64_t n_blocks, const uint32_t* ray_offsets, int64_t n_candidates, void* workspace, size_t workspace_bytes,
                           int64_t* counts_dev, void* stream);
int lnr_tsdf_sparse_merge(const uint64_t* keys, const uint32_t* slot, int64_t n_blocks, int64_t n_new, int64_t n_candidates, int32_t nx,
                          int32_t ny, int32_t nz, void* workspace, size_t workspace_bytes, uint64_t* keys_out, uint32_t* slot_out,
                          void* stream);
int lnr_tsdf_sparse_integrate(const double* rays, const double* ranges, int64_t n_rays, int32_t nx, int32_t ny, int32_t nz,
                              const double* origin /*host [3]*/, double voxel_size, double trunc, double front, const uint64_t* keys,
                              const uint32_t* slot, int64_t n_blocks, int64_t n_new, int64_t capacity, int64_t* sum, uint32_t* count,
                              int64_t* info_dev, void* stream);
int lnr_tsdf_sparse_field(const int64_t* sum, const uint32_t* count, const uint32_t* slot, int64_t n_blocks, int64_t capacity,
                          uint32_t min_count, float* field, uint8_t* valid, void* stream);

/* Marching cubes over the blocks of a directory (keys uint64 [n_blocks], ascending, unique and inside the lattice; 1 <= n_blocks <
 * 2^22), with field fp32 and valid uint8 [n_blocks][8][8][8] in directory order: the two-call protocol of lnr_mc_count / lnr_mc_emit
 * (totals_dev uint64 [2] = {vertices, triangles} read back by the caller, the same workspace in both calls, V < 2^30).  The definition
 * is that of lnr_mc_*_masked on the full lattice of nx ny nz nodes with every node of a missing block not valid: a vertex sits on every
 * lattice edge whose ends are both valid and differ, owned by the lower node; a cell is named by its lower node, which may lie in any
 * block, with its other corners in up to seven neighbouring blocks, and emits its case's triangles only when all eight corners are
 * valid; nodes with index n_a - 1 name no cell, and a valid byte of a node with an index >= n_a is not read.  Coordinates use global
 * indices in the dense formula, ((float) index + t) * spacing + origin with each operation rounded in fp32.  Order: blocks in
 * directory order, then nodes in block-local order (z fastest), then axis; triangles follow cell order, then the case table's order.
 * The mesh therefore equals the dense masked mesh as a set: the same triangles with the same nine floats each, in another order. */
size_t lnr_mc_sparse_workspace(int64_t n_blocks);
int lnr_mc_sparse_count(const uint64_t* keys, int64_t n_blocks, const float* field, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz,
                        float level, void* workspace, size_t workspace_bytes, uint64_t* totals_dev, void* stream);
int lnr_mc_sparse_emit(const uint64_t* keys, int64_t n_blocks, const float* field, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz,
                       float level, const float* spacing /*host [3]*/, const float* origin /*host [3]*/, void* workspace,
                       size_t workspace_bytes, int64_t n_verts, int64_t n_tris, float* verts, int32_t* tris, void* stream);

/* ---- tracking(src/common/frame.py:104-145; src/common/sensors.py:176-232; src/tracking/tracker.py:257-297) ----------------- */
#define LNR_MOCOMP_CONSTS 30      /* fp64 entries of lnr_motion_compensate's consts */
#define LNR_SKY_MAX_RAYS 65160    /* 181 x 360: the row stride lnr_sky_rays' output needs */

/* Frame.build_point_cloud (frame.py:136-144): the points of scan entries start, start + step, ... below stop (0 <= start,
 * stop <= n_points, step >= 1; the host derives them from the timestamps with the reference's expressions).  ray_directions fp32
 * [3, n_points], distances fp32 [n_points]; points fp64 [m,3], m = ceil((stop - start) / step): each coordinate is the fp32 product
 * dir * dist widened to fp64, the array the reference hands to open3d, in the layout lnr_nn_grid_build and the ICP take. */
int lnr_frame_cloud(const float* ray_directions, const float* distances, int64_t n_points, int64_t start, int64_t stop, int64_t step,
                    double* points, void* stream);

/* LidarScan.motion_compensate (sensors.py:176-232), in place on ray_directions [3, n_points] and distances [n_points]; timestamps
 * [n_points] (fp32, or fp64 when timestamps_fp64 != 0) are only read.  Per point f = (t_i - t0) / denom in the timestamps' type
 * (denom = t1 - t0 as the caller's own subtraction gave it; not clamped: the reference extrapolates), then in fp64:
 * trans = t_start + f (t_end - t_start); R = R_start exp(f theta axis) by Rodrigues' formula, R = R_start when theta < 1e-9 (the
 * reference's NUMERIC_TOLERANCE branch); q = T_target^-1 [R | trans] (dir dist); distances = |q| and ray_directions = q / |q|, each
 * rounded to fp32 once, at the store.  The reference's own chain is fp32 through pytorch3d; the fp64 value is this entry's
 * definition.  consts host fp64 [LNR_MOCOMP_CONSTS]: theta axis [3] (the axis-angle of R_start^-1 R_end), R_start [9] row-major,
 * t_start [3], t_end [3], the top three rows of T_target^-1 [12]; all must be finite (LNR_ERR_INVALID_ARG otherwise). */
int lnr_motion_compensate(float* ray_directions, float* distances, const void* timestamps, int32_t timestamps_fp64, int64_t n_points,
                          double t0, double denom, const double* consts /*host*/, void* stream);

/* Tracker.compute_sky_rays (tracker.py:257-297).  Per direction, in fp32: theta = round(rad2deg(atan2(y, x))) and
 * phi = round(rad2deg(atan2(sqrt(x x + y y), z))) (round half to even).  The occupancy image has phi_max - phi_min + 1 rows and 360
 * columns, a point sets pixel (phi - phi_min, theta - theta_min) with column 360 folded to 0; a 3x3 dilation and a 3x3 erosion follow,
 * both ignoring out-of-image neighbours (kornia's geodesic border) and without azimuth wrap; the top three rows are set.  Every zero
 * pixel (r, c), in row-major order, gives the unit vector (sin p cos t, sin p sin t, cos p) of p = deg2rad(r + phi_min),
 * t = deg2rad(c + theta_min); it is rotated by rotation (device fp32 [9], row-major) and kept when
 * 90 - rad2deg(atan2(sqrt(xw xw + yw yw), zw)) > 10.  sky fp32 [3, sky_stride] (sky_stride >= LNR_SKY_MAX_RAYS) receives the kept
 * vectors in that order in its first m columns.  workspace: lnr_sky_rays_workspace() bytes.  info_dev int32 [8], written by the call:
 * {status, m, zero pixels, rows, phi_min, theta_min, non-finite directions, 0}; status bit 1: a non-finite direction (it sets no
 * pixel).  One host read of info_dev gives m. */
size_t lnr_sky_rays_workspace(void);
int lnr_sky_rays(const float* ray_directions, int64_t n_points, const float* rotation, void* workspace, size_t workspace_bytes,
                 float* sky, int64_t sky_stride, int32_t* info_dev, void* stream);

/* ---- scan ingestion (examples/run_loner.py:59-157) --------------------------------------------------------------------------- */
#define LNR_SCAN_MAX_FOV_SEGMENTS 8
#define LNR_SCAN_TIME_NONE 0          /* no per-point times: every time is the stamp */
#define LNR_SCAN_TIME_GIVEN 1         /* point_times [n] fp32 */
#define LNR_SCAN_TIME_RECOMPUTE 2     /* (i % 2048) / 2048 * 0.1 of the original index i */
/* bits of info_dev[1]: the branches the timestamp heuristics took */
#define LNR_SCAN_NANOSECONDS 1        /* max |t| > 1e7: scaled by 1e-9 */
#define LNR_SCAN_NEGATIVE_START 2     /* t[first] < -0.001: t[first] subtracted */
#define LNR_SCAN_LOCAL 4              /* t[first] < 1e-2: the stamp added */
#define LNR_SCAN_GLOBAL 8             /* otherwise: rebased to the stamp */
#define LNR_SCAN_CONSTANT 16          /* t[last] - t[first] < 1e-3 (or no times): every time is the stamp */
#define LNR_SCAN_NO_TIMES 32          /* LNR_SCAN_TIME_NONE */

/* build_scan_from_msg of run_loner.py (:59-157) on the device: xyz [n,3] fp32 (and point_times [n] fp32) become the time-ordered scan
 * ray_directions [3,M], distances [M], timestamps [M] and order [M] int64, the original index of every output point.
 *  1. FOV.  If fov_enabled: theta = atan2f(y, x) in degrees (times the fp32 constant 180/pi), plus 360 where negative; a point passes
 *     if lo <= theta <= hi for any of the n_fov_segments <= LNR_SCAN_MAX_FOV_SEGMENTS segments (fov_segments host fp32 [n,2], degrees).
 *  2. Range.  dist = sqrtf(fmaf(z, z, fmaf(y, y, x*x))), what torch.Tensor.norm(dim=1) gives on a CPU build; the order is fixed here,
 *     not left to the compiler.  A point is kept if it passed the FOV test and dist > min_range; a NaN coordinate drops it.
 *  3. Times, on the kept points in input order, every operation in fp32; stamp is the scan's time as fp32.  LNR_SCAN_TIME_NONE: every
 *     time is stamp.  LNR_SCAN_TIME_RECOMPUTE: t = (i % 2048) / 2048 * 0.1 of the ORIGINAL index i; LNR_SCAN_TIME_GIVEN: t = point_times.
 *     Then, with first / last the first / last kept point:  if max |t| > 1e7: t *= 1e-9;  if t[first] < -0.001: t -= t[first] (on
 *     every call; the reference does it on its first call only, under its warn-once flag);  if t[first] < 1e-2: t += stamp, else
 *     t = (t - t[first]) + stamp;  if t[last] - t[first] < 1e-3: every time is stamp.
 *  4. Order.  Stable ascending sort by time, ties (-0 and +0 among them) keep input order; directions = xyz / dist (IEEE fp32
 *     division); everything gathered by the sort.
 * ray_directions is written with row stride M, so the caller allocates 3 n floats and views the first 3 M as [3,M].  workspace:
 * lnr_scan_from_points_workspace(n) bytes (about 28 n; 0 = n out of range).  All launches go to `stream`, nothing waits on the host.
 * info_dev int64 [8], written by the call: {M, LNR_SCAN_* bits, kept points whose input time is not finite, adjacent output times out
 * of order (0 unless a time is not finite), digit passes the sort ran, first kept index, last kept index, 0}.  One host read of
 * info_dev gives M; the caller treats M == 0 and a non-finite time as errors. */
size_t lnr_scan_from_points_workspace(int64_t n_points);
int lnr_scan_from_points(const float* xyz, const float* point_times /*nullable*/, int64_t n_points, int32_t time_mode, float stamp,
                         int32_t fov_enabled, const float* fov_segments /*host, nullable*/, int32_t n_fov_segments, float min_range,
                         void* workspace, size_t workspace_bytes, float* ray_directions, float* distances, float* timestamps,
                         int64_t* order, int64_t* info_dev, void* stream);

/* ---- loss ------------------------------------------------------------------------------------------ */
/* get_weights_gt (losses.py:29-51); eps_ray [n] per-ray or NULL -> eps_scalar. */
int lnr_weights_gt(const float* s /*[n,S] metres*/, const float* g /*[n] metres*/, const float* eps_ray,
                   float eps_scalar, int32_t normalise, int32_t n_rays, int32_t n_samples,
                   float* out /*[n,S]*/, void* stream);

/* get_logits_grad (losses.py:54-62), defaults eps=2, l_free=0.25, l_occ=2.5. */
int lnr_logits_grad(const float* s /*[n,S]*/, const float* g /*[n]*/, int32_t n_rays, int32_t n_samples,
                    float margin, float l_free, float l_occ, float* out, void* stream);

/* Front-to-back inference, an opt-in route of Model.render_depth (the reference composites all N_samples_test samples of every ray:
 * model_tcnn.py:73-105 -> rendering_tcnn.py:71-147).  The ray's sorted depths z [n_rays, n_samples] are drawn in full; the network is
 * evaluated in blocks of 256 samples along the ray on the rays whose transmittance is still >= 2^-24 (what lies behind contributes less
 * than fp32 resolution to the depth).  Per block b0: lnr_render_ftb_gather copies the alive rays' records and block depths into
 * compact arrays for lnr_density_forward (rays form, n_rays_dev = n_alive_dev) and zeroes next_count_dev; lnr_render_ftb_composite
 * (one wave per alive ray, the arithmetic and noise draw of lnr_render_forward) adds the block's contributions to depth_acc /
 * opacity_acc [n_rays], updates transmittance [n_rays] (caller: ones / zeros before block 0) and appends surviving rays to next_idx.
 * idx [cap] int32: alive ray indices, n_alive_dev their count; last != 0: nothing is appended.  depth = depth_acc + (1 - opacity_acc) far. */
int lnr_render_ftb_gather(const float* rays, const float* z, int32_t n_samples, const int32_t* idx, const int32_t* n_alive_dev,
                          int32_t cap, int32_t b0, int32_t block_samples, float* rays_c /*[cap,13]*/, float* z_c /*[cap,block]*/,
                          int32_t* next_count_dev, void* stream);
int lnr_render_ftb_composite(const float* sigma_c /*[cap,256]*/, const float* z, const float* rays, int32_t n_samples, const int32_t* idx,
                             const int32_t* n_alive_dev, int32_t cap, int32_t b0, int32_t block_samples,
                             const float* noise /*[n_rays,n_samples] explicit draws or NULL*/, float noise_std, uint64_t seed, float* transmittance, float* depth_acc, float* opacity_acc, int32_t* next_idx, int32_t* next_count_dev,
                             int32_t last, void* stream);

/* Fused Optimizer.compute_loss (optimizer.py:437-595, lidar branch) forward + backward:
 * render (as lnr_render_forward), weighted mean/var, JS divergence (:476-482,:614-626), dynamic
 * margin (:495-503), target weights (:504-506), depth MSE + LOS L1/L2 + opacity terms, then the
 * analytic backward to d_sigma [n,S] and the direct part of d_rays [n,13] (overwritten).
 * Reproduces the reference's `depth > far[0]` broadcast quirk (:460-461): every ground-truth depth is compared with the
 * `far` of the FIRST ray of the batch.  far0_dev (nullable, device float[1]): that value when this call sees only a shard
 * of the batch (keyframe-sharded window: rank 0's first ray, broadcast by the caller); NULL = this call's own first ray.
 * counts_dev [2] int32: {number of rays, number of opaque rays} over the WHOLE batch the loss is
 * normalised by (all GPUs) -- from lnr_count_opaque, all-reduced by the caller when sharded.
 * loss_out [8] float (accumulated; caller zeroes): {total, depth, los, opacity, sum of eps, -,-,-};
 * block_partials (nullable) [ceil(n_rays / LNR_LOSS_RAYS_PER_BLOCK) * 8] scratch: with it the terms are summed
 * without atomics (deterministic, and ~0.25 ms faster at 4096 rays than 20 k same-address atomics);
 * ray_stats (nullable) [n,8]: {depth, opacity, variance, mean_m, std_m, js, eps, opaque}.
 * weights_out (nullable) [n,S].
 * n_samples: 2 .. LNR_LOSS_MAX_SAMPLES.  More is refused with LNR_ERR_UNSUPPORTED before anything is launched, also for n_rays = 0:
 * the 32-samples-per-lane instantiation (1024 < S <= 2048) ended in a memory fault on its first launch and is not built (DESIGN.md
 * 3.5); lnr_render_forward / lnr_render_backward keep their 2048. */
int lnr_count_opaque(const float* rays, const float* depth_gt, int32_t n_rays, const int32_t* n_rays_dev,
                     const float* far0_dev, int32_t* counts_dev /*[2], overwritten*/, void* stream);
int lnr_los_loss_fused(const float* sigma, const float* z, const float* rays, const float* depth_gt,
                       int32_t n_rays, const int32_t* n_rays_dev, int32_t n_samples,
                       const float* noise, float noise_std, uint64_t seed,
                       float scale, const LnrLossConfig* cfg /*host*/, const int32_t* counts_dev, const float* far0_dev,
                       float* loss_out, float* d_sigma, float* d_rays, float* ray_stats,
                       float* weights_out, float* block_partials, int32_t* poison_dev, int32_t poison_tag, void* stream);

/* ---- optimisers -------------------------------------------------------------------------------------- */
/* torch.optim.Adam step (optimizer.py:257-269,376-380): betas (b1,b2), eps, no weight decay,
 * `step` = 1-based step count.  If zero_grad != 0 the gradient is cleared after use
 * (zero_grad(set_to_none=True), :380).  grad_scale multiplies the gradient first (1.0 normally). */
int lnr_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t count,
                  float lr, float beta1, float beta2, float eps, int32_t step, float grad_scale,
                  int32_t zero_grad, const int32_t* poison_dev, void* stream);

/* Optimizer._step_occupancy_grid (optimizer.py:598-609): pseudo-gradient per sample
 * (losses.py:54-62) scattered trilinearly into the logit grid, SGD step grid -= lr*grad.
 * grad_acc (nullable int64 [V^3]): if given, the pseudo-gradient is accumulated there in 64-bit fixed point (2^-42;
 * caller zeroes; integer atomics: exact, independent of the order of the waves and of the rays, and summable over ranks
 * with an integer all-reduce) and
 * applied by lnr_occ_grid_apply, which re-zeroes what it applied; if NULL the update is applied in place with float
 * atomics (summation order not fixed).  V <= 1023. */
int lnr_occ_grid_step(float* grid, int32_t V, const float* rays, const float* z, const float* depth_gt,
                      int32_t n_rays, const int32_t* n_rays_dev, int32_t n_samples, float scale,
                      float lr, float margin, float l_free, float l_occ, int64_t* grad_acc, void* stream);
int lnr_occ_grid_apply(float* grid, int64_t* grad_acc, int64_t count, float lr, int32_t zero_grad, const int32_t* poison_dev,
                       void* stream);

/* ---- self test ------------------------------------------------------------------------------------------ */
/* Checks the MFMA fragment layouts the density kernels rely on (v_mfma_f32_16x16x4_f32, v_mfma_f32_16x16x32_f16 and the split-bf16
 * product on v_mfma_f32_16x16x32_bf16; asymmetric operands); out[0] = max abs error of the fp32 form, out[1] = of the fp16 form,
 * out[2] = of the three-term bf16 split (operands chosen so that the kept partial products are the exact product: must be 0, and
 * the split itself must give back its input). */
int lnr_selftest_mfma(float* out /*[3]*/, void* stream);

/* ---- pose graph: multiway registration (open3d's GetInformationMatrixFromPointClouds, PoseGraph and GlobalOptimization with ------
 *      Levenberg-Marquardt; Choi et al., "Robust Reconstruction of Indoor Scenes", CVPR 2015) ---------------------------------------
 * Everything is fp64 without fma and rounds operation by operation.  Two runs give the same bytes: no float atomics, nothing handed
 * between workgroups inside a launch, ordinary launches only. */

/* The information matrix of a registered pair.  Each source point is moved by transformation (host [16], row-major, bottom row
 * 0 0 0 1; lnr_cloud_append_transformed's rounding), then paired by lnr_icp_correspondences' rule (strict d2 < r r, ties by the lower
 * index).  For every pair with the target q: G = [-[q]x | I] (3x6, rotation columns first: rows (0, q2, -q1, 1, 0, 0),
 * (-q2, 0, q0, 0, 1, 0), (q1, -q0, 0, 0, 0, 1)) and the 21 upper-triangle terms (G0a G0b + G1a G1b) + G2a G2b are summed in the fixed
 * order of the ICP systems.  workspace: lnr_icp_workspace(n_source) bytes.  result_dev fp64 [36]: the symmetric 6x6, row-major; all
 * zeros without a correspondence, which is no error.  info_dev int64 [4]: {status, correspondences, non-finite source points, 0};
 * status bits as lnr_icp_point_to_plane's: 1 a non-finite source point (it takes no correspondence), 2 the grid is unusable.  No host
 * read. */
int lnr_icp_information(const void* grid, int64_t n_targets, const double* source, int64_t n_source, const double* transformation,
                        double max_distance, void* workspace, size_t workspace_bytes, double* result_dev, int64_t* info_dev,
                        void* stream);

/* The graph.  Node i has the pose T_i [16] (node frame to world, rigid).  Edge k = (s, t, X, L, uncertain): X [16] takes source-frame
 * points to the target frame (ideally T_t^-1 T_s = X), L [36] is its information matrix, read as given and expected symmetric.
 *   E = X^-1 T_t^-1 T_s (rigid inverses [R^T | -R^T t]; products ((a0 b0 + a1 b1) + a2 b2) + a3)
 *   e = [(E21 - E12) / 2, (E02 - E20) / 2, (E10 - E01) / 2, E03, E13, E23]                   (0-based entries)
 * A step moves a pose by T_i <- M(d_i) T_i with M lnr_icp_point_to_plane's update rule ([Rz(d2) Ry(d1) Rx(d0) | d3..d5], composed
 * as there).  With A = X^-1 T_t^-1 and B = T_s, E(d_s, d_t) = A M(d_t)^-1 M(d_s) B, so at 0 dE/d d_s,c = A G_c B and
 * dE/d d_t,c = -A G_c B (G_c the generator of component c): J_t = -J_s exactly.  J = J_s is, with e_c the unit vector and b_j column
 * j of B's rotation,
 *   c < 3:  N_c[r][j] = A_R[r] . (e_c x b_j);  J[0..2][c] = ((N_c)21 - (N_c)12, (N_c)02 - (N_c)20, (N_c)10 - (N_c)01) / 2;
 *           J[3 + r][c] = A_R[r] . (e_c x B_t)
 *   c >= 3: J[0..2][c] = 0;  J[3 + r][c] = A_R[r][c - 3]
 * One block per edge carries the linearisation: W = J^T (L J) and g = J^T (L e); J_s^T L J_s = J_t^T L J_t = W, J_s^T L J_t = -W,
 * and the edge adds -w g to b_s and +w g to b_t.  q = e^T (L e).  Weight w: 1 for a certain edge, the line-process value l for an
 * uncertain one.  Objective F = sum w q + mu sum over uncertain edges of (sqrt(l) - 1)^2.
 *
 * Status bits of every info word 0 below: 1 an edge names a node out of range, 2 a self edge (both refused by lnr_pose_graph_build:
 * the graph then takes part in nothing), 4 a non-finite pose, 8 a non-finite measurement or information matrix, 16 a breakdown of
 * the conjugate gradients (p.Ap not > 0, or a non-finite sum). */
#define LNR_PG_MAX_NODES (1 << 24)
#define LNR_PG_MAX_EDGES (1 << 26)
size_t lnr_pose_graph_bytes(int64_t n_nodes, int64_t n_edges);        /* the graph buffer; 0 outside the limits (n_nodes >= 1) */
size_t lnr_pose_graph_workspace(int64_t n_nodes, int64_t n_edges);    /* the workspace of every call below */

/* The CSR adjacency: node -> its incident slots, slot = 2 k + role (role 0: the node is edge k's source, 1: its target), from the
 * keys (node, slot) by the shared radix sort, so every later gather walks a node's edges in edge order.  source, target int32 [m].
 * info_dev int64 [4]: {status, edges with an id out of range, self edges, 0}.  No host read. */
int lnr_pose_graph_build(const int32_t* source, const int32_t* target, int64_t n_nodes, int64_t n_edges, void* graph,
                         size_t graph_bytes, void* workspace, size_t workspace_bytes, int64_t* info_dev, void* stream);

/* Per edge e [m,6], q [m], W [m,36], g [m,6]; per node, through the adjacency and in its order, H_diag [n,36] = sum w W and
 * b [n,6] = -sum w J_i^T L e.  reference_node (-1 for none): its block is the identity and its b zero; in the solve its row and
 * column hold nothing else.  uncertain int32 [m], line fp64 [m] (read for uncertain edges).  info_dev int64 [4]: {status, 0, 0, 0}. */
int lnr_pose_graph_linearize(const void* graph, int64_t n_nodes, int64_t n_edges, const int32_t* source, const int32_t* target,
                             const double* poses, const double* measurements, const double* information, const int32_t* uncertain,
                             const double* line, int32_t reference_node, double* e, double* q, double* W, double* g, double* H_diag,
                             double* b, void* workspace, size_t workspace_bytes, int64_t* info_dev, void* stream);

/* (H + lambda I) delta = b by conjugate gradients with the block-Jacobi preconditioner: each diagonal block H_ii + lambda I through
 * lnr_icp_point_to_plane's pivoted LDLT, the product with H as a per-node gather over the adjacency (off-diagonal blocks -w W and
 * -w W^T), dot products as per-block sums folded by one workgroup.  It stops on |r| <= rtol |b| or after max_cg iterations, decided
 * on the device: every iteration is enqueued and later ones return at once.  Not a direct solve: delta carries an error of the order
 * of cond(H + lambda I) rtol |delta|.  delta [n,6].  info_dev int64 [4]: {status, iterations, 1 if the tolerance was met (0: the
 * max_cg stop), 0}.  No host read. */
int lnr_pose_graph_solve(const void* graph, int64_t n_nodes, int64_t n_edges, const int32_t* source, const int32_t* target,
                         const double* W, const int32_t* uncertain, const double* line, const double* H_diag, const double* b,
                         double lambda, int32_t reference_node, double rtol, int32_t max_cg, void* workspace, size_t workspace_bytes,
                         double* delta, int64_t* info_dev, void* stream);

/* open3d's GlobalOptimizationLevenbergMarquardt with the line process.  poses [n,16] are updated in place; line [m] is set to 1 and
 * receives the final line-process values.  mu = preference_loop_closure * max_correspondence_distance^2 * the mean of L[5][5] over
 * the uncertain edges.  lambda0 = 1e-5 * the largest diagonal entry of H, nu = 2.  One trial: delta from lnr_pose_graph_solve's
 * iteration at the current lambda; it stops (reason 2) when |delta| <= min_relative_increment (|x| + min_relative_increment), |x| the
 * norm of all node positions; F_new at the trial poses with the current line values; rho = (F - F_new) / (delta . (lambda delta +
 * b)).  rho > 0 accepts: lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2, every uncertain edge's l = (mu / (mu + q))^2 at the new
 * poses, and the system and F are formed again; then reason 3 when |b|_inf < min_right_term, 4 when F < min_residual, 1 after
 * max_iteration accepted steps.  Otherwise lambda *= nu, nu *= 2, and reason 5 after max_iteration_lm rejections in a row.  Reason 6:
 * a status bit.  The host reads one word per trial.  history_dev int32 [history_capacity] (nullable with capacity 0): per trial 1
 * accepted, 0 rejected, -1 the relative-increment stop.  result_dev fp64 [4]: {F, |b|_inf, lambda, mu}.  info_dev int64 [8]:
 * {status, trials, conjugate-gradient iterations of all trials, accepted, rejected, stop reason, 1 if stopped by a criterion (0: the
 * trials ran out), trials whose solve ended on max_cg and not on rtol (their steps are inexact)}.  With mu = 0 (every uncertain
 * edge's L[5][5] is 0) the line values stay 1. */
int lnr_pose_graph_optimize(const void* graph, int64_t n_nodes, int64_t n_edges, const int32_t* source, const int32_t* target,
                            double* poses, const double* measurements, const double* information, const int32_t* uncertain,
                            double* line, int32_t reference_node, double max_correspondence_distance, double preference_loop_closure,
                            int32_t max_iteration, int32_t max_iteration_lm, double min_relative_increment, double min_right_term,
                            double min_residual, double rtol, int32_t max_cg, void* workspace, size_t workspace_bytes,
                            int32_t* history_dev, int32_t history_capacity, double* result_dev, int64_t* info_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LONER_HIP_H */
