#!/usr/bin/env python3
"""bench.py -- training rays/s of the LONER mapping iteration on MI355X (BASELINE.json metric).

    python bench.py [--gpus N --steps K --warmup W]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one mapping iteration (optimizer.py:276-385 of the reference) over the default window:
8 keyframes x 512 rays x 512 samples, default network (16-level hash grid -> 64 -> 1), joint
optimisation of the density field and of 7 of the 8 poses (the first is anchored), occupancy-grid
step every 10th iteration, synthetic 64x1024 scans of an analytic scene (loner_amd/utils/synthetic.py).
With N > 1 the SAME 8-keyframe window is sharded over the ranks (keyframe i -> rank i mod N) with an
RCCL all-reduce of the density gradient per step ("strong" scaling).

A plain run sets up, warms up, times the steps (with the sampled per-kernel events of that region), writes --dump-outputs and
prints the line.  --full adds what the headline does not need, each outside the timed region: the L1 depth of the trained map,
an extended run, the other dtype, the north-star network, API-parity mode, the render leg, and (unless --no-cpu-baseline) the CPU
and torch-ROCm baselines with the matched-quality legs.

Prints ONE JSON line on rank 0 (see README / DESIGN.md for the fields).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--keyframes", type=int, default=8)
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--dtype", choices=["f32", "f16", "f32_chain"], default="f32",
                    help="arithmetic of the density network: f32 (default, stricter than the reference; the MLP's products as three-term "
                         "bf16 splits on the bf16 matrix pipe), f16 (the reference's storage types: fp16 features and weights on MFMA, fp32 "
                         "accumulation) or f32_chain (fp32 with exact fma chains on v_mfma_f32_16x16x4_f32: the pre-round-5 kernels, for A/B runs)")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg outside the headline (train mode, one GPU): L1 depth of the trained map, extended run, other "
                         "dtype, north-star network, API-parity mode, render leg, CPU / torch-ROCm baselines and matched-quality legs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the baselines and the matched-quality legs")
    ap.add_argument("--quick", action="store_true",
                    help="no effect: a run without --full is already only the timed region and its kernel table (kept so that older "
                         "command lines still parse)")
    ap.add_argument("--profile-every", type=int, default=-1,
                    help="HIP-event timing of the kernels on every N-th iteration of the timed region (0: none - then no roofline / kernels_ms; "
                         "default: every 4th, every 10th from 100 steps on - about ten sampled iterations)")
    ap.add_argument("--mode", choices=["train", "render"], default="train",
                    help="train (default): the mapping iteration (with --full, the inference leg as a `render` block in the line); "
                         "render: only the inference leg (Model.forward(testing=True) over a whole scan), for profiling")
    ap.add_argument("--launch-check", action="store_true",
                    help="only bring the ranks up, check the world size against --gpus, print {n_gpus, ranks} and exit "
                         "(no GPU work: with LNR_DIST_BACKEND=gloo this runs on a CPU-only box; tests/test_host.py)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what their last step handed back to the caller - density parameters, keyframe "
                         "poses, occupancy grid, loss terms - as DIR/<name>.npy (train mode), to compare two builds output for output")
    args = ap.parse_args()
    if args.dump_outputs is not None and (args.mode != "train" or args.steps < 1):
        ap.error("--dump-outputs needs --mode train and --steps >= 1")
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` (N > 1) without a launcher around it: re-exec this command line under
    torch.distributed.run, one rank per GPU, rendezvous on 127.0.0.1 (the reference fans its processes out itself too,
    examples/run_loner.py:339-424).  Returns the launcher's exit code."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


def build_window(n_kf, device=None):
    from loner_amd.common.frame import Frame
    from loner_amd.common.pose import Pose
    from loner_amd.common.sensors import LidarScan
    from loner_amd.mapping.keyframe import KeyFrame
    from loner_amd.utils import synthetic as SY
    from loner_amd.common.pose_utils import tensor_to_transform
    dirs, ts = SY.lidar_pattern()
    base, init = window_poses(n_kf)
    kfs = []
    for i in range(n_kf):
        dist = SY.scene_ranges(dirs, tensor_to_transform(base[i]))
        p6 = init[i]
        fr = Frame(None, LidarScan(dirs.clone(), dist, ts + 3.0 * i, sky_rays=torch.Tensor()), Pose())
        fr._lidar_pose = Pose(pose_tensor=p6, fixed=False)
        fr._gt_lidar_pose = Pose(pose_tensor=base[i].clone(), fixed=True)
        kfs.append(KeyFrame(fr, device))
    kfs[0].is_anchored = True
    return kfs


L1_RAYS = 512            # held-out rays of keyframe 0 for the matched-quality probe of every leg: the subset the reference's curve (G13) was scored on


def l1_subset(total=65536):
    """ray indices of the synthetic 64 x 1024 scan the G13 fixture scored (tests/support.py l1_scan_subset: every 128th ray, offset 7)"""
    return torch.arange(7, total, total // L1_RAYS)[:L1_RAYS]


def window_poses(n_kf):
    """(ground-truth pose6, initial pose6) of the synthetic window: N(0, 2 cm / 0.2 deg) error on every keyframe but the first"""
    from loner_amd.utils import synthetic as SY
    base = SY.trajectory_pose6(n_kf)
    gen = torch.Generator().manual_seed(1)
    init = []
    for i in range(n_kf):
        p6 = base[i].clone()
        if i > 0:
            p6[:3] += torch.randn(3, generator=gen) * 0.02
            p6[3:] += torch.randn(3, generator=gen) * 0.2 * 3.14159265 / 180
        init.append(p6)
    return base, init


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or "unknown"


class _Shape:
    def __init__(self, keyframes, rays, samples):
        self.keyframes, self.rays, self.samples = keyframes, rays, samples


# The reduced configuration on which "matched L1 depth" is established: the one of the G13 fixture (tests/golden/make_golden3.py),
# where the REFERENCE's own optimiser was recorded: 30.0 m before training, 14.55 m after 50 iterations.
QUALITY_SHAPE = _Shape(keyframes=2, rays=256, samples=128)
QUALITY_ITERS = 100
QUALITY_SEEDS = 8        # runs per GPU leg (each with its own random draws): the spread of L1 after 100 Adam iterations is part of the answer
QUALITY_REFERENCE = {"l1_initial_m": 30.02, "l1_after_50_iterations_m": 14.55, "l1_after_100_iterations_m": 10.86,
                     "source": "tests/golden/g13_l1_curve.npz: the reference's Optimizer + compute_l1_depth on this configuration (512 held-out rays, 256 samples)"}


def available_cores():
    """cores this process may actually use: os.cpu_count() is the HOST's (256 on the GPU boxes), the scheduler affinity and the cgroup
    CPU quota are what a container gets (an oversubscribed torch thread pool - 256 threads on a 16-core quota - runs an oracle iteration
    many times slower than 16 threads do)"""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                quota, period = txt[0], float(txt[1])
            else:
                quota, period = txt[0], float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota not in ("max", "-1"):
                n = min(n, max(1, int(float(quota) / period + 0.5)))
        except Exception:
            pass
    return max(n, 1)


def oracle_leg(args, device, budget_s, max_iters, min_iters=2, seed=0, threads=None):
    """A baseline leg: the oracle (oracle/mapping_step.py - the reference's mapping iteration restated op for op in torch, with
    the reference's own sampler op sequence, oracle/torch_sampling.py) on the SAME workload as the HIP path: the whole
    keyframe window, joint optimisation of the density field and the non-anchored poses, occupancy step at global steps 0, 10, ...
    device "cpu": timed on the host cores (cpu_baseline, kind "port").  device "cuda": the same torch ops executed by
    PyTorch-ROCm on the MI355X (torch_rocm_baseline) - what a straight PyTorch port of the reference would run at, with the
    hash-grid network written in torch instead of tinycudann.  Bounded: as many iterations as fit in ~budget_s (>= min_iters)."""
    from oracle import analysis as OA
    from oracle import mapping_step as MS
    from oracle import network as NW
    from oracle import poses as OP
    from loner_amd.common.settings import default_nerf_config
    from loner_amd.utils import synthetic as SY
    dev = torch.device(device)
    if threads is None:
        threads = min(os.cpu_count() or 1, 16)       # (the quality legs; the headline's cpu_baseline picks the fastest of three counts: main())
    if dev.type == "cpu":
        torch.set_num_threads(threads)
    nc = default_nerf_config()
    spec = NW.NetworkSpec.from_config(nc["pos_encoding_sigma"], nc["sigma_network"])
    scale, shift = SY.world_cube()
    cfg = MS.MapperConfig(n_rays=args.rays, n_samples=args.samples)
    dirs, _ = SY.lidar_pattern()
    base, init = window_poses(args.keyframes)
    dist0 = None

    def make():
        nonlocal dist0
        m = MS.OracleMapper(spec, NW.init_params(spec, 0), scale, shift, cfg, grid_size=100, device=dev, sampler="torch")
        kfs = []
        for i in range(args.keyframes):
            d = SY.scene_ranges(dirs, OP.transform_from_pose6(base[i]))
            if i == 0:
                dist0 = d
            kfs.append(MS.OracleKeyframe(dirs.to(dev), d.to(dev), init[i].clone().to(dev), anchored=(i == 0), time=3.0 * i))
        return m, kfs
    sync = (lambda: torch.cuda.synchronize()) if dev.type == "cuda" else (lambda: None)
    if dev.type == "cuda":                           # one untimed iteration: kernel selection, allocator warm-up
        m, kfs = make(); torch.manual_seed(0); m.iterate(kfs, 1); sync()
    m, kfs = make()

    def probe():
        idx = l1_subset(dirs.shape[1])
        torch.manual_seed(123)
        return OA.l1_depth(spec, m.params, m.grid[0, 0], dirs[:, idx].to(dev), dist0[idx].to(dev), kfs[0].pose6.detach(), m.scale, m.shift,
                           torch.tensor([1.0, 50.0], device=dev), 256, torch.rand(L1_RAYS, 128).to(dev), (torch.randn(L1_RAYS, 256) * 1.0).to(dev),
                           sampler="torch")[0]
    l1_before = probe()
    torch.manual_seed(seed)
    t0 = time.time()
    # ONE optimisation phase (one Adam, as the HIP leg's _do_iterate_optimizer call), cut short by the time budget.  (Round 3 called
    # iterate(kfs, 1) in a loop: every call started a fresh Adam, i.e. the baseline legs trained with sign-SGD steps of size lr and ended
    # ~10 % lower in L1 after 100 iterations than the same oracle with a proper Adam - the "bias" of the HIP leg in BENCH_r03.)
    n_valid = m.iterate(kfs, max_iters, stop_after_s=budget_s, min_iters=min_iters, sync=sync)
    sync()
    iters = m.last_iterations
    dt = time.time() - t0
    # quality probe (outside the timed region): L1 depth of L1_RAYS held-out rays of keyframe 0, as compute_l1_depth does (256 samples)
    l1 = probe()
    out = {"value": n_valid / dt, "unit": "rays/s", "kind": "port", "l1_depth_m_before": l1_before,
           "sample": f"{iters} mapping iterations of the SAME workload ({args.keyframes} keyframes x {args.rays} rays x {args.samples} samples, joint map + "
                     f"pose optimisation, default network, occupancy step at global step 0), oracle torch ops in fp32, {dt:.1f} s wall",
           "ms_per_iter": 1e3 * dt / iters, "iterations": iters, "l1_depth_m_after": l1}
    if dev.type == "cpu":
        out["cores"] = threads
        out["host_cores"] = os.cpu_count()
        out["cpu_model"] = cpu_model()
    else:
        out["device"] = torch.cuda.get_device_name(0)
        out["kind"] = "port (the oracle's torch ops through PyTorch-ROCm on the same MI355X: a restatement - the reference's density net is tinycudann, CUDA-only)"
    return out


class KernelTimer:
    """HIP-event timing of selected C-ABI calls on the stream they are launched on (torch's current stream)."""

    def __init__(self, ops, names):
        self.ops, self.names = ops, names
        self.events = {n: [] for n in names}
        self.enabled = False
        self.every = 4
        self.calls = {n: 0 for n in names}
        self.pool = []
        self._orig = {}
        for n in names:
            self._orig[n] = getattr(ops, n)
            setattr(ops, n, self._wrap(n))

    def _wrap(self, name):
        orig = self._orig[name]

        def inner(*a, **k):
            self.calls[name] += 1
            # every 4th call of an op is timed, and the library's per-kernel events (lnr_profile_*) are switched on for every 4th
            # iteration only (density_forward opens an iteration's density work, density_backward closes it): an event record costs
            # host time and keeps consecutive kernels from overlapping - with all of them on, the loop ran 12 % slower
            sampled = self.enabled and self.calls[name] % self.every == 0
            if sampled and name == "density_forward":
                self.ops.profile_enable(True)
            if not sampled:
                return orig(*a, **k)
            e0, e1 = self._event(), self._event()
            e0.record()
            r = orig(*a, **k)
            e1.record()
            self.events[name].append((e0, e1))
            if name == "density_backward":
                self.ops.profile_enable(False)
            return r
        return inner

    def _event(self):
        return self.pool.pop() if self.pool else torch.cuda.Event(enable_timing=True)

    def reserve(self, n_sampled_iterations):
        """Events for that many sampled iterations, created AND recorded once here, outside the timed region (torch creates the HIP
        event at the first record: ~15 us each - a sampled one-keyframe iteration paid 0.9 ms for them, two and a half iterations)."""
        for _ in range(2 * len(self.names) * max(int(n_sampled_iterations), 0)):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.pool.append(e)

    def summary(self):
        out = {}
        for n, evs in self.events.items():
            if evs:
                ms = [a.elapsed_time(b) for a, b in evs]
                out[n] = {"calls": len(ms), "avg_ms": sum(ms) / len(ms), "total_ms": sum(ms)}
        return out


def render_leg(opt, kf, scans=3, dtype="f32"):
    """The inference path that defines the metric's quality half (analysis/compute_l1_depth.py:42-64,262-265; renderer_lidar.py:71-93):
    every ray of a 64 x 1024 scan through Model.forward(testing=True) - N_samples_test = 2048 samples per ray, occupancy-guided
    sampling without jitter, density network forward, compositing - here through Model.render_depth, the depth-only form of it (no
    [N,S] weights, forward-only workspace, launches of 2^23 samples), and through Model.forward for comparison.  A "step" = one scan."""
    from loner_amd import ops
    from loner_amd.common.ray_utils import LidarRayDirections
    model, sampler = opt._model, opt._ray_sampler
    scan = kf.get_lidar_scan()
    lrd = LidarRayDirections(scan, chunk_size=len(scan))
    T = kf.get_lidar_pose().get_transformation_matrix().detach()
    with torch.no_grad():
        rays, depths = lrd.build_lidar_rays(torch.arange(len(scan)), opt._ray_range, opt._world_cube, T)
    n, S = rays.shape[0], int(model.cfg.render.N_samples_test)

    def timed(fn, reps):
        fn(); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            out = fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / reps, out
    ms_depth, depth = timed(lambda: model.render_depth(rays, sampler, opt._scale_f, testing=True), scans)
    # the opt-in front-to-back route (Model._render_depth_front_to_back): the same scan, the network evaluated only where the transmittance
    # is still >= 2^-24.  What it skips depends on how far the map has formed (profiles/r06_render_dead.txt)
    try:
        ms_ftb, depth_ftb = timed(lambda: model.render_depth(rays, sampler, opt._scale_f, testing=True, front_to_back=True), scans)
    except Exception as e:                                   # never let the optional route break the line
        ms_ftb, depth_ftb = None, None
        ftb_error = str(e)
    with torch.no_grad():
        ms_full, _ = timed(lambda: model(rays, sampler, opt._scale_f, testing=True, camera=False, return_variance=True), 1)
    # per-kernel times of one scan: the library's own events inside lnr_density_forward, torch events around the other two ops
    ops.profile_read()
    ops.profile_enable(True)
    spans = {"sample_rays_occ": [], "render_forward": []}
    orig = {k: getattr(ops, k) for k in spans}

    def wrap(name):
        def inner(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); r = orig[name](*a, **k); e1.record()
            spans[name].append((e0, e1))
            return r
        return inner
    for k in spans:
        setattr(ops, k, wrap(k))
    try:
        model.render_depth(rays, sampler, opt._scale_f, testing=True)
        torch.cuda.synchronize()
    finally:
        for k, f in orig.items():
            setattr(ops, k, f)
        ops.profile_enable(False)
    kern = {k: round(v["total_ms"], 4) for k, v in ops.profile_read().items()}
    kern.update({k: round(sum(a.elapsed_time(b) for a, b in v), 4) for k, v in spans.items()})
    spec = model.nerf_model._model_sigma.spec
    pts = float(n) * S
    half = dtype == "f16"
    enc_bytes = pts * (4.0 + spec.enc_dim * (2.0 if half else 4.0)) + n * 24.0 + (float(spec.n_params) - spec.n_mlp_params) * 4.0
    t_enc = kern.get("encode_forward", 0.0) * 1e-3
    gt = depths * opt._scale_f
    good = (gt > float(opt._ray_range[0])) & (gt < float(opt._ray_range[1]) - 0.25)
    l1 = float(((depth * opt._scale_f)[good] - gt[good]).abs().mean()) if bool(good.any()) else None
    return {"metric": "inference rays/sec (Model.forward(testing=True) depth, every ray of a 64x1024 scan)", "value": n / (ms_depth * 1e-3), "unit": "rays/s",
            "rays": n, "samples_per_ray": S, "ms_per_scan": round(ms_depth, 3), "ms_per_scan_full_result_dictionary": round(ms_full, 3),
            "dtype": dtype, "kernels_ms_per_scan": kern,
            "kernels_note": "event spans on the stream each kernel runs on: the sampler of launch i + 1 runs on a second stream BESIDE the density "
                            "forward of launch i (Model._render_no_grad), so its span is stretched by the sharing and the spans do not add up to "
                            "ms_per_scan; alone it takes 2.3 ms per scan (profiles/r04_render_kernel_stats.csv)",
            "l1_depth_m_of_this_scan": l1,
            "front_to_back": ({"ms_per_scan": round(ms_ftb, 3), "value": n / (ms_ftb * 1e-3), "unit": "rays/s",
                               "l1_depth_m_of_this_scan": (float(((depth_ftb * opt._scale_f)[good] - gt[good]).abs().mean()) if bool(good.any()) else None),
                               "mean_depth_relative_difference_to_default_route": float((depth_ftb.mean() - depth.mean()).abs() / depth.mean().abs()),
                               "note": "opt-in route (cfg.render.front_to_back / Model.render_depth(front_to_back=True)): blocks of 256 samples along the ray, "
                                       "a ray leaves once its transmittance is below 2^-24; different launch sizes key different in-kernel random numbers, so "
                                       "the two routes agree statistically here and to 1e-6 on replayed draws (tests/test_gpu_mapping.py)"}
                              if ms_ftb is not None else {"error": ftb_error}),
            "roofline": {"kernel": "encode_forward", "bound": "hbm", "achieved": enc_bytes / t_enc / 1e9 if t_enc > 0 else None, "peak": 8000.0,
                         "unit": "GB/s", "frac": enc_bytes / t_enc / 8e12 if t_enc > 0 else None, "algorithmic_bytes_per_scan": enc_bytes,
                         "traffic": None,
                         "note": "the dominant kernel of a scan: 8 table gathers per sample and level from the level's L2-resident table, bound by "
                                 "the L1/L2 line rate of the gathers (tools/gather_bench.hip), not by HBM bytes; feature planes are its HBM traffic"}}


def north_star_network_leg(n_rays, n_samples, device):
    """The network class the north star names besides the default one (sin/cos encoding + a wider ReLU MLP: frequency-12 -> 128 x 2,
    fp16 mode): forward and backward of lnr_density_* at the bench's sample count, against the dense fp16 MFMA peak.  Not part of the
    timed region; a secondary roofline entry (this is the one place where MFMA utilisation is the right yardstick)."""
    from loner_amd import hip, ops
    spec = hip.make_net_spec(dict(otype="Frequency", n_frequencies=12), dict(activation="ReLU", n_neurons=128, n_hidden_layers=2, precision="fp16"))
    g = torch.Generator(device="cpu").manual_seed(5)
    rays = torch.zeros(n_rays, 13); rays[:, 0:3] = torch.rand(n_rays, 3, generator=g) * 0.2 - 0.1
    rays[:, 3:6] = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=1); rays[:, 11] = 0.0117; rays[:, 12] = 0.58
    z = torch.sort(torch.rand(n_rays, n_samples, generator=g) * 0.57 + 0.0117, dim=1).values
    rays, z = rays.to(device), z.to(device)
    ds = torch.randn(n_rays, n_samples, generator=g).to(device); dr = torch.zeros(n_rays, 13, device=device)
    p = (torch.rand(int(spec.n_params), generator=g) - 0.5).to(device); grad = torch.zeros_like(p)

    def timed(fn, n=20):
        fn(); fn(); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / n
    fwd = timed(lambda: ops.density_forward(spec, p, rays=rays, z=z))
    bwd = timed(lambda: ops.density_backward(spec, p, ds, grad, rays=rays, z=z, reuse_features=True, d_rays=dr))
    mac = spec.n_neurons * spec.in_dim + (spec.n_hidden - 1) * spec.n_neurons ** 2 + spec.n_neurons
    pts = n_rays * n_samples
    return {"network": "Frequency(12) -> 128 ReLU x 2 -> 1, fp16 storage / fp32 accumulation (v_mfma_f32_16x16x32_f16)", "samples": pts,
            "forward_ms": round(fwd, 4), "backward_ms": round(bwd, 4),
            "forward_TFLOPs": round(pts * 2.0 * mac / fwd / 1e9, 1), "backward_TFLOPs": round(pts * 6.0 * mac / bwd / 1e9, 1),
            "peak_TFLOPs": 2500.0, "forward_mfma_frac": round(pts * 2.0 * mac / fwd / 1e9 / 2500.0, 4),
            "backward_mfma_frac": round(pts * 6.0 * mac / bwd / 1e9 / 2500.0, 4),
            "note": "backward = weight + input gradients incl. the encoding's backward, features reused from the forward (the training loop's route)"}


def make_bench_optimizer(rays, samples, dtype="f32", device_index=0, rank=0, params0=None):
    """The Optimizer of the benchmark: default settings, `rays` per keyframe x `samples` per ray, no sky rays, density network in
    `dtype`; params0 (optional): initial density parameters (the quality legs all start from oracle.network.init_params(spec, 0))."""
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import Optimizer
    from loner_amd.utils import synthetic as SY
    scale, shift = SY.world_cube()
    settings = default_optimizer_settings(log_directory=f"/tmp/loner_amd_bench_{rank}")
    settings["num_samples"]["lidar"] = rays
    settings["num_samples"]["sky"] = 0
    settings["model_config"]["model"]["render"]["N_samples_train"] = samples
    settings["model_config"]["model"]["nerf_config"]["sigma_network"]["precision"] = {"f16": "fp16", "f32_chain": "fp32_chain"}.get(dtype, "fp32")
    torch.manual_seed(0)                               # identical initial parameters on every rank
    o = Optimizer(settings, None, WorldCube(torch.tensor(scale), torch.from_numpy(shift)), device_index, False, True, False)
    if params0 is not None:
        with torch.no_grad():
            o._model.nerf_model._model_sigma.params.copy_(params0.to(o._device))
    return o


def l1_probe(o, kf0, max_rays):
    """analysis/compute_l1_depth.py semantics on keyframe kf0 with the optimiser's map; max_rays == L1_RAYS: exactly G13's subset"""
    from loner_amd.analysis.l1_depth import compute_l1_depth
    from loner_amd.common.ray_utils import LidarRayDirections
    scan = kf0.get_lidar_scan()
    return compute_l1_depth(kf0.get_lidar_pose(), LidarRayDirections(scan, chunk_size=2048), o._model,
                            o._ray_sampler, o._world_cube, o._ray_range, o._device, max_rays=max_rays,
                            indices=l1_subset(len(scan)) if max_rays == L1_RAYS else None)


def quality_initial_params():
    """Initial density parameters of every quality leg: the PRODUCT's initialiser with seed 0.  The oracle legs start from the same
    tensor - oracle.network.init_params(spec, 0) is bit-identical to it (tests/test_host.py::test_product_initialiser_equals_the_oracles),
    so the HIP legs need nothing from oracle/."""
    from loner_amd.common.settings import default_nerf_config
    from loner_amd.models.nerf_tcnn import SigmaNetwork
    nc = default_nerf_config()
    return SigmaNetwork(3, 1, nc["pos_encoding_sigma"], nc["sigma_network"], seed=0).params.detach().clone()


def hip_quality_run(seed, iters=None, shape=None, device_index=0):
    """One run of the HIP path on the quality configuration (QUALITY_SHAPE, the G13 fixture's) with its own random draws seeded by
    `seed`: L1 depth of L1_RAYS held-out rays of keyframe 0 before and after `iters` iterations of ONE optimisation phase."""
    from loner_amd.mapping.optimizer import OptimizationSettings
    q = shape or QUALITY_SHAPE
    iters = QUALITY_ITERS if iters is None else iters
    o, w = make_bench_optimizer(q.rays, q.samples, "f32", device_index, params0=quality_initial_params()), build_window(q.keyframes)
    o._model.cfg["render"]["N_samples_test"] = 256
    torch.manual_seed(123)
    l1_0 = l1_probe(o, w[0], L1_RAYS)
    torch.manual_seed(seed)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    o._do_iterate_optimizer(w, [None], optimizer_settings=OptimizationSettings(iters, False, False, False, True))
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    torch.manual_seed(123)
    return {"value": o.last_stats["n_valid_rays"] / dt, "unit": "rays/s", "ms_per_iter": 1e3 * dt / max(iters, 1),
            "l1_depth_m_before": l1_0, "l1_depth_m_after": l1_probe(o, w[0], L1_RAYS)}


def api_parity_leg(args, device_index, iters, warmup):
    """SURVEY 8d "state both modes": the training throughput in API-PARITY mode - the reference's own loop shape
    (optimizer.py:276-385) driven through the boundary classes one call at a time: per keyframe torch.randint + KeyFrame.build_lidar_rays
    (poses on the host, autograd through tensor_to_transform), Optimizer.compute_loss_api = Model.forward -> the result dictionary with
    its [N,S] weights / samples and [N,S,3] points in HBM -> torch ops for the loss (optimizer.py:437-595) -> loss.backward() through
    torch autograd -> Adam on the density parameters (the fused kernel) and on the host-side poses (torch.optim.Adam) -> occupancy step
    every N_iters_acc-th iteration, and one host sync per iteration (the reference's loss.item(), optimizer.py:354).  Same window, same
    network, same sample counts as the headline, which runs the fused-loss mode (no dictionary, no host sync, poses on the device)."""
    from loner_amd.mapping.optimizer import HipAdam, OptimizationSettings
    o, w = make_bench_optimizer(args.rays, args.samples, args.dtype, device_index), build_window(args.keyframes)
    o._optimization_settings = OptimizationSettings(iters, False, False, False, True)
    o._model.freeze_sigma_head(False)
    pose_params = []
    for kf in w:
        kf.get_lidar_pose().set_fixed(kf.is_anchored)
        if not kf.is_anchored:
            pose_params.append(kf.get_lidar_pose().get_pose_tensor())
    tr = o._model_config.train
    adam_sigma = HipAdam([{'params': o._model.get_sigma_parameters(), 'lr': tr.lrate_sigma_mlp}])
    adam_pose = torch.optim.Adam([{'params': pose_params, 'lr': tr.lrate_pose}])
    every = int(o._model_config.model.occ_model.N_iters_acc)
    n_scan = len(w[0].get_lidar_scan())

    def run(n_it):
        n_rays = 0
        for it in range(n_it):
            rays, depths = [], []
            for kf in w:
                r, d = kf.build_lidar_rays(torch.randint(n_scan, (args.rays,)), o._ray_range, o._world_cube, False)
                rays.append(r); depths.append(d)
            rays, depths = torch.vstack(rays), torch.cat(depths)
            loss = o.compute_loss_api((rays, depths), it)
            loss.backward()
            adam_sigma.step(zero_grad=True)
            adam_pose.step()
            adam_pose.zero_grad(set_to_none=True)
            if o._global_step % every == 0:
                o._step_occupancy_grid()
            o._global_step += 1
            n_rays += rays.shape[0]
            loss.item()                                    # the reference's per-iteration host sync
        return n_rays
    run(warmup)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    n = run(iters)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    S = args.samples
    return {"value": n / dt, "unit": "rays/s", "ms_per_step": 1e3 * dt / max(iters, 1), "steps": iters, "warmup": warmup, "dtype": args.dtype,
            "result_dictionary_bytes_per_ray": 20 * S + 12,
            "note": "API-parity mode (SURVEY 8d): KeyFrame.build_lidar_rays per keyframe -> Optimizer.compute_loss_api (Model.forward -> result "
                    "dictionary -> torch ops) -> torch autograd -> Adam; one host sync per iteration; poses optimised on the host like the "
                    "reference.  The headline value is the fused-loss mode of the same window."}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, opt, window, world, rank):
    """--dump-outputs: what the last timed step handed back to the caller of the mapping loop, as out_dir/<name>.npy, in full
    (33.7 MB for the default network):
      sigma_params    float32 [n_params]       density network parameters after the step (MLP weights, then the hash tables)
      poses           float32 [K, 6]           every keyframe's lidar pose (translation, axis-angle); sharded: each from its owner rank
      occupancy_grid  float32 [1, 1, V, V, V]  occupancy grid logits
      loss_terms      float64 [5]              the step's {total, depth, los, opacity, sum of eps}; sharded: summed over the ranks
    Inputs are seeded (synthetic scans, torch.manual_seed in make_bench_optimizer / per rank), so two runs with the same arguments
    start from the same state.  Collective in a sharded run (every rank calls it); rank 0 writes."""
    import numpy as np
    import torch.distributed as dist
    dev = torch.device("cuda", torch.cuda.current_device())
    poses = torch.stack([kf.get_lidar_pose().get_pose_tensor().detach().float().cpu() for kf in window]).to(dev)
    loss = opt.last_stats["loss_terms"][-1, :5].to(dev, torch.float64)
    if world > 1:
        from loner_amd.mapping.sharding import shard_window
        owned = torch.zeros(len(window), 1, device=dev)
        owned[shard_window(len(window), world, rank)] = 1.0
        poses = poses * owned                      # a rank's own keyframes only: the sum over the ranks is each keyframe's owner's pose
        dist.all_reduce(poses)
        dist.all_reduce(loss)
    if rank != 0:
        return
    arrays = {"sigma_params": opt._model.nerf_model._model_sigma.params.detach().float(),
              "poses": poses, "occupancy_grid": opt._occupancy_grid_model.occupancy_grid.detach().float(), "loss_terms": loss}
    arrays = {k: v.cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} bytes"
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    print(f"bench.py: wrote {', '.join(f'{k}{list(a.shape)}' for k, a in arrays.items())} ({total / 1e6:.1f} MB) to {out_dir}",
          file=sys.stderr, flush=True)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args))                # no launcher around us: become one
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s) (WORLD_SIZE)")
    # LNR_DIST_BACKEND=gloo lets two ranks share one GPU (RCCL refuses that): used to exercise the sharded code path on a 1-GPU box
    backend = os.environ.get("LNR_DIST_BACKEND", "nccl")
    import torch.distributed as dist
    if args.launch_check:
        # the argument -> ranks path alone (CPU test): every rank joins, rank 0 reports what the process group saw
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group(backend if backend != "nccl" or torch.cuda.is_available() else "gloo")
        seen = dist.get_world_size() if world > 1 else 1
        assert seen == args.gpus, (seen, args.gpus)
        ranks = [None] * seen
        if world > 1:
            dist.all_gather_object(ranks, rank)
            dist.destroy_process_group()
        else:
            ranks = [0]
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": seen, "ranks": ranks}), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (torch.cuda.is_available() is False)")
    if backend != "nccl":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
        # n_gpus in the line is what the process group saw, and it must be what --gpus asked for
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)
        world = dist.get_world_size()

    import __graft_entry__ as ge
    if rank == 0:
        ge.build()
    if world > 1:
        dist.barrier()

    from loner_amd import ops
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import OptimizationSettings, Optimizer
    from loner_amd.mapping.sharding import DistContext
    from loner_amd.utils import synthetic as SY

    scale, shift = SY.world_cube()

    def make_optimizer(dtype, params0=None):
        return make_bench_optimizer(args.rays, args.samples, dtype, local, rank, params0)

    opt = make_optimizer(args.dtype)
    window = build_window(args.keyframes)
    if world > 1:
        ctx = DistContext()
        opt.set_distributed(ctx)                           # the optimiser shards the window itself: keyframe i -> rank i mod N
        torch.manual_seed(1000 + rank)                     # different ray draws per rank
    my_window = window
    phase = lambda n: OptimizationSettings(n, False, False, False, True)

    if args.mode == "render":
        if args.warmup > 0:
            opt._do_iterate_optimizer(my_window, [None], optimizer_settings=phase(args.warmup))
        r = render_leg(opt, my_window[0], scans=max(args.steps, 1), dtype=args.dtype)
        r.update({"n_gpus": world, "steps": max(args.steps, 1), "warmup": args.warmup, "ms_per_step": r["ms_per_scan"], "higher_is_better": True,
                  "scaling": "weak", "vs_baseline": None, "data": "synthetic",
                  "config": {"workload": "inference: one 64x1024 synthetic scan (65536 rays) x 2048 samples through the default network after "
                                         f"{args.warmup} training iterations", "parallelism": "single GPU"}})
        if rank == 0:
            print(json.dumps(r), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    timer = KernelTimer(ops, ["density_backward", "density_forward", "los_loss_fused", "sample_rays_occ", "adam_step",
                              "occ_grid_step", "compact_rays", "lidar_rays_backward", "points_grad_to_rays"])
    # ---- warm-up (untimed) ----
    if args.warmup > 0:
        opt._do_iterate_optimizer(my_window, [None], optimizer_settings=phase(args.warmup))
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    timer.calls = {n: 0 for n in timer.names}
    # An event record keeps the kernels around it from running back to back (~25 us each, three dozen per sampled iteration: 1.1 % of
    # an 8-keyframe iteration when every 4th is sampled, but 2.5 iterations' worth for a one-keyframe shard): about ten sampled
    # iterations on one GPU, two per rank in a sharded run (the per-kernel table is rank 0's and secondary there)
    every = args.profile_every if args.profile_every >= 0 else \
        (max(4, args.steps // 2) if world > 1 else (4 if args.steps < 100 else 10))
    timer.every = max(every, 1)
    timer.enabled = every > 0                           # (it also switches the library's kernel events on, for the sampled iterations)
    if timer.enabled:
        timer.reserve(args.steps // timer.every + 2)
        ops.profile_enable(True); ops.profile_enable(False)      # (the library fills its own event pool here)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    opt._do_iterate_optimizer(my_window, [None], optimizer_settings=phase(args.steps))
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    timer.enabled = False

    final_loss = float(opt.last_stats["loss_terms"][-1, 0])
    n_valid_timed = float(opt.last_stats["n_valid_rays"])          # (the extended run below overwrites last_stats)
    n_valid = torch.tensor([float(opt.last_stats["n_valid_rays"]), elapsed], device="cuda", dtype=torch.float64)
    if world > 1:
        rays_total = n_valid[0:1].clone(); dist.all_reduce(rays_total)
        t_max = n_valid[1:2].clone(); dist.all_reduce(t_max, op=dist.ReduceOp.MAX)
        total_rays, elapsed = float(rays_total), float(t_max)
    else:
        total_rays = float(n_valid[0])

    kprof = ops.profile_read()                     # kernels inside lnr_density_forward / _backward, HIP events in the library
    ops.profile_enable(False)
    if args.dump_outputs is not None:
        dump_outputs(args.dump_outputs, opt, my_window, world, rank)      # (before anything below trains the map further)
    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    # quality half of the metric ("at matched L1 depth"): render held-out rays of the first keyframe with the trained
    # map (Model.forward(testing=True), 2048 samples) and compare with the analytic ranges.  Outside the timed region, --full only.
    from loner_amd.analysis.l1_depth import compute_l1_depth
    from loner_amd.common.ray_utils import LidarRayDirections

    def l1_of(o, kf0, max_rays):
        try:
            return compute_l1_depth(kf0.get_lidar_pose(), LidarRayDirections(kf0.get_lidar_scan(), chunk_size=2048), o._model,
                                    o._ray_sampler, o._world_cube, o._ray_range, o._device, max_rays=max_rays)
        except Exception as e:      # never let the quality probe break the benchmark line
            return f"failed: {e}"
    l1_depth = l1_of(opt, my_window[0], 4096) if args.full else None

    # A longer look at the same loop, OUTSIDE the official timed region (which is whatever --steps asked for; the driver uses 20 steps =
    # ~45 ms, where run-to-run spread is the size of a typical kernel gain): 200 further iterations of the same optimiser, timed the same
    # way, no per-kernel events.  The iteration gets cheaper as the map forms (dead samples produce no gradient records), so this is a
    # companion figure, not a replacement for ms_per_step.
    extended = None
    if world == 1 and args.full:
        torch.cuda.synchronize()
        t_e = time.perf_counter()
        opt._do_iterate_optimizer(my_window, [None], optimizer_settings=phase(200))
        torch.cuda.synchronize()
        dt_e = time.perf_counter() - t_e
        extended = {"steps": 200, "after_iterations": args.warmup + args.steps, "ms_per_step": 1e3 * dt_e / 200,
                    "value": opt.last_stats["n_valid_rays"] / dt_e, "unit": "rays/s"}

    # the other arithmetic mode of the density network, same workload, same step counts (outside the headline's timed region)
    other = None
    if world == 1 and args.full:
        try:
            od = "f16" if args.dtype == "f32" else "f32"
            o2, w2 = make_optimizer(od), build_window(args.keyframes)
            # (at least 10 warm-up iterations: this leg builds a second optimiser - 6 GB of workspace, another set of kernels - late in the
            # process, and with the driver's --warmup 5 its short timed window caught one-time costs: 5.3 ms per step against 1.96 alone)
            o2._do_iterate_optimizer(w2, [None], optimizer_settings=phase(max(args.warmup, 10)))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            o2._do_iterate_optimizer(w2, [None], optimizer_settings=phase(args.steps))
            torch.cuda.synchronize()
            dt2 = time.perf_counter() - t1
            other = {"dtype": od, "value": o2.last_stats["n_valid_rays"] / dt2, "unit": "rays/s", "ms_per_step": 1e3 * dt2 / max(args.steps, 1),
                     "final_loss": float(o2.last_stats["loss_terms"][-1, 0]), "l1_depth_m": l1_of(o2, w2[0], 4096),
                     "note": "f16 = the reference's storage types (tinycudann half precision): fp16 encoded features and MLP weights on "
                             "v_mfma_f32_16x16x32_f16 with fp32 accumulation, fp32 master parameters and gradients; f32 = everything fp32"}
            del o2, w2
        except Exception as e:
            other = {"error": str(e)}

    ns_net = None
    if world == 1 and args.full:
        try:
            ns_net = north_star_network_leg(args.keyframes * args.rays, args.samples, "cuda")
        except Exception as e:
            ns_net = {"error": str(e)}
    api_mode = None
    if world == 1 and args.full:
        try:
            api_mode = api_parity_leg(args, local, iters=min(max(args.steps, 1), 20), warmup=3)
        except Exception as e:
            api_mode = {"error": str(e)}
    render = None
    if world == 1 and args.full:
        try:
            render = render_leg(opt, my_window[0], scans=2, dtype=args.dtype)
        except Exception as e:
            render = {"error": str(e)}
    ksum = timer.summary()
    spec = opt._model.nerf_model._model_sigma.spec
    n_local = n_valid_timed / max(args.steps, 1)          # rays per launch on this rank
    pts = n_local * args.samples
    F = int(spec.n_features)
    n_rec = int(spec.n_levels)                                      # every level goes through the record kernel
    rec_table_floats = sum(int(spec.level_size[l]) * F for l in range(int(spec.n_levels)))
    h, ind, nh = spec.n_neurons, spec.in_dim, spec.n_hidden
    mac = h * ind + (nh - 1) * h * h
    plane_b = 2.0 if args.dtype == "f16" else 4.0                      # bytes of one feature-plane element
    # dense MFMA peak of the MLP kernels' arithmetic type: the fp32 mode runs 6 bf16 products per fp32 product on the bf16 pipe, i.e. at
    # best 2500 / 6 = 417 TFLOP/s of fp32-equivalent work (its yardstick); the exact-chain kernels are held to the fp32 MFMA peak
    mfma_peak = 2500.0e12 if args.dtype == "f16" else (157.3e12 if args.dtype == "f32_chain" else 2500.0e12 / 6.0)
    # Algorithmic work per launch:
    #   encode_backward: d_feature planes in, z and the ray records once, 6 ray-gradient floats out, the table gradient once
    #   mlp_backward:    forward recompute + input gradient + weight gradient GEMMs of the fp32 MLP
    alg = {
        "encode_backward": {"bytes": pts * (n_rec * F * 4.0 + 4.0) + n_local * 24.0 + rec_table_floats * 4.0},
        # encode_dx (the input gradient as its own launch): d_feature planes and z in, the ray records once, 6 ray-gradient floats out
        "encode_dx": {"bytes": pts * (n_rec * F * 4.0 + 4.0) + n_local * (24.0 + 24.0)},
        "encode_forward": {"bytes": pts * (4.0 + int(spec.n_levels) * F * 4.0) + n_local * 24.0 + (float(spec.n_params) - spec.n_mlp_params) * 4.0},
        "table_grad_reduce": {"bytes": rec_table_floats * 8.0},
        # (fp16 mode: the feature planes the MLP kernels read are half2 pairs, the d_feature planes they write stay fp32)
        "mlp_backward": {"flops": pts * 2.0 * (3 * mac + h), "bytes": pts * (spec.enc_dim * (2.0 * plane_b + 4.0) + 4.0)},
        "mlp_forward": {"flops": pts * 2.0 * (mac + h), "bytes": pts * (spec.enc_dim * plane_b + 4.0)},
    }
    traffic = {}
    tf = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tf):
        try:
            traffic = json.load(open(tf))
        except Exception:
            traffic = {}
    traffic_stale = None
    if traffic:
        from loner_amd.build import sources_digest
        traffic_stale = traffic.get("kernel_sources_sha") != sources_digest()
        if traffic_stale:
            print(f"bench.py: WARNING - profiles/traffic.json was collected on other kernel sources (its stamp {traffic.get('kernel_sources_sha')!r}, "
                  f"commit {traffic.get('commit')!r}; now {sources_digest()!r}): roofline.traffic is stale, re-run tools/pmc.sh + tools/traffic_from_pmc.py",
                  file=sys.stderr)
    kernels = {}
    for name, v in kprof.items():
        ent = {"avg_ms": round(v["avg_ms"], 4), "calls": v["calls"]}
        a_ = alg.get(name)
        if a_:
            t = v["avg_ms"] * 1e-3
            if "bytes" in a_:
                ent["hbm_GBps"] = round(a_["bytes"] / t / 1e9, 1); ent["hbm_frac"] = round(a_["bytes"] / t / 8e12, 4)
            if "flops" in a_:
                ent["mfma_TFLOPs"] = round(a_["flops"] / t / 1e12, 2); ent["mfma_peak_TFLOPs"] = mfma_peak / 1e12
                ent["mfma_frac"] = round(a_["flops"] / t / mfma_peak, 4)
        kernels[name] = ent
    for name, v in ksum.items():
        if name not in ("density_forward", "density_backward"):
            kernels[name] = {"avg_ms": round(v["avg_ms"], 4), "calls": v["calls"]}
    roofline = None
    if kprof:
        dom = max(kprof, key=lambda k: kprof[k]["total_ms"])
        t = kprof[dom]["avg_ms"] * 1e-3
        a_ = alg.get(dom, {"bytes": 0.0})
        roofline = {"kernel": dom, "bound": "hbm", "achieved": a_.get("bytes", 0.0) / t / 1e9, "peak": 8000.0, "unit": "GB/s",
                    "frac": a_.get("bytes", 0.0) / t / 8e12, "traffic": traffic.get(dom + "_bytes_per_launch"),
                    "traffic_stale": traffic_stale, "traffic_commit": traffic.get("commit"),
                    "avg_launch_ms": kprof[dom]["avg_ms"], "algorithmic_bytes_per_launch": a_.get("bytes", 0.0),
                    "traffic_source": "profiles/traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of an earlier run of this command "
                                      "(tools/pmc.sh), NOT measured by this run; FETCH_SIZE doubled as the microarchitecture guide prescribes for gfx950",
                    "note": "dominant kernel by total time over the timed region, timed with HIP events recorded by the library on the "
                            "launch stream (lnr_profile_*).  It moves few algorithmic bytes and is not HBM-bound: the SQ counters "
                            "(profiles/r04_pmc_sq_instmix.txt) show an instruction-bound kernel pair - 176 M + 121 M VALU wave instructions per backward "
                            "(the VALU 72 % / 50 % busy), half of a wave's cycles parked in s_waitcnt / barriers - whose in-LDS radix partition of the "
                            "gradient records, hashing, and the d/dx term's table re-gather (47 M L2 line reads = 6 GB over the L2 -> L1 path, "
                            "profiles/r04_pmc_tcp_tcc_encode.txt) overlap only partly; four structural variants were measured in round 4 "
                            "(DESIGN.md 3.4; docs/HISTORY.md 4.3, 8)",
                    "secondary": {k: v for k, v in kernels.items() if k != dom and k in ("encode_backward", "encode_dx", "mlp_backward", "mlp_forward", "encode_forward", "table_grad_reduce")}}
    line = {
        "metric": "training rays/sec", "value": total_rays / elapsed, "unit": "rays/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / max(args.steps, 1), "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"mapping iteration, {args.keyframes}-keyframe window x {args.rays} rays x {args.samples} samples, "
                               "default cfg (HashGrid 16x2 T=2^18 -> 64 -> 1, L1_JS loss, OGM sampler), joint map+pose optimisation, "
                               "synthetic 64x1024 scans (stand-in for Fusion Portable canteen, BASELINE configs[1])",
                   "keyframes": args.keyframes, "rays_per_keyframe": args.rays, "samples_per_ray": args.samples,
                   "parallelism": f"keyframe-sharded x{world}" if world > 1 else "single GPU"},
        "roofline": roofline,
        "north_star_network": ns_net,
        "api_parity_mode": api_mode,
        "render": render,
        # whole-path HBM roofline of SURVEY 8d: B_ray = 72 B (ray record, gt depth, per-ray outputs) + dense Adam traffic
        # (28 B per parameter: read p,g,m,v, write p,m,v) amortised over the rays of an iteration
        "path_hbm_roofline": (lambda b: {"algorithmic_bytes_per_ray": b, "rays_per_s_at_8TBps": 8e12 / b * world,
                                         "frac": (total_rays / elapsed) / (8e12 / b * world)})(
            72.0 + 28.0 * float(spec.n_params) / max(total_rays / max(args.steps, 1) / world, 1.0)),
        "kernels_ms": {k: v["avg_ms"] for k, v in kernels.items()},
        "ops_ms": {k: round(v["avg_ms"], 4) for k, v in ksum.items()},
        "final_loss": final_loss,
        "l1_depth_m": l1_depth, "iterations_trained": args.warmup + args.steps, "extended_run": extended,
        "other_dtype": other,
        "disclosures": {
            "table_gradient_records": "hash-table gradient contributions travel as 8-byte records whose two values are rounded to 26 bits "
                                      "(sign, 8 exponent, 17 mantissa bits; relative error <= 2^-18) before an exact 64-bit fixed-point sum - a "
                                      "sub-fp32 step inside the f32 mode (DESIGN.md 3.4; parity vs the fp32 oracle 2e-5)",
            "grid_position": "fma(x, scale, 0.5) as tiny-cuda-nn (one rounding); spec switch pos_rounding=mul_add for the other convention",
            "timed_region": "inputs resident in HBM (scans uploaded once per keyframe before the loop); no host sync inside the loop",
        },
    }
    if world == 1 and args.full and not args.no_cpu_baseline:
        print(json.dumps(line), file=sys.stderr, flush=True)          # progress copy: the legs below take minutes
        # baseline legs on the SAME workload, each bounded; then the HIP path's L1 after the same number of iterations as the CPU leg
        # BASELINE.md section 3 planned os.cpu_count() threads; torch's CPU ops on [4096,512] tensors do not scale that far on a 256-core
        # host, so the thread count is MEASURED: one iteration each at 16 / 64 / all cores, the fastest count runs the bounded sample
        # and all three timings are reported
        n_cpu = available_cores()
        probe = {}
        t_probe = time.time()
        for th in sorted({min(16, n_cpu), min(64, n_cpu), n_cpu}):
            if probe and time.time() - t_probe > 40.0:      # (the line must finish within minutes whatever the host does)
                break
            # (one iteration of a ONE-keyframe window - an eighth of the workload: a badly oversubscribed count costs seconds, not minutes)
            probe[th] = oracle_leg(_Shape(1, args.rays, args.samples), "cpu", budget_s=0.0, max_iters=1, min_iters=1, threads=th)["ms_per_iter"]
        best = min(probe, key=probe.get)
        print(f"bench.py: cpu thread probe {probe} ms per one-keyframe iteration in {time.time() - t_probe:.1f} s ({n_cpu} usable cores)", file=sys.stderr, flush=True)
        cpu = oracle_leg(args, "cpu", budget_s=12.0, max_iters=6, threads=best)
        cpu["threads_probe_ms_per_iter"] = {str(k): round(v, 1) for k, v in probe.items()}
        cpu["available_cores"] = n_cpu
        cpu["sample"] += (f"; thread count chosen by a one-iteration probe of a one-keyframe window at {sorted(probe)} threads (fastest: {best}; {n_cpu} cores usable "
                          f"by this process - affinity and cgroup quota - of the host's {os.cpu_count()})")
        try:
            rocm = oracle_leg(args, "cuda", budget_s=4.0, max_iters=max(cpu["iterations"], 3), min_iters=cpu["iterations"])
        except Exception as e:
            rocm = {"error": str(e)}
        line["cpu_baseline"] = cpu
        line["torch_rocm_baseline"] = rocm
        # "at matched L1 depth" (BASELINE.json metric).  Every leg trains the REDUCED configuration of the G13 fixture - the one on which the
        # REFERENCE's own optimiser was recorded (tests/golden/make_golden3.py: 30.0 m -> 14.55 m after 50, 10.86 m after 100 iterations) -
        # from the same initial parameters for the same number of iterations and is scored the same way.  100 Adam iterations turn
        # rounding and draw differences into different maps, so ONE run per leg says little (round 3: 9.5 / 11.1 / 12.4 m): the two GPU
        # legs run QUALITY_SEEDS times each, every run with its own random draws, and what is compared is the distribution -
        # "matched" = the HIP leg's mean L1 within one pooled standard deviation AND within 10 % of the torch-ROCm oracle leg's mean,
        # both below half of where they started.  The speed-ups on the full workload are reported as "at matched quality" only then.
        q = _Shape(QUALITY_SHAPE.keyframes, QUALITY_SHAPE.rays, QUALITY_SHAPE.samples)
        seeds = list(range(QUALITY_SEEDS))
        legs = {}
        try:
            legs["cpu_oracle"] = [oracle_leg(q, "cpu", budget_s=0.0, max_iters=QUALITY_ITERS, min_iters=QUALITY_ITERS, seed=0)]
        except Exception as e:
            legs["cpu_oracle"] = [{"error": str(e)}]
        legs["torch_rocm_oracle"] = []
        for sd in seeds:
            try:
                legs["torch_rocm_oracle"].append(oracle_leg(q, "cuda", budget_s=0.0, max_iters=QUALITY_ITERS, min_iters=QUALITY_ITERS, seed=sd))
            except Exception as e:
                legs["torch_rocm_oracle"].append({"error": str(e)})
        legs["hip_f32"] = []
        for sd in seeds:
            try:
                legs["hip_f32"].append(hip_quality_run(sd, device_index=local))
            except Exception as e:
                legs["hip_f32"].append({"error": str(e)})

        def stats_of(runs, key):
            v = [r[key] for r in runs if isinstance(r.get(key), float)]
            if not v:
                return None
            m = sum(v) / len(v)
            sdv = (sum((x - m) ** 2 for x in v) / (len(v) - 1)) ** 0.5 if len(v) > 1 else None
            return {"n": len(v), "mean": m, "sd": sdv, "min": min(v), "max": max(v), "runs": [round(x, 4) for x in v]}
        after = {k: stats_of(v, "l1_depth_m_after") for k, v in legs.items()}
        before = {k: stats_of(v, "l1_depth_m_before") for k, v in legs.items()}
        hs, rs = after.get("hip_f32"), after.get("torch_rocm_oracle")
        matched, detail = False, {}
        if hs and rs and hs["sd"] is not None and rs["sd"] is not None:
            pooled = (((hs["n"] - 1) * hs["sd"] ** 2 + (rs["n"] - 1) * rs["sd"] ** 2) / max(hs["n"] + rs["n"] - 2, 1)) ** 0.5
            diff = hs["mean"] - rs["mean"]
            off_plateau = all(a and b and a["max"] < 0.5 * b["mean"] for a, b in ((after[k], before[k]) for k in ("hip_f32", "torch_rocm_oracle")))
            detail = {"mean_difference_m": diff, "pooled_sd_m": pooled, "relative_difference": diff / rs["mean"],
                      "within_one_pooled_sd": abs(diff) <= pooled, "within_10pct": abs(diff) <= 0.10 * rs["mean"],
                      "all_runs_below_half_of_initial": bool(off_plateau),
                      "hip_mean_vs_reference_curve": hs["mean"] / QUALITY_REFERENCE["l1_after_100_iterations_m"] - 1.0}
            matched = bool(detail["within_one_pooled_sd"] and detail["within_10pct"] and off_plateau)
        ms_of = lambda runs: (lambda v: sum(v) / len(v) if v else None)([r["ms_per_iter"] for r in runs if isinstance(r.get("ms_per_iter"), float)])
        rate_of = lambda runs: (lambda v: sum(v) / len(v) if v else None)([r["value"] for r in runs if isinstance(r.get("value"), float)])
        line["matched_quality"] = {
            "config": f"{q.keyframes} keyframes x {q.rays} rays x {q.samples} samples, default network, joint map + pose optimisation, {QUALITY_ITERS} iterations",
            "runs_per_leg": {k: len(v) for k, v in legs.items()}, "reference": QUALITY_REFERENCE,
            "l1_depth_m_before": before, "l1_depth_m_after": after, "rays": L1_RAYS,
            "rays_per_s": {k: rate_of(v) for k, v in legs.items()}, "ms_per_iter": {k: ms_of(v) for k, v in legs.items()},
            "comparison_hip_vs_torch_rocm": detail, "matched": matched,
            "errors": [r["error"] for v in legs.values() for r in v if "error" in r],
            "note": "L1 depth with analysis/compute_l1_depth.py semantics (Model.forward(testing=True), 256 samples, the same held-out rays "
                    "of keyframe 0, the same probe seed) before and after the SAME number of iterations from the same initial parameters; the GPU "
                    f"legs {QUALITY_SEEDS} runs each with different random draws (HIP: the in-kernel generator, tests/test_gpu_rng.py), the CPU leg one run; "
                    "tests/test_gpu_mapping.py::test_l1_depth_curve_matches_the_reference_on_its_own_draws ties the HIP path to the reference's own curve"}
        # ... and ONE pair of runs at the headline workload itself: 25 iterations of the whole window from the same
        # initial parameters, the HIP path against the oracle's torch ops on the same MI355X, scored on the same 512 rays.  One run per
        # leg (the torch leg costs ~0.85 s per iteration): reported, with the 10 % band as a flag, not folded into `matched`.
        try:
            t_hw = time.time()
            hw_it = 25
            hw_shape = _Shape(args.keyframes, args.rays, args.samples)
            hw_hip = hip_quality_run(0, iters=hw_it, shape=hw_shape, device_index=local)
            hw_ref = oracle_leg(hw_shape, "cuda", budget_s=0.0, max_iters=hw_it, min_iters=hw_it, seed=0)
            hw_rel = hw_hip["l1_depth_m_after"] / hw_ref["l1_depth_m_after"] - 1.0
            line["matched_quality"]["headline_workload"] = {
                "config": f"{hw_shape.keyframes} keyframes x {hw_shape.rays} rays x {hw_shape.samples} samples, {hw_it} iterations, one run per leg",
                "l1_depth_m_before": {"hip_f32": hw_hip["l1_depth_m_before"], "torch_rocm_oracle": hw_ref["l1_depth_m_before"]},
                "l1_depth_m_after": {"hip_f32": hw_hip["l1_depth_m_after"], "torch_rocm_oracle": hw_ref["l1_depth_m_after"]},
                "relative_difference": hw_rel, "within_10pct": abs(hw_rel) <= 0.10,
                "ms_per_iter": {"hip_f32": hw_hip["ms_per_iter"], "torch_rocm_oracle": hw_ref["ms_per_iter"]}}
            print(f"bench.py: headline-workload quality pair in {time.time() - t_hw:.1f} s", file=sys.stderr, flush=True)
        except Exception as e:
            line["matched_quality"]["headline_workload"] = {"error": str(e)}
        # speed-ups: on the full workload only as "same workload" figures with the quality flag beside them; "at matched quality" on the
        # configuration where quality was actually compared
        line["quality_matched"] = matched
        if matched:
            hv, cv, rv = rate_of(legs["hip_f32"]), rate_of(legs["cpu_oracle"]), rate_of(legs["torch_rocm_oracle"])
            line["matched_quality"]["speedup_at_matched_quality"] = {"vs_cpu_oracle": hv / cv if cv else None, "vs_torch_rocm_oracle": hv / rv if rv else None}
            line["speedup_vs_cpu_oracle_same_workload"] = line["value"] / cpu["value"] if args.dtype == "f32" else None
            if isinstance(rocm.get("value"), float):
                line["speedup_vs_torch_rocm_oracle_same_workload"] = line["value"] / rocm["value"]
    print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
