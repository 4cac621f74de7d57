"""Map rendering and evaluation costs (profiles/lidar_map.txt), device events after a warm-up:
  1. per pose at 450 x 3600 rays, N_samples_test = 2048 (default network, untrained): the render alone against scan points plus the
     per-scan voxel down-sample;
  2. voxel_down_sample at 1.6, 16 and 64 M points: ms and modelled HBM bytes per second;
  3. both distance passes of compare_point_clouds for the synthetic box scene at v = 0.05 (grid edge 2 v): ms, shells, fallback
     fraction, and scipy's cKDTree with workers=16 on the host for scale;
  4. the worst case: two disjoint clouds of 10^6 points (every query takes the exact pass).

    python tools/probe_lidar_map.py [--out FILE] [--skip-render] [--skip-kdtree]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def vds_bytes(n, k, bits):
    """modelled HBM traffic of one voxel_down_sample: bound (24 B/pt), keys (24 read + 12 written), per digit pass count (8) and
    scatter (12 + 12), heads (8 + 4), scan (8), starts (4 + 4), the averaging gather (4 + 24) and the output (24 per voxel)"""
    passes = (bits + 7) // 8
    return n * (24 + 36 + passes * 32 + 12 + 8 + 8 + 28) + 24 * k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-render", action="store_true")
    ap.add_argument("--skip-kdtree", action="store_true")
    args = ap.parse_args()
    from loner_amd import ops
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    say(f"device: {torch.cuda.get_device_name(0)}")

    if not args.skip_render:
        from loner_amd.analysis.lidar_map import LidarMapRenderer
        from loner_amd.common.pose import Pose
        from loner_amd.common.pose_utils import WorldCube
        from loner_amd.common.settings import default_optimizer_settings
        from loner_amd.mapping.optimizer import Optimizer
        from loner_amd.utils import synthetic as SY
        scale, shift = SY.world_cube()
        wc = WorldCube(torch.tensor(scale), torch.from_numpy(shift))
        s = default_optimizer_settings()
        s["num_samples"]["sky"] = 0
        torch.manual_seed(0)
        opt = Optimizer(s, None, wc, 0, False, True, False)
        model, sampler = opt._model, opt._ray_sampler
        model.cfg.render["N_samples_test"] = 2048
        r = LidarMapRenderer(model, {"poses": []}, wc, torch.tensor([1.0, 50.0]), resolution=0.1)
        pose = Pose(pose_tensor=SY.trajectory_pose6(1)[0].clone()).to(dev)
        rays, kept, dirs = r.scan_rays(pose)
        scale32, var_max, depth_max = r._thresholds(1e9)
        with torch.no_grad():
            render = lambda: model(rays, sampler, wc.scale_factor, testing=True, return_variance=True, camera=False)
            t_render = timed(render, 1)
            out = render()
        pts_count = {}

        def points_and_downsample():
            p, c = ops.lidar_scan_points(out["depth_fine"], out["variance"], kept, dirs, scale32, var_max, depth_max)
            pts_count["k"] = ops.voxel_down_sample(p, 0.05, c).shape[0]
        t_new = timed(points_and_downsample, 5)
        say(f"1. per pose, {rays.shape[0]} rays kept of {dirs.shape[1]}, N_samples_test 2048: render {t_render:.1f} ms; scan points + "
            f"per-scan voxel_down_sample(0.05) {t_new:.3f} ms ({100 * t_new / t_render:.3f} % of the render), {pts_count['k']} voxels "
            f"(every ray kept: variance bound 1e9)")
        del out, rays

    g = torch.Generator(device=dev).manual_seed(1)
    for n in (1_600_000, 16_000_000, 64_000_000):
        # a scan-like cloud: points on a sphere shell of radius 5..30 m, voxel 0.05
        d = torch.randn(n, 3, device=dev, dtype=torch.float64, generator=g)
        d = d / d.norm(dim=1, keepdim=True) * (5.0 + 25.0 * torch.rand(n, 1, device=dev, dtype=torch.float64, generator=g))
        k = ops.voxel_down_sample(d, 0.05).shape[0]
        t = timed(lambda: ops.voxel_down_sample(d, 0.05), 3)
        bits = sum(int(np.ceil(np.log2(np.floor(60.0 / 0.05) + 1))) for _ in range(3))
        say(f"2. voxel_down_sample n={n}: {t:.2f} ms, {k} voxels, {n / t / 1e6:.2f} G points/s, modelled traffic "
            f"{vds_bytes(n, k, bits) / t / 1e6:.0f} GB/s ({bits}-bit key)")
        del d

    # the synthetic box scene's surfaces at 0.05 against a noisy copy (about 1.4 M points each after down-sampling)
    from tests.test_gpu_lidar_map import _gt_cloud
    v = 0.05
    gt = torch.from_numpy(_gt_cloud(v)).to(dev)
    est = gt + 0.02 * torch.randn(gt.shape, device=dev, dtype=torch.float64, generator=g)
    gt_ds, est_ds = ops.voxel_down_sample(gt, v), ops.voxel_down_sample(est, v)
    for name, q, t_ in (("accuracy (est -> gt)", est_ds, gt_ds), ("completion (gt -> est)", gt_ds, est_ds)):
        st = {}

        def both():
            grid = ops.NNGrid(t_, 2 * v)
            grid.distance(q, stats=st)
        t = timed(both, 3)
        t_build = timed(lambda: ops.NNGrid(t_, 2 * v), 3)
        say(f"3. {name}: {q.shape[0]} queries, {t_.shape[0]} targets: {t:.2f} ms (grid build {t_build:.2f} ms), "
            f"{st['shells'] / q.shape[0]:.2f} shells per query, fallback {st['fallback'] / q.shape[0]:.2e}")
        if not args.skip_kdtree:
            from scipy.spatial import cKDTree
            qn, tn = q.cpu().numpy(), t_.cpu().numpy()
            t0 = time.perf_counter()
            cKDTree(tn).query(qn, workers=16)
            say(f"   cKDTree build + query, workers=16, host: {1e3 * (time.perf_counter() - t0):.0f} ms")

    a = torch.rand(1_000_000, 3, device=dev, dtype=torch.float64, generator=g) * 10
    b = torch.rand(1_000_000, 3, device=dev, dtype=torch.float64, generator=g) * 10 + torch.tensor([100.0, 0, 0], device=dev,
                                                                                                     dtype=torch.float64)
    st = {}
    grid = ops.NNGrid(b)
    t = timed(lambda: grid.distance(a, stats=st), 1)
    say(f"4. disjoint clouds, 10^6 queries x 10^6 targets: {t:.0f} ms, fallback {st['fallback']} queries "
        f"({1e12 / (t * 1e-3) / 1e12:.2f} T pair distances/s)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
