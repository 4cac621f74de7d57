"""Depth-image costs (profiles/camera_render.txt), device events after a warm-up, on the synthetic map trained for 150 iterations:
a 384 x 512 image (the lidar-only default camera) at N_samples_test = 2048, from one camera pose.
  1. the ray build (lnr_build_camera_rays) against the same records built with torch ops on the device;
  2. Model.render_depth_peak (no [N,S] array kept) against the route it replaces, whose code this probe does not touch:
     forward(testing=True) with retraw, argmax of weights_fine, gather from samples_fine - the two alternated in one process, each
     with its peak of torch.cuda.max_memory_allocated;
  3. the colour map (lnr_depth_colormap) and the PNG encoder on the host.

    python tools/probe_camera_render.py [--out FILE] [--reps N] [--train-iterations N]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def torch_rays(directions, width, T, range_min, scale, shift):
    """CameraRayDirections.build_rays of the reference (ray_utils.py:175-213) in torch ops on the device"""
    T = T.clone()
    T[:3, 3] = (T[:3, 3] + shift) / scale
    d = directions @ T[:3, :3].T
    d = d / torch.norm(d, dim=-1, keepdim=True)
    o = T[:3, 3].expand_as(d)
    dd = d + 1e-15
    far = torch.maximum(((-1.0 - o) / dd).clamp(min=0), ((1.0 - o) / dd).clamp(min=0)).min(dim=1, keepdim=True).values
    idx = torch.arange(d.shape[0], device=d.device)
    near = (range_min / scale) * torch.ones_like(far)
    return torch.cat([o, d, -d, (idx % width).float()[:, None], (idx // width).float()[:, None], near, far], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--train-iterations", type=int, default=150)
    args = ap.parse_args()
    from loner_amd.analysis.renderer import DepthRenderer, depth_to_rgba, write_png
    from loner_amd.common.pose import Pose
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import OptimizationSettings, Optimizer
    from loner_amd.utils import synthetic as SY
    from tests.test_gpu_mapping import make_keyframes
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    say(f"device: {torch.cuda.get_device_name(0)}")
    scale, shift = SY.world_cube()
    wc = WorldCube(torch.tensor(scale), torch.from_numpy(shift))
    s = default_optimizer_settings()
    s["num_samples"]["sky"] = 0
    torch.manual_seed(0)
    opt = Optimizer(s, None, wc, 0, False, True, False)
    kf = make_keyframes([SY.trajectory_pose6(1)[0]])[0]
    opt._do_iterate_optimizer([kf], [None], optimizer_settings=OptimizationSettings(args.train_iterations, True, False, False, True))
    model, sampler = opt._model, opt._ray_sampler
    model.cfg["render"]["N_samples_test"] = 2048
    assert model._sample_counts(True)[0] == 2048
    r = DepthRenderer(model, {"poses": []}, wc, torch.tensor([1.0, 50.0]))
    H, W = r.im_size
    cam = r.camera_pose(Pose(pose_tensor=SY.trajectory_pose6(1)[0].clone())).to(dev)
    crd = r.ray_directions
    say(f"image {H} x {W} = {H * W} rays, N_samples_test 2048, map trained for {args.train_iterations} iterations")

    # 1. rays
    build = lambda: crd.build_rays(None, cam, None, wc, r.ray_range)[0]
    T = cam.get_transformation_matrix().to(dev).float()
    shift_d, scale_d = wc.shift.to(dev).float(), torch.tensor(float(wc.scale_factor), device=dev)
    by_torch = lambda: torch_rays(crd.directions, W, T, 1.0, scale_d, shift_d)
    rays = build()
    ref = by_torch()
    err = float(((rays - ref).abs().max(0).values / ref.abs().max(0).values.clamp_min(1e-30)).max())
    t_new, t_old = timed(build, 20), timed(by_torch, 20)
    say(f"1. ray build: lnr_build_camera_rays (with the host side of build_rays) {t_new:.3f} ms; torch ops on the device {t_old:.3f} ms "
        f"(ratio {t_old / t_new:.2f}); largest relative difference per column {err:.2e}")

    # 2. render: the two routes alternated
    def new_route():
        return model.render_depth_peak(rays, sampler)

    def old_route():
        with torch.no_grad():
            out = model(rays, sampler, wc.scale_factor, testing=True, camera=False)
        s_vals, w = out["samples_fine"], out["weights_fine"]
        return out["depth_fine"], s_vals[torch.arange(rays.shape[0], device=dev), w.argmax(dim=1)]

    torch.manual_seed(1)
    a = new_route()
    torch.manual_seed(1)
    b = old_route()
    same = bool(torch.equal(a[0], b[0])) and bool(torch.equal(a[1], b[1]))
    del a, b
    torch.cuda.synchronize()
    t = {"new": [], "old": []}
    mem = {}
    for _ in range(args.reps):
        for name, fn in (("new", new_route), ("old", old_route)):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t[name].append(timed(fn, 1))
            mem[name] = torch.cuda.max_memory_allocated() - base
    tn, to = min(t["new"]), min(t["old"])
    say(f"2. render_depth_peak {tn:.1f} ms (runs: {', '.join(f'{x:.1f}' for x in t['new'])}), peak memory above the resident state "
        f"{mem['new'] / 2 ** 20:.0f} MiB")
    say(f"   forward(testing=True) + argmax + gather {to:.1f} ms (runs: {', '.join(f'{x:.1f}' for x in t['old'])}), peak memory "
        f"{mem['old'] / 2 ** 20:.0f} MiB")
    say(f"   ratio old / new {to / tn:.3f}; memory difference {(mem['old'] - mem['new']) / 2 ** 20:.0f} MiB; same seed, same depth and "
        f"peak bit for bit: {same}")

    # 3. colour and PNG
    depth, _ = r.render_frame(cam, sampler, consistency=False)
    rgba = depth_to_rgba(depth, max_depth=75)
    t_col = timed(lambda: depth_to_rgba(depth, max_depth=75), 50)
    t0 = time.perf_counter()
    write_png(os.devnull, rgba)
    t_png = 1e3 * (time.perf_counter() - t0)
    say(f"3. lnr_depth_colormap {1e3 * t_col:.1f} us for {H * W} pixels ({8 * H * W / t_col / 1e6:.1f} GB/s of 8 B per pixel); "
        f"copy to the host + PNG encoding (zlib level 6) {t_png:.1f} ms on the host")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
