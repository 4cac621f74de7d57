"""Ray casting costs (profiles/raycast.txt): on the marching-cubes mesh of the trained synthetic map (tests/test_gpu_mesh.py's scene,
one keyframe) at 0.1 m and on its 0.3 m simplification, the BVH build, and rays/s and node visits per ray for a 64 x 1024 scan, a
128 x 2048 scan and a 384 x 512 camera image from inside the room; and one simulated sweep (trajectory rays + cast + filter), which has
to cost less than the 100 ms it represents.

    python tools/raycast_probe.py [--out FILE] [--resolution 0.1] [--iterations 150] [--voxel 0.3] [--append FILE]

Every figure: device events around one call after two warm-up calls, 9 calls, median and minimum; a call includes its output
allocations (and, for the build, its workspace and its one host read).  --append: a text file (the closed-loop run's output) copied
to the end of the report.
"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=9, warm=2):
    """(median ms, min ms) of single calls by device events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", default=None)
    ap.add_argument("--resolution", type=float, default=0.1)
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--voxel", type=float, default=0.3)
    args = ap.parse_args()
    from loner_amd import ops
    from loner_amd.analysis import lidar_sim
    from loner_amd.analysis.gt_map import load_trajectory
    from loner_amd.analysis.mesher import Mesher, TriangleMesh
    from loner_amd.analysis.raycast import RaycastingScene
    from loner_amd.analysis.renderer import lidar_only_calibration
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.common.ray_utils import CameraRayDirections
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import OptimizationSettings, Optimizer
    from loner_amd.utils import synthetic as SY
    from loner_amd.utils import synthetic_mesh as SM
    from tests.test_gpu_mapping import make_keyframes
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    s = default_optimizer_settings()
    s["num_samples"]["sky"] = 0
    torch.manual_seed(0)
    scale, shift = SY.world_cube()
    wc = WorldCube(torch.tensor(scale), torch.from_numpy(shift))
    opt = Optimizer(s, None, wc, 0, False, True, False)
    kf = make_keyframes([SY.trajectory_pose6(1)[0]])[0]
    opt._do_iterate_optimizer([kf], [None], optimizer_settings=OptimizationSettings(args.iterations, True, False, False, True))
    mcb = [[-21.0, 21.0], [-16.0, 16.0], [-3.0, 7.0]]
    mesher = Mesher(opt._model, {"poses": [kf.get_pose_state()]}, wc, torch.tensor([1.0, 50.0]), resolution=args.resolution,
                    marching_cubes_bound=mcb, level_set=0)
    torch.manual_seed(3)
    full = mesher.get_mesh(dev, opt._ray_sampler, skip_step=1)
    small = TriangleMesh(full.vertices, full.triangles).simplify_vertex_clustering(args.voxel, device=dev)
    say(f"# ray casting on one MI355X ({torch.cuda.get_device_name(0)}); device events around single calls after 2 warm-up calls, 9 calls:")
    say("# median (minimum) ms.  Rays leave from (0, 0, 1) inside the room; t window [0, inf)")
    cam = CameraRayDirections(lidar_only_calibration(), device=dev)
    yaw = math.radians(20.0)
    pose = torch.tensor([[math.cos(yaw), -math.sin(yaw), 0, 0.0], [math.sin(yaw), math.cos(yaw), 0, 0.0], [0, 0, 1, 1.0], [0, 0, 0, 1]],
                        dtype=torch.float64)
    # the camera of lidar_only_calibration looks along the lidar's x: its frame's z forward, x right, y down
    l2c = torch.tensor([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1.0]], dtype=torch.float64)

    def scan_rays(beams, azimuths):
        d, _ = SY.lidar_pattern(beams, azimuths)
        d = d.to(dev).double().T
        world = d @ pose[:3, :3].T.to(dev)
        return torch.cat([pose[:3, 3].to(dev).expand_as(world), world], dim=1).contiguous()

    for name, mesh in ((f"{args.resolution} m mesh", full), (f"its {args.voxel} m simplification", small)):
        v, t = torch.tensor(mesh.vertices, device=dev), torch.tensor(mesh.triangles, device=dev)
        med, low = timed(lambda: ops.BVH(v, t), reps=5, warm=1)
        bvh = ops.BVH(v, t)
        say(f"{name}: {v.shape[0]} vertices, {t.shape[0]} triangles; BVH build {med:.2f} ({low:.2f}) ms, depth {bvh.depth}, "
            f"{bvh.buf.numel() / 2 ** 20:.0f} MiB")
        scene = RaycastingScene(v, t)
        sets = (("64 x 1024 scan", scan_rays(64, 1024)), ("128 x 2048 scan", scan_rays(128, 2048)),
                ("384 x 512 camera image", scene.camera_rays(pose @ l2c, cam)))
        for what, rays in sets:
            stats = {}
            ops.cast_rays(scene.bvh, rays, stats=stats)
            med, low = timed(lambda: ops.cast_rays(scene.bvh, rays))
            n = rays.shape[0]
            say(f"  {what}: {n} rays, {stats['hits']} hits, {med:.3f} ({low:.3f}) ms = {n / med / 1e3:.1f} M rays/s, "
                f"{stats['node_visits'] / n:.1f} node visits per ray")
    say("# the neural render of the same rays, from README.md: a 64 x 1024 scan x 2048 samples 28.7 ms (profiles/r06_bench_default_run.log),")
    say("# a 384 x 512 image x 2048 samples 90.2 ms (profiles/camera_render.txt)")
    # one simulated sweep of the synthetic scene mesh along a moving trajectory: what simulate_sequence pays per scan before it writes
    scene = RaycastingScene(*SM.scene_mesh(), device=dev)
    rows = np.array([[0.1 * k, 1.0 * k, 0.0, 1.0, 0.0, 0.0, math.sin(math.radians(5.0) * k), math.cos(math.radians(5.0) * k)]
                     for k in range(3)])
    traj = load_trajectory(rows, dev)
    for beams, azimuths in ((64, 1024), (128, 2048)):
        d, times = SY.lidar_pattern(beams, azimuths)
        d, times = d.to(dev), times.to(dev)
        med, low = timed(lambda: lidar_sim.simulate_scan(scene, traj, d, times, 0.0, (1.0, 50.0)))
        say(f"simulate_scan, {beams} x {azimuths} rays on scene_mesh() ({scene.triangles.shape[0]} triangles), 1 m and 10 degrees of motion "
            f"in the sweep: {med:.3f} ({low:.3f}) ms against the 100 ms sweep it represents")
        med, low = timed(lambda: lidar_sim.simulate_scan(scene, traj, d, times, 0.0, (1.0, 50.0), 0.02, 1))
        say(f"  with range noise (sigma 0.02 m): {med:.3f} ({low:.3f}) ms")
    if args.append and os.path.exists(args.append):
        say("# the closed loop: examples/simulate_sequence.py, then examples/run_sequence.py --gt on its folder")
        for line in open(args.append).read().splitlines():
            say(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
