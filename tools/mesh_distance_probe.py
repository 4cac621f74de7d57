"""Point-to-mesh query costs (profiles/mesh_distance.txt): on the marching-cubes mesh of the trained synthetic map
(tools/raycast_probe.py's scene) at 0.1 m and on its 0.3 m simplification, with clouds of about 1 M surface samples of the other mesh
as queries: the time and node visits per query of compute_distance and compute_occupancy, evaluate_mesh_to_mesh end to end, and
beside it the sampled route evaluate_mesh takes to the same accuracy figure (sample the ground-truth mesh at mesh_eval's defaults,
50 M points down-sampled at 0.05 m, build the NNGrid, query it) with the difference between the two figures.

    python tools/mesh_distance_probe.py [--out FILE] [--resolution 0.1] [--iterations 150] [--voxel 0.3] [--points 1000000]

Every kernel figure: device events around one call after two warm-up calls, 9 calls, median and minimum; a call includes its output
allocations.  The end-to-end figures are host clocks around one call between device synchronisations, after one warm-up call.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.raycast_probe import timed  # noqa: E402


def wall(fn, warm=1):
    """(seconds, result) of one call by the host clock, the device idle before and after"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--resolution", type=float, default=0.1)
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--points", type=int, default=1_000_000)
    args = ap.parse_args()
    from loner_amd import ops
    from loner_amd.analysis import mesh_eval
    from loner_amd.analysis.mesher import Mesher, TriangleMesh
    from loner_amd.analysis.raycast import RaycastingScene
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import OptimizationSettings, Optimizer
    from loner_amd.utils import synthetic as SY
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
    del opt, mesher
    torch.cuda.empty_cache()
    say(f"# python tools/mesh_distance_probe.py --resolution {args.resolution} --iterations {args.iterations} --voxel {args.voxel} "
        f"--points {args.points}")
    say(f"# point-to-mesh queries on one MI355X ({torch.cuda.get_device_name(0)}); device events around single calls after 2 warm-up")
    say("# calls, 9 calls: median (minimum) ms.  Queries are uniform surface samples of the OTHER mesh, in sample order")
    scenes = {"full": RaycastingScene(full, device=dev), "small": RaycastingScene(small, device=dev)}
    names = {"full": f"{args.resolution} m mesh", "small": f"its {args.voxel} m simplification"}
    n = args.points
    for key, other in (("full", "small"), ("small", "full")):
        scene = scenes[key]
        q = ops.mesh_sample_points(scenes[other].vertices, scenes[other].triangles, n, 0)
        say(f"{names[key]}: {scene.vertices.shape[0]} vertices, {scene.triangles.shape[0]} triangles, depth {scene.bvh.depth}; "
            f"{q.shape[0]} queries on {names[other]}")
        stats = {}
        d = scene.compute_distance(q, stats=stats)
        med, low = timed(lambda: scene.compute_distance(q))
        say(f"  compute_distance: {med:.3f} ({low:.3f}) ms = {q.shape[0] / med / 1e3:.1f} M queries/s, "
            f"{stats['node_visits'] / q.shape[0]:.1f} node visits per query; mean distance {float(d.mean()):.6f} m")
        box_lo, box_hi = scene.vertices.min(0).values, scene.vertices.max(0).values
        p = box_lo + (box_hi - box_lo) * torch.rand(n, 3, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(1))
        stats = {}
        d = scene.compute_distance(p, stats=stats)
        med, low = timed(lambda: scene.compute_distance(p))
        say(f"  compute_distance, {n} uniform points of the mesh's box: {med:.3f} ({low:.3f}) ms, "
            f"{stats['node_visits'] / n:.1f} node visits per query; mean distance {float(d.mean()):.4f} m")
        for nsamples in (1, 3):
            stats = {}
            occ = scene.compute_occupancy(p, nsamples, stats=stats)
            med, low = timed(lambda: scene.compute_occupancy(p, nsamples))
            say(f"  compute_occupancy(nsamples={nsamples}), the same points: {med:.3f} ({low:.3f}) ms = {n / med / 1e3:.1f} M points/s, "
                f"{stats['node_visits'] / (n * nsamples):.1f} node visits per ray; {float(occ.mean()):.4f} of the points inside (the mesh "
                "of a room seen from inside is not closed: a figure, not a truth)")
    say("# evaluate_mesh_to_mesh(estimate = the simplification, ground truth = the full mesh): host clock around one call")
    sec, got = wall(lambda: mesh_eval.evaluate_mesh_to_mesh(small, full, 0.1, n, 0, dev))
    say(f"from two TriangleMeshes (uploads, both BVH builds, 2 x {n} samples, 2 x {n} queries): {sec * 1e3:.1f} ms")
    sec2, got2 = wall(lambda: mesh_eval.evaluate_mesh_to_mesh(scenes["small"], scenes["full"], 0.1, n, 0))
    assert got2 == got
    say(f"from two ready scenes: {sec2 * 1e3:.1f} ms")
    say("  " + ", ".join(f"{k} {v:.6f}" if isinstance(v, float) else f"{k} {v}" for k, v in got.items()))
    say("# the sampled route to the accuracy figure (evaluate_mesh's defaults: 50 M samples of the ground-truth mesh, voxel_down_sample")
    say("# at 0.05 m; then NNGrid build and distance of the same estimate samples)")
    est = ops.mesh_sample_points(scenes["small"].vertices, scenes["small"].triangles, n, 0)

    def sampled_cloud():
        cloud = full.sample_points_uniformly(50_000_000, seed=0, device=dev)
        return cloud.voxel_down_sample(0.05)

    sec_cloud, cloud = wall(sampled_cloud)
    sec_grid, grid = wall(lambda: ops.NNGrid(cloud.points))
    sec_dist, dist = wall(lambda: grid.distance(est))
    sampled = float(dist.mean())
    say(f"sample + down-sample: {sec_cloud * 1e3:.1f} ms -> {len(cloud)} points; NNGrid build {sec_grid * 1e3:.1f} ms; distance of {n} "
        f"queries {sec_dist * 1e3:.1f} ms; total {(sec_cloud + sec_grid + sec_dist) * 1e3:.1f} ms")
    say(f"accuracy: sampled route {sampled:.6f} m, exact {got['accuracy']:.6f} m, difference {sampled - got['accuracy']:+.6f} m "
        f"({(sampled - got['accuracy']) / got['accuracy'] * 100:+.1f} %)")
    exact = scenes["full"].compute_distance(est)
    say(f"per query: max (sampled - exact) {float((dist - exact).max()):.6f} m, min {float((dist - exact).min()):.3e} m (a down-sampled "
        "point is the mean of a voxel's samples and lies off the surface, so the sampled figure can fall below the exact one)")
    # the 50 M samples themselves lie on the surface: no point of it can be nearer than the surface is, at 7 M triangles too
    raw = ops.NNGrid(full.sample_points_uniformly(50_000_000, seed=0, device=dev).points).distance(est)
    say(f"against the 50 M samples before down-sampling: mean {float(raw.mean()):.6f} m, max (sampled - exact) "
        f"{float((raw - exact).max()):.6f} m, min {float((raw - exact).min()):.3e} m")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
