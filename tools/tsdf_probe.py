"""TSDF fusion costs (profiles/tsdf.txt): on the synthetic room with its sphere (utils/synthetic_mesh.scene_mesh) at a voxel size of
0.1 m over the scene's box grown by 1 m, the integration of one simulated 64 x 1024 and one 128 x 2048 sweep, band only and carving,
with node updates per ray and per second; the field and the masked marching cubes over the fused volume; and fuse_scans plus
extract_mesh for the twelve-frame sequence examples/simulate_sequence.py writes by default.

    python tools/tsdf_probe.py [--out FILE] [--voxel 0.1] [--append FILE]

Every kernel figure: device events around one call after two warm-up calls, 9 calls, median and minimum; a call includes its output
allocations.  The end-to-end figure is a host clock around one call between device synchronisations, after one warm-up call.  Beside
each stands the time of the numpy restatement (tests/tsdf_restatement.py) on the same input, on this host's CPU; the restated
integration walks its rays in Python, so it is timed on every --stride-th ray and scaled.  --append: a text file (the closed-loop
run's output, examples/run_sequence.py --gt --gt-mesh --tsdf-baseline) copied to the end of the report.
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mesh_distance_probe import wall  # noqa: E402
from tools.raycast_probe import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", default=None)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--stride", type=int, default=64)
    args = ap.parse_args()
    from examples.simulate_sequence import default_trajectory
    from loner_amd import ops
    from loner_amd.analysis import lidar_sim
    from loner_amd.analysis.gt_map import load_trajectory
    from loner_amd.analysis.mesh_eval import evaluate_mesh_to_mesh
    from loner_amd.analysis.mesher import TriangleMesh
    from loner_amd.analysis.raycast import RaycastingScene
    from loner_amd.analysis.tsdf import TSDFVolume, fuse_scans
    from loner_amd.utils import synthetic as SY
    from loner_amd.utils import synthetic_mesh as SM
    from tests import tsdf_restatement as TR
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    v = args.voxel
    vertices, triangles = SM.scene_mesh()
    scene = RaycastingScene(vertices, triangles, device=dev)
    bound = (vertices.min(axis=0) - 1.0, vertices.max(axis=0) + 1.0)
    rows = default_trajectory(12, 0.1)
    traj = load_trajectory(rows, dev)
    say(f"# python tools/tsdf_probe.py --voxel {v} --stride {args.stride}")
    say(f"# TSDF fusion on one MI355X ({torch.cuda.get_device_name(0)}); device events around single calls after 2 warm-up calls, 9 calls:")
    say("# median (minimum) ms.  Beside each: the numpy restatement (tests/tsdf_restatement.py) on the same input on the host CPU")
    probe = TSDFVolume(*bound, v, device=dev)
    say(f"volume: {' x '.join(map(str, probe.dims))} = {np.prod(probe.dims) / 1e6:.1f} M nodes at {v} m, trunc {probe.sdf_trunc:.2f} m, "
        f"{(probe.sum.numel() * 12) / 2 ** 20:.0f} MiB (int64 sum, uint32 count)")
    for beams, azimuths in ((64, 1024), (128, 2048)):
        d, times = SY.lidar_pattern(beams, azimuths)
        scan, _ = lidar_sim.simulate_scan(scene, traj, d.to(dev), times.to(dev), 0.3, (1.0, 50.0))
        rays, _ = ops.trajectory_rays(scan.ray_directions, scan.timestamps.double(), traj)
        ranges = scan.distances.double()
        n = rays.shape[0]
        for what, front in (("band only (front = trunc)", probe.sdf_trunc), ("carving (front = inf)", math.inf)):
            vol = TSDFVolume(*bound, v, front=front, device=dev)
            got = vol.integrate_rays(rays, ranges)
            med, low = timed(lambda: ops.tsdf_integrate(rays, ranges, vol.sum, vol.count, vol.origin, v, vol.sdf_trunc, front))
            sub_rays, sub_ranges = rays[::args.stride].cpu().numpy(), ranges[::args.stride].cpu().numpy()
            t0 = time.perf_counter()
            TR.integrate(sub_rays, sub_ranges, vol.dims, vol.origin, v, vol.sdf_trunc, front)
            host = (time.perf_counter() - t0) * n / sub_rays.shape[0]
            say(f"integrate, {beams} x {azimuths} sweep ({n} returns), {what}: {med:.3f} ({low:.3f}) ms, "
                f"{got['node_updates'] / n:.1f} node updates per ray, {got['node_updates'] / med / 1e6:.2f} G updates/s, "
                f"{n / med / 1e3:.1f} M rays/s; {got['missed_rays']} rays miss, {got['invalid_rays']} invalid; "
                f"restatement {host:.1f} s (every {args.stride}th ray, scaled)")
            del vol
    del probe
    # the twelve-frame sequence of examples/simulate_sequence.py's defaults, fused along its ground truth
    d, times = SY.lidar_pattern(64, 1024)
    scans = [lidar_sim.simulate_scan(scene, traj, d.to(dev), times.to(dev), 0.1 * k, (1.0, 50.0), 0.0, k)[0] for k in range(12)]

    def fuse_and_mesh():
        volume = fuse_scans(scans, rows, bound, v, device=dev)
        return volume, volume.extract_mesh()

    seconds, (volume, mesh) = wall(fuse_and_mesh)
    say(f"fuse_scans + extract_mesh, 12 sweeps of 64 x 1024 along the ground truth, band only: {seconds * 1e3:.1f} ms by the host clock "
        f"({volume.n_rays} rays; {mesh.vertices.shape[0]} vertices, {mesh.triangles.shape[0]} triangles)")
    med, low = timed(lambda: volume.field())
    field, valid = volume.field()
    say(f"field + valid over the fused volume: {med:.3f} ({low:.3f}) ms; {int(valid.sum())} nodes observed "
        f"({float(valid.float().mean()) * 100:.2f} %)")
    med, low = timed(lambda: ops.marching_cubes(field, 0.0, volume.spacing, volume.origin, valid=valid))
    say(f"masked marching cubes: {med:.3f} ({low:.3f}) ms")
    med, low = timed(lambda: ops.marching_cubes(field, 0.0, volume.spacing, volume.origin))
    say(f"  unmasked, the same field (zeros where nothing was observed): {med:.3f} ({low:.3f}) ms")
    sum_h, count_h = volume.sum.cpu().numpy(), volume.count.view(torch.int32).cpu().numpy().view(np.uint32)
    t0 = time.perf_counter()
    field_h, valid_h = TR.field(sum_h, count_h)
    t1 = time.perf_counter()
    want = TR.marching_cubes_masked(field_h, valid_h, 0.0, ops.mc_case_table(), volume.spacing, volume.origin)
    t2 = time.perf_counter()
    same = want[0].tobytes() == ops.marching_cubes(field, 0.0, volume.spacing, volume.origin, valid=valid)[0].cpu().numpy().tobytes()
    say(f"  restatement: field {(t1 - t0) * 1e3:.0f} ms, masked marching cubes {(t2 - t1) * 1e3:.0f} ms (vertices "
        f"{'equal' if same else 'DIFFER'} byte for byte)")
    score = evaluate_mesh_to_mesh(mesh, TriangleMesh(vertices, triangles), device=dev)
    say("the ground-truth fusion against the scene's mesh (exact distances, m; shares at 0.1 m): " +
        ", ".join(f"{k} {score[k]:.4f}" for k in ("accuracy", "completion", "chamfer", "precision", "recall", "f_score")))
    if args.append and os.path.exists(args.append):
        say("# the closed loop: TriangleMesh(*scene_mesh()).write_ply(<mesh.ply>), then examples/simulate_sequence.py <folder> --mesh <mesh.ply>")
        say("# --frames 12, then examples/run_sequence.py <folder> --gt <folder>/gt_tum.txt --gt-mesh <mesh.ply> --tsdf-baseline")
        for line in open(args.append).read().splitlines():
            say(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
