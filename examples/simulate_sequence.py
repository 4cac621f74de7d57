"""Simulate a LiDAR flying through a triangle mesh and write the folder examples/run_sequence.py reads.

    python examples/simulate_sequence.py <out folder> [--mesh mesh.ply] [--trajectory poses_tum.txt] [--frames 12]
                                         [--beams 64] [--azimuths 1024] [--scan-period 0.1] [--ray-range 1 50] [--range-sigma 0] [--seed 0]

Without --mesh the scene is the synthetic room with its sphere (loner_amd.utils.synthetic_mesh.scene_mesh).  Without --trajectory the
sensor drives --frames scan periods along x from (-4, -2, 0.5) at 1 m/s while it yaws at 10 degrees per second.  Every ray is cast
from the pose at its own time, so the scans are motion-distorted exactly as a moving sensor's are; the folder also gets gt_tum.txt,
the pose at every scan stamp:

    python examples/run_sequence.py <out folder> --gt <out folder>/gt_tum.txt
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loner_amd.analysis.lidar_sim import simulate_sequence          # noqa: E402
from loner_amd.analysis.mesher import TriangleMesh                  # noqa: E402
from loner_amd.analysis.raycast import RaycastingScene              # noqa: E402
from loner_amd.common.pose_utils import read_tum                    # noqa: E402
from loner_amd.utils.synthetic import lidar_pattern                 # noqa: E402
from loner_amd.utils.synthetic_mesh import scene_mesh               # noqa: E402


def default_trajectory(frames, scan_period, speed=1.0, yaw_rate_deg=10.0, start=(-4.0, -2.0, 0.5)):
    """TUM rows: one pose per scan period (and two more, so that the last sweep ends inside the trajectory)"""
    rows = []
    for k in range(frames + 2):
        t = k * scan_period
        half = math.radians(yaw_rate_deg) * t / 2.0
        rows.append([t, start[0] + speed * t, start[1], start[2], 0.0, 0.0, math.sin(half), math.cos(half)])
    return np.asarray(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--mesh")
    ap.add_argument("--trajectory")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuths", type=int, default=1024)
    ap.add_argument("--scan-period", type=float, default=0.1)
    ap.add_argument("--ray-range", type=float, nargs=2, default=(1.0, 50.0))
    ap.add_argument("--range-sigma", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if args.mesh:
        mesh = TriangleMesh.read_ply(args.mesh)
        scene = RaycastingScene(mesh)
    else:
        scene = RaycastingScene(*scene_mesh())
    rows = read_tum(args.trajectory) if args.trajectory else default_trajectory(args.frames, args.scan_period)
    pattern = lidar_pattern(args.beams, args.azimuths)
    stamps = simulate_sequence(scene, rows, args.out, pattern, scan_period=args.scan_period, n_scans=args.frames,
                               ray_range=tuple(args.ray_range), range_sigma=args.range_sigma, seed=args.seed)
    print(f"{len(stamps)} scans of {scene.triangles.shape[0]} triangles (BVH depth {scene.bvh.depth}) written to {args.out}")


if __name__ == "__main__":
    main()
