"""A simulated LiDAR: the scans a sensor would measure while it moves through a triangle mesh along a trajectory, with exact ground
truth.  Every ray leaves from the pose interpolated at the ray's own time (ops.trajectory_rays: include/loner_hip.h,
lnr_trajectory_rays) and is cast against the mesh (analysis/raycast.py), so the scans carry the motion distortion that the tracker's
and build_lidar_map's motion compensation undo: ops.trajectory_transform with the same trajectory is the exact inverse.

simulate_scan makes one LidarScan; simulate_sequence writes the folder examples/run_sequence.py reads (NNNNNN.npy of [N,4] x y z t,
stamps.txt) and the ground truth (gt_tum.txt).  A scan simulated this way also scores a trained map against a mesh with no further
code: compute_l1_depth compares the map's rendered depth with the scan's distances, which are the mesh's.

Not modelled: intensity, multiple echoes, beam divergence, the window of utils/synthetic.py's room.
"""
import math
import os

import numpy as np
import torch

from .. import ops
from ..common.sensors import LidarScan
from .gt_map import trajectory_arrays
from .renderer import Slerp, _interp_linear, _matrix_to_quat


def _check_pattern(directions, point_times, what):
    if not torch.is_tensor(directions) or directions.dim() != 2 or directions.shape[0] != 3 or directions.dtype != torch.float32:
        raise ValueError(f"{what}: directions fp32 [3,n], got "
                         f"{tuple(directions.shape) if torch.is_tensor(directions) else type(directions).__name__}")
    if not torch.is_tensor(point_times) or tuple(point_times.shape) != (directions.shape[1],):
        raise ValueError(f"{what}: point_times [{directions.shape[1]}], got "
                         f"{tuple(point_times.shape) if torch.is_tensor(point_times) else type(point_times).__name__}")


def _check_range(ray_range, range_sigma, seed, what):
    lo, hi = (float(x) for x in ray_range)
    if not (math.isfinite(lo) and lo >= 0 and hi > lo):
        raise ValueError(f"{what}: ray_range must be 0 <= min < max, got {ray_range!r}")
    sigma = float(range_sigma)
    if not (math.isfinite(sigma) and sigma >= 0):
        raise ValueError(f"{what}: range_sigma must be finite and >= 0, got {range_sigma!r}")
    if int(seed) != seed:
        raise ValueError(f"{what}: seed must be an integer, got {seed!r}")
    return lo, hi, sigma


def simulate_scan(scene, trajectory, directions, point_times, stamp, ray_range, range_sigma=0.0, seed=0):
    """One sweep -> (LidarScan, keep).  scene: a RaycastingScene; trajectory: an ops.Trajectory on the scene's device; directions
    [3,n] fp32 unit vectors in the sensor frame; point_times [n]: every ray's time relative to stamp (seconds); ray n is cast at the
    absolute time stamp + point_times[n] (fp64) from the pose interpolated there.  The distance of a ray is float32(t); with
    range_sigma > 0 a seeded normal draw on the device (torch.Generator(seed)) times range_sigma is added.  Rays that miss, leave
    ray_range = (min, max) or were cast outside the trajectory's time span are dropped, as a sensor driver drops no-returns: keep
    (bool [n]) marks the rays that stayed.  The scan holds the kept directions as given, the distances, and the timestamps
    float32(point_times) + float32(stamp) (what build_scan_from_points makes of local times); scan.primitive_ids (int32) names the
    triangle each kept ray hit."""
    _check_pattern(directions, point_times, "simulate_scan")
    lo, hi, sigma = _check_range(ray_range, range_sigma, seed, "simulate_scan")
    stamp = float(stamp)
    if not math.isfinite(stamp):
        raise ValueError(f"simulate_scan: stamp must be finite, got {stamp!r}")
    dev = scene.device
    dirs = directions.to(dev).contiguous()
    local = point_times.to(dev)
    rays, _ = ops.trajectory_rays(dirs, local.to(torch.float64) + stamp, trajectory)
    hit = scene.cast_rays(rays)
    dist = hit["t_hit"].to(torch.float32)
    if sigma > 0:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        dist = dist + sigma * torch.randn(dist.shape, generator=gen, device=dev, dtype=torch.float32)
    keep = torch.isfinite(dist) & (dist >= lo) & (dist <= hi)
    scan = LidarScan(dirs[:, keep].contiguous(), dist[keep].contiguous(),
                     (local.to(torch.float32) + torch.tensor(stamp, dtype=torch.float32, device=dev))[keep].contiguous())
    scan.primitive_ids = hit["primitive_ids"][keep]
    return scan, keep


def sequence_stamps(t0, t1, scan_period, sweep, n_scans=None):
    """The scan times t0 + k * scan_period whose whole sweep [stamp, stamp + sweep] lies inside [t0, t1] (at most n_scans of them)"""
    stamps, k = [], 0
    while (n_scans is None or k < n_scans) and t0 + k * scan_period + sweep <= t1:
        stamps.append(t0 + k * scan_period)
        k += 1
    return stamps


def simulate_sequence(scene, trajectory_tum, out_dir, pattern, scan_period=0.1, n_scans=None, ray_range=(1.0, 50.0), range_sigma=0.0,
                      seed=0, scan_fn=None):
    """Flies the sensor through the scene and writes the folder examples/run_sequence.py reads -> the list of scan stamps.

    trajectory_tum: TUM rows [K,8] (ts x y z qx qy qz qw) or a TUM file; pattern: (directions [3,n] fp32, point_times [n]) as
    utils/synthetic.lidar_pattern gives them, the times relative to a scan's stamp and >= 0.  Scan k has the stamp T_0 + k *
    scan_period; scans are made while the whole sweep lies inside the trajectory (at most n_scans).  Written to out_dir:
      NNNNNN.npy   float32 [N,4]: x y z = direction * distance in the sensor frame at each point's own time (not compensated), and t,
                   the point's time relative to the stamp
      stamps.txt   one stamp per line
      gt_tum.txt   the trajectory's pose at every stamp (ts x y z qx qy qz qw)
    Scan k is drawn with seed + k.  scan_fn: simulate_scan, or a stand-in with its signature (another sensor model)."""
    directions, point_times = pattern
    _check_pattern(directions, point_times, "simulate_sequence")
    _check_range(ray_range, range_sigma, seed, "simulate_sequence")
    period = float(scan_period)
    if not (math.isfinite(period) and period > 0):
        raise ValueError(f"simulate_sequence: scan_period must be finite and > 0, got {scan_period!r}")
    if n_scans is not None and (int(n_scans) != n_scans or n_scans < 1):
        raise ValueError(f"simulate_sequence: n_scans must be a positive integer or None, got {n_scans!r}")
    if point_times.numel() == 0 or float(point_times.min()) < 0:
        raise ValueError("simulate_sequence: the pattern needs at least one ray and point times >= 0")
    times, positions, rotations, rotvecs = trajectory_arrays(trajectory_tum)
    sweep = float(point_times.max())
    stamps = sequence_stamps(float(times[0]), float(times[-1]), period, sweep, n_scans)
    if not stamps:
        raise ValueError(f"simulate_sequence: the trajectory spans {float(times[-1] - times[0])} s, shorter than one sweep of {sweep} s")
    trajectory = ops.Trajectory(times, positions, rotations, rotvecs, scene.device)
    scan_fn = simulate_scan if scan_fn is None else scan_fn
    os.makedirs(out_dir, exist_ok=True)
    slerp = Slerp(times, rotations)
    gt_rows = []
    for k, stamp in enumerate(stamps):
        scan, keep = scan_fn(scene, trajectory, directions, point_times, stamp, ray_range, range_sigma, seed + k)
        xyz = (scan.ray_directions * scan.distances).T
        local = point_times.to(keep.device)[keep].to(torch.float32)
        rows = torch.cat([xyz.to(torch.float32), local[:, None]], dim=1).cpu().numpy()
        np.save(os.path.join(out_dir, f"{k:06d}.npy"), np.ascontiguousarray(rows, dtype=np.float32))
        quat = _matrix_to_quat(slerp(stamp)[None])[0]
        gt_rows.append(np.concatenate([[stamp], _interp_linear(times, positions, stamp), quat]))
    with open(os.path.join(out_dir, "stamps.txt"), "w") as f:
        f.writelines(f"{s!r}\n" for s in stamps)
    np.savetxt(os.path.join(out_dir, "gt_tum.txt"), np.asarray(gt_rows), fmt="%.17g")
    return stamps
