"""Ground-truth LiDAR maps from measured scans and a ground-truth trajectory, and their masking (the reference's
examples/fusion_portable/create_lidar_map.py and mask_gt_with_trajectory.py), on HIP and without open3d, scipy or a process pool.

build_lidar_map moves every point of every scan by the trajectory's pose at the point's own timestamp (ops.trajectory_transform:
include/loner_hip.h, lnr_cloud_trajectory_transform), voxel-down-samples each scan and the merged cloud, and optionally removes
statistical outliers (PointCloud.remove_statistical_outlier).  mask_by_distance keeps the points of one cloud that lie near another.
Differences from the reference, by intent:
  * the poses are interpolated on the device in fp64 with every rounding stated; scipy's Slerp and interp1d give the same poses up to
    rounding (at an exact pose time scipy takes the end of the segment before it, this takes the start of the one after it);
  * the scans are (xyz, absolute timestamps) arrays: reading the bag and the script's guesses about its time field (:85-100) stay with
    the caller;
  * a scan is skipped when any of its points beyond min_range lies outside the trajectory's time span; the script tests the message's
    time against both ends and the latest point time against the last pose only (:65, :102);
  * a scan with a non-finite point or time raises ValueError (the script would carry NaN into open3d);
  * voxel_down_sample returns its voxels in ascending order and the outlier filter's sums have a fixed order (include/loner_hip.h).
"""
import os

import numpy as np
import torch

from .. import ops
from ..common.pose_utils import quat_to_matrix, read_tum
from .lidar_map import PointCloud, _device


def segment_rotvecs(quats):
    """[K-1,3]: the rotation vectors log(R_k^T R_k+1) of consecutive unit quaternions (rows x y z w), angle in [0, pi], in numpy fp64
    (scipy: (rotations[:-1].inv() * rotations[1:]).as_rotvec())."""
    q = np.asarray(quats, dtype=np.float64).reshape(-1, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    a, b = q[:-1], q[1:]
    av, aw, bv, bw = -a[:, :3], a[:, 3:], b[:, :3], b[:, 3:]                # conj(a) * b
    v = aw * bv + bw * av + np.cross(av, bv)
    w = (aw * bw)[:, 0] - (av * bv).sum(1)
    flip = w < 0
    v[flip], w[flip] = -v[flip], -w[flip]
    norm = np.linalg.norm(v, axis=1)
    angle = 2.0 * np.arctan2(norm, w)
    small = norm < 1e-12
    scale = np.where(small, 2.0, angle / np.where(small, 1.0, norm))
    return v * scale[:, None]


def trajectory_arrays(trajectory):
    """(times [K], positions [K,3], rotations [K,3,3], rotvecs [K-1,3]) in numpy fp64 from TUM rows [K,8] (ts x y z qx qy qz qw) or the
    path of a TUM file.  ValueError for fewer than 2 poses, another shape, or pose times that do not strictly increase."""
    rows = read_tum(trajectory) if isinstance(trajectory, (str, os.PathLike)) else np.asarray(trajectory, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != 8:
        raise ValueError(f"trajectory: TUM rows [K,8] (ts x y z qx qy qz qw), got {rows.shape}")
    if rows.shape[0] < 2:
        raise ValueError(f"trajectory: at least 2 poses are needed, got {rows.shape[0]}")
    if not (np.diff(rows[:, 0]) > 0).all():
        raise ValueError("trajectory: the pose times must be strictly increasing")
    return rows[:, 0], rows[:, 1:4], quat_to_matrix(rows[:, 4:]), segment_rotvecs(rows[:, 4:])


def load_trajectory(trajectory, device=None):
    """An ops.Trajectory on the device from TUM rows or a TUM file (trajectory_arrays)."""
    arrays = trajectory_arrays(trajectory)
    return ops.Trajectory(*arrays, _device(device))


def build_lidar_map(scans, trajectory, voxel_size=0.05, run_outlier_filter=False, min_range=0.5, device=None):
    """create_lidar_map.py -> PointCloud.  scans: an iterable of (xyz [n,3], timestamps [n]) (arrays or tensors; sensor frame, absolute
    times); trajectory: TUM rows, a TUM file, or an ops.Trajectory.  Points within min_range of the sensor are dropped; a scan with a
    point outside the trajectory's time span is skipped whole (one host read per scan); every other scan is compensated,
    voxel-down-sampled and appended; the merged cloud is down-sampled again and, when asked, filtered with
    remove_statistical_outlier(20, 1.5)."""
    v = float(voxel_size)
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"build_lidar_map: voxel_size must be finite and > 0, got {voxel_size!r}")
    arrays = None if isinstance(trajectory, ops.Trajectory) else trajectory_arrays(trajectory)
    dev = _device(device)
    traj = trajectory if arrays is None else ops.Trajectory(*arrays, dev)
    parts = []
    for k, (xyz, stamps) in enumerate(scans):
        pts = xyz if torch.is_tensor(xyz) else torch.from_numpy(np.asarray(xyz, dtype=np.float64))
        ts = stamps if torch.is_tensor(stamps) else torch.from_numpy(np.asarray(stamps, dtype=np.float64))
        if pts.dim() != 2 or pts.shape[1] != 3 or ts.shape != (pts.shape[0],):
            raise ValueError(f"build_lidar_map: scan {k}: xyz [n,3] and timestamps [n], got {tuple(pts.shape)} and {tuple(ts.shape)}")
        out, info = ops.trajectory_transform(pts.to(dev), ts.to(dev), traj, min_range)
        info = info.cpu()
        if int(info[0]):
            raise ValueError(f"build_lidar_map: scan {k}: {int(info[4])} points with a non-finite coordinate or timestamp")
        if int(info[3]) or int(info[1]) == 0:
            continue
        parts.append(ops.voxel_down_sample(out[:int(info[1])], v))
    if not parts:
        return PointCloud(torch.zeros(0, 3, dtype=torch.float64, device=dev))
    print("Downsampling")
    cloud = PointCloud(torch.cat(parts)).voxel_down_sample(v)
    if run_outlier_filter:
        print("Running SOR filter")
        cloud, _ = cloud.remove_statistical_outlier(nb_neighbors=20, std_ratio=1.5)
    return cloud


def mask_by_distance(cloud, reference, threshold=0.1):
    """mask_gt_with_trajectory.py:94-97 -> a new PointCloud of the points of `cloud` whose exact distance to the nearest point of
    `reference` is < threshold, in order, with their normals and covariances.  The distances are compute_point_cloud_distance's, and
    they and the mask stay on the device.  Nothing is near an empty reference: it keeps no point."""
    if not isinstance(cloud, PointCloud) or not isinstance(reference, PointCloud):
        raise ValueError("mask_by_distance: cloud and reference must be PointClouds")
    t = float(threshold)
    if not (np.isfinite(t) and t > 0):
        raise ValueError(f"mask_by_distance: threshold must be finite and > 0, got {threshold!r}")
    dev = cloud.points.device
    if len(cloud) == 0 or len(reference) == 0:
        index = torch.zeros(0, dtype=torch.int64, device=dev)
    else:
        index = (ops.NNGrid(reference.points.to(dev)).distance(cloud.points) < t).nonzero().squeeze(1)
    out = PointCloud(cloud.points[index])
    out.normals = None if cloud.normals is None else cloud.normals[index].contiguous()
    out.covariances = None if cloud.covariances is None else cloud.covariances[index].contiguous()
    return out
