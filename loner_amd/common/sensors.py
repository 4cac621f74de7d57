"""LidarScan: the keyframe point buffer (SoA), mirroring src/common/sensors.py:57-232, and build_scan_from_points, which makes one
from a raw point array on the device (examples/run_loner.py:59-157)."""
from typing import Tuple, Union

import numpy as np
import torch


class LidarScan:
    """ray_directions [3,n] unit vectors (sensor frame), distances [n] metres, timestamps [n];
    optional sky_rays [3,m] (directions that hit nothing)."""

    def __init__(self, ray_directions: torch.Tensor = None, distances: torch.Tensor = None,
                 timestamps: torch.Tensor = None, sky_rays: torch.Tensor = None) -> None:
        self.ray_directions = torch.Tensor() if ray_directions is None else ray_directions
        self.distances = torch.Tensor() if distances is None else distances
        self.timestamps = torch.Tensor() if timestamps is None else timestamps
        self.sky_rays = sky_rays

    def __len__(self) -> int:
        return self.timestamps.shape[0]

    def get_start_time(self) -> torch.Tensor:
        return self.timestamps[0]

    def get_end_time(self) -> torch.Tensor:
        return self.timestamps[-1]

    def clear(self) -> "LidarScan":
        """Empties the scan.  A scan that carried sky rays keeps an (empty) sky tensor; one without stays without."""
        self.ray_directions, self.distances, self.timestamps = (torch.Tensor() for _ in range(3))
        self.sky_rays = None if self.sky_rays is None else torch.Tensor()
        return self

    def remove_points(self, num_points: int) -> "LidarScan":
        """Drops the num_points oldest points (the scan is time-ordered); sky rays are not points and stay."""
        tail = slice(num_points, None)
        self.ray_directions, self.distances, self.timestamps = self.ray_directions[..., tail], self.distances[tail], self.timestamps[tail]
        return self

    @staticmethod
    def _appended(held, more):
        """`more` behind `held` along the point axis; whatever is empty or absent is left out"""
        return more if held is None or held.numel() == 0 else torch.cat((held, more), dim=-1)

    def add_points(self, ray_directions: torch.Tensor, distances: torch.Tensor, timestamps: torch.Tensor,
                   sky_rays: torch.Tensor = None) -> "LidarScan":
        """Appends points (and sky rays, when given) behind the ones held."""
        self.ray_directions = self._appended(self.ray_directions, ray_directions)
        self.distances = self._appended(self.distances, distances)
        self.timestamps = self._appended(self.timestamps, timestamps)
        if sky_rays is not None:
            self.sky_rays = self._appended(self.sky_rays, sky_rays)
        return self

    def merge(self, other: "LidarScan") -> "LidarScan":
        return self.add_points(other.ray_directions, other.distances, other.timestamps, other.sky_rays)

    def motion_compensate(self, poses: Tuple["Pose", "Pose"], timestamps: Tuple[float, float], target_frame: "Pose",
                          use_gpu: bool = False) -> None:
        """Moves every point from the pose interpolated (or extrapolated) at its own timestamp between `poses`, whose times are
        `timestamps`, into target_frame (sensors.py:176-232), in place on the device the scan lives on (ops.motion_compensate;
        use_gpu is accepted and ignored).  The per-call constants - the relative axis-angle, the start rotation, both translations
        and the inverse target - are formed on the host in fp64 from the poses' fp32 matrices; those of them, and of the two pose
        times, that live on a device come over in one read."""
        from .. import ops
        from . import pose_utils as PU
        if len(self) == 0:
            raise ValueError("motion_compensate: the scan is empty")
        ops.require_device(self.ray_directions, self.distances, self.timestamps)
        dev = self.timestamps.device
        start_pose, end_pose = poses
        start_ts, end_ts = timestamps
        denom = end_ts - start_ts                                  # the caller's own subtraction, in the times' own type
        parts = [p.get_transformation_matrix().detach().double().reshape(16) for p in (start_pose, end_pose, target_frame)]
        parts += [t.detach().double().reshape(1) if torch.is_tensor(t) else torch.tensor([float(t)], dtype=torch.float64)
                  for t in (start_ts, denom)]
        # what is on the host already stays there; what lives on a device comes over in one read
        remote = [k for k, t in enumerate(parts) if t.device.type != "cpu"]
        if remote:
            fetched = torch.cat([parts[k].to(dev) for k in remote]).cpu()
            for k, piece in zip(remote, fetched.split([parts[k].numel() for k in remote])):
                parts[k] = piece
        host = torch.cat(parts)
        if not bool(torch.isfinite(host).all()):
            raise ValueError("motion_compensate: a pose or a pose time is not finite")
        T_start, T_end, T_target = (host[16 * k:16 * k + 16].reshape(4, 4) for k in range(3))
        relative_rotation = torch.linalg.inv(T_start[:3, :3]) @ T_end[:3, :3]
        axis_angle = PU.matrix_to_axis_angle(relative_rotation)
        T_inv = torch.linalg.inv(T_target)
        consts = torch.cat([axis_angle, T_start[:3, :3].reshape(9), T_start[:3, 3], T_end[:3, 3], T_inv[:3].reshape(12)])
        if not self.ray_directions.is_contiguous():
            self.ray_directions = self.ray_directions.contiguous()
        if not self.distances.is_contiguous():
            self.distances = self.distances.contiguous()
        ops.motion_compensate(self.ray_directions, self.distances, self.timestamps, float(host[48]), float(host[49]), consts.tolist())

    def clone(self) -> "LidarScan":
        return LidarScan(self.ray_directions.clone(), self.distances.clone(), self.timestamps.clone(),
                         self.sky_rays.clone() if self.sky_rays is not None else None)

    def to(self, device: Union[int, str]) -> "LidarScan":
        self.ray_directions = self.ray_directions.to(device)
        self.distances = self.distances.to(device)
        self.timestamps = self.timestamps.to(device)
        return self

    def get_sky_scan(self, distance: float) -> "LidarScan":
        sky = self.sky_rays
        return LidarScan(sky, torch.full_like(sky[0], float(distance)), torch.full_like(sky[0], float(self.timestamps[-1])))


# the reference's warn-once switches (run_loner.py:55-56): each message is printed for the first scan that takes its branch
_WARN_MOCOMP_ONCE = True
_WARN_LIDAR_TIMES_ONCE = True


def _on_device(a, device, dtype):
    """`a` (tensor or array) as a contiguous tensor of `dtype` on `device`: cast on the side it lives on, uploaded once"""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dtype).to(device).contiguous()


def build_scan_from_points(xyz, point_times, stamp: float, fov=None, min_range: float = 0.3, recompute_timestamps: bool = False,
                           device=None) -> Tuple[LidarScan, torch.Tensor]:
    """A raw point array -> (LidarScan on the device, order): run_loner.py's build_scan_from_msg without ROS, on the GPU
    (include/loner_hip.h, "scan ingestion", is the definition).

    xyz [N,3] fp32; point_times [N] of any real dtype (cast to fp32), or None; stamp the scan's time in seconds; fov None or an
    object with `enabled` and `range`, a list of at most 8 [lo, hi] degree segments.  Host inputs are uploaded once, device inputs
    are used in place (device: where to work; default the inputs' device, or the current GPU for host inputs).  order int64 [M] is the
    original index of every point of the scan, for carrying intensity or ring along.

    Unlike the reference the negative-start correction applies on every call, ties in time keep input order, and a scan with no
    point left or with a non-finite time on a kept point raises ValueError.  The scan is time-ordered: `scan.time_sorted` is True,
    read from the same status words as the count."""
    from .. import ops
    global _WARN_MOCOMP_ONCE, _WARN_LIDAR_TIMES_ONCE
    shape = tuple(xyz.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"build_scan_from_points: xyz [N,3], got {shape}")
    if point_times is not None and tuple(point_times.shape) != (shape[0],):
        raise ValueError(f"build_scan_from_points: point_times [{shape[0]}], got {tuple(point_times.shape)}")
    segments = None
    if fov is not None and fov.enabled:
        segments = [(float(s[0]), float(s[1])) for s in fov.range]
        if len(segments) > 8:
            raise ValueError(f"build_scan_from_points: {len(segments)} FOV segments, at most 8")
    if device is None:
        device = xyz.device if torch.is_tensor(xyz) and xyz.is_cuda else torch.device("cuda", torch.cuda.current_device())
    xyz_d = _on_device(xyz, device, torch.float32)
    times_d = None if point_times is None else _on_device(point_times, device, torch.float32)
    dirs, dist, times, order, info = ops.scan_from_points(xyz_d, times_d, stamp, segments, min_range, recompute_timestamps)
    m, flags, nonfinite, unsorted = info[:4]
    if m == 0:
        raise ValueError(f"build_scan_from_points: none of the {shape[0]} points passed the FOV and range tests")
    if nonfinite:
        raise ValueError(f"build_scan_from_points: {nonfinite} kept points have a non-finite time")
    from .. import hip
    if flags & hip.SCAN_NO_TIMES:
        if _WARN_MOCOMP_ONCE:
            print("Warning: LiDAR Data has No Associated Timestamps. Motion compensation is useless.")
            _WARN_MOCOMP_ONCE = False
    else:
        if _WARN_LIDAR_TIMES_ONCE:
            if flags & hip.SCAN_NANOSECONDS:
                print("Timestamps look to be in nanoseconds. Scaling")
            if flags & hip.SCAN_NEGATIVE_START:
                print("Timestamps negative (velodyne?). Correcting")
            print("Assuming LiDAR timestamps within a scan are local, and start at 0" if flags & hip.SCAN_LOCAL
                  else "Assuming lidar timestamps within a scan are global.")
            _WARN_LIDAR_TIMES_ONCE = False
        if flags & hip.SCAN_CONSTANT and _WARN_MOCOMP_ONCE:
            print("Warning: Timestamps in LiDAR data aren't unique. Motion compensation is useless")
            _WARN_MOCOMP_ONCE = False
    scan = LidarScan(dirs, dist, times)
    scan.time_sorted = unsorted == 0
    scan.ingest_flags = flags
    return scan, order
