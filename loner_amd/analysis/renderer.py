"""Depth images and fly-throughs of a trained map from camera poses (the reference's analysis/renderer.py and the save_depth of
analysis/render_utils.py), on HIP and without matplotlib, imageio, scipy or pandas.

DepthRenderer builds the rays of a whole image in one launch (CameraRayDirections -> lnr_build_camera_rays), renders them through
Model.render_depth_peak - the compositing kernel also finds each ray's sample of maximal weight, so the [N,S] weights and depths the
reference reads back for its peak-depth consistency image (renderer.py:195-198) are never written - and colours the depth with the
turbo map on the device (lnr_depth_colormap).  Differences from the reference, by intent:
  * no colour image: the colour branch is never trained on the LiDAR path, so rgb_fine has no content (Model.forward(camera=True)
    raises);
  * the image is rendered as one batch instead of chunks of 1024 rays (the result does not depend on the chunking, only the order
    in which torch's generator is asked for seeds does);
  * no video encoder: render_flythrough writes numbered PNG frames and returns the spin indices, the reference's mp4 / gif files
    are not produced;
  * a camera origin outside the world cube raises, as LidarMapRenderer.scan_rays does;
  * the trajectory is read with numpy and interpolated with the slerp / linear interpolation below.
"""
import os
import struct
import zlib

import numpy as np
import torch

from .. import ops
from ..common.pose import Pose
from ..common.pose_utils import quat_to_matrix, read_tum
from ..common.ray_utils import CameraRayDirections, mapping_device
from ..common.settings import Settings
from .turbo import turbo_u8


def lidar_only_calibration():
    """The camera the reference falls back to when the configuration has none (renderer.py:112-120): 512 x 384 pixels,
    K = [[302, 0, 260], [0, 302, 197], [0, 0, 1]] (also new_k), no distortion, and the lidar-to-camera orientation
    [0.5, -0.5, 0.5, -0.5] (w, x, y, z: x right, y down, z forward for a lidar with x forward and z up)."""
    k = torch.tensor([[302.0, 0.0, 260.0], [0.0, 302.0, 197.0], [0.0, 0.0, 1.0]])
    return Settings({"camera_intrinsic": {"width": 512, "height": 384, "k": k, "new_k": k, "distortion": torch.zeros(4)},
                     "lidar_to_camera": {"xyz": [0.0, 0.0, 0.0], "orientation": [0.5, -0.5, 0.5, -0.5]}})


# ---------------------------------------------------------------- PNG
def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, image):
    """An 8-bit PNG from a uint8 array [H,W,4] (RGBA), [H,W,3] (RGB) or [H,W] (grey), with zlib and struct only: filter type 0 on
    every row, one IDAT chunk."""
    img = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (3, 4)) or img.size == 0:
        raise ValueError(f"write_png: uint8 [H,W], [H,W,3] or [H,W,4], got {img.dtype} {img.shape}")
    h, w = img.shape[:2]
    colour_type = 0 if img.ndim == 2 else (2 if img.shape[2] == 3 else 6)
    rows = np.ascontiguousarray(img).reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), rows], axis=1).tobytes()
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour_type, 0, 0, 0)))
        f.write(_png_chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(_png_chunk(b"IEND", b""))


# ---------------------------------------------------------------- colour
_tables = {}


def _turbo_table(device):
    t = _tables.get(str(device))
    if t is None:
        t = _tables[str(device)] = torch.from_numpy(turbo_u8()).to(device)
    return t


def depth_to_rgba(depth, min_depth=1, max_depth=50, multiplier=1.0):
    """uint8 [H,W,4] on the device: the colours save_depth writes for a depth image [1,1,H,W] (or [H,W]) - turbo over
    [min_depth, max_depth], pixels at or beyond max_depth black (render_utils.py:116-127).  multiplier: applied first (the world
    cube's scale for depths in cube units)."""
    img = depth.detach().squeeze()
    return ops.depth_colormap(img, _turbo_table(img.device), multiplier, min_depth, max_depth)


def save_depth(depth_fine, fname, render_dir, min_depth=1, max_depth=50):
    """The reference's save_depth: depth [1,1,H,W] in metres -> {render_dir}/{fname} as an RGBA PNG.  Returns the path."""
    path = os.path.join(str(render_dir), fname)
    write_png(path, depth_to_rgba(depth_fine, min_depth, max_depth))
    return path


# ---------------------------------------------------------------- fly-through poses
def _matrix_to_quat(R):
    """unit quaternions [n,4] (x, y, z, w) of rotation matrices [n,3,3], fp64: the branch with the largest denominator"""
    R = np.asarray(R, dtype=np.float64)
    q = np.empty((R.shape[0], 4))
    for n, m in enumerate(R):
        d = [m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2]]
        c = int(np.argmax(d))
        if c == 3:
            q[n] = [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1.0 + d[3]]
        else:
            i, j, k = c, (c + 1) % 3, (c + 2) % 3
            q[n, i] = 1.0 - d[3] + 2.0 * m[i, i]
            q[n, j] = m[j, i] + m[i, j]
            q[n, k] = m[k, i] + m[i, k]
            q[n, 3] = m[k, j] - m[j, k]
        q[n] /= np.linalg.norm(q[n])
    return q


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _quat_to_rotvec(q):
    q = q if q[3] >= 0 else -q                       # the rotation by at most pi
    s = float(np.linalg.norm(q[:3]))
    angle = 2.0 * np.arctan2(s, q[3])
    if angle <= 1e-3:
        scale = 2.0 + angle * angle / 12.0 + 7.0 * angle ** 4 / 2880.0
    else:
        scale = angle / np.sin(angle / 2.0)
    return scale * q[:3]


def _rotvec_to_matrix(v):
    angle = float(np.linalg.norm(v))
    if angle <= 1e-3:
        scale = 0.5 - angle * angle / 48.0 + angle ** 4 / 3840.0
    else:
        scale = np.sin(angle / 2.0) / angle
    q = np.concatenate([scale * v, [np.cos(angle / 2.0)]])
    return quat_to_matrix(q[None])[0]


class Slerp:
    """Spherical linear interpolation between timed rotations: within [t_i, t_i+1] the rotation is R_i exp(a log(R_i^T R_i+1)) with
    a = (t - t_i) / (t_i+1 - t_i) and the logarithm of the rotation by at most pi (the definition scipy's Slerp implements)."""

    def __init__(self, times, matrices):
        self.times = np.asarray(times, dtype=np.float64)
        if self.times.ndim != 1 or self.times.size < 2 or not np.all(np.diff(self.times) > 0):
            raise ValueError("Slerp: times must be strictly increasing, at least two of them")
        self.quats = _matrix_to_quat(matrices)
        self.matrices = quat_to_matrix(self.quats)
        conj = self.quats * np.array([-1.0, -1.0, -1.0, 1.0])
        self.rotvecs = np.stack([_quat_to_rotvec(_quat_mul(conj[i], self.quats[i + 1])) for i in range(len(self.times) - 1)])

    def __call__(self, t):
        t = float(t)
        if t < self.times[0] or t > self.times[-1]:
            raise ValueError(f"Slerp: time {t} outside [{self.times[0]}, {self.times[-1]}]")
        i = max(int(np.searchsorted(self.times, t)) - 1, 0)
        a = (t - self.times[i]) / (self.times[i + 1] - self.times[i])
        return self.matrices[i] @ _rotvec_to_matrix(a * self.rotvecs[i])


def _interp_linear(times, values, t):
    """scipy's interp1d(times, values, axis=0) at one time: slope * (t - t_lo) + v_lo on the interval found by searchsorted"""
    hi = min(max(int(np.searchsorted(times, t)), 1), len(times) - 1)
    lo = hi - 1
    slope = (values[hi] - values[lo]) / (times[hi] - times[lo])
    return slope * (t - times[lo]) + values[lo]


def flythrough_poses(trajectory_tum, velocity=1.0, fps=5, spin_spacing_m=10.0, spin_duration_s=15.0, render_global=False,
                     interpolate=True):
    """The lidar poses of the reference's fly-through (renderer.py:345-420): -> (poses fp32 [n,4,4], spin_idxs).  Computed in numpy
    fp64 (flythrough_poses_f64) and rounded to fp32 at the end, as the reference does."""
    poses, spin_idxs = flythrough_poses_f64(trajectory_tum, velocity, fps, spin_spacing_m, spin_duration_s, render_global, interpolate)
    return torch.from_numpy(poses.astype(np.float32)), spin_idxs


def flythrough_poses_f64(trajectory_tum, velocity=1.0, fps=5, spin_spacing_m=10.0, spin_duration_s=15.0, render_global=False,
                         interpolate=True):
    """-> (poses numpy fp64 [n,4,4], spin_idxs).
    trajectory_tum: a TUM file (ts x y z qx qy qz qw) or its rows [m,8].  Unless render_global, poses are relative to the first.
    The camera moves along the trajectory at `velocity` m/s and `fps` images per second (rotations by slerp, positions linear in
    time); whenever more than spin_spacing_m metres have been covered since the last spin it turns once about the lidar's z axis in
    spin_duration_s * fps steps.  The reference's loop is kept as it is: the distance is measured from the previous iteration's last
    pose, and every spin pose's index enters spin_idxs twice.  interpolate=False: the trajectory's own poses and no spins."""
    rows = read_tum(trajectory_tum) if isinstance(trajectory_tum, (str, os.PathLike)) else np.asarray(trajectory_tum, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != 8 or rows.shape[0] < 1:
        raise ValueError(f"flythrough_poses: TUM rows [n,8], got {rows.shape}")
    n = rows.shape[0]
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3] = quat_to_matrix(rows[:, 4:])
    T[:, :3, 3] = rows[:, 1:4]
    if not render_global:
        T = np.linalg.inv(T[0].copy()) @ T
    if not interpolate:
        return T, []
    gt_xyz = T[:, :3, 3]
    dists = np.sqrt(np.sum(np.diff(gt_xyz, axis=0) ** 2, axis=1))
    timestamps = np.insert(np.cumsum(dists / velocity), 0, 0.)
    slerp = Slerp(timestamps, T[:, :3, :3])
    num_images = int(timestamps[-1] * fps)
    image_timestamps = np.linspace(0, timestamps[-1], num_images)
    lidar_poses = []
    dist_since_last_spin = 0
    prev_pose = np.eye(4)
    spin_idxs = []
    for timestamp in image_timestamps:
        xyz = _interp_linear(timestamps, gt_xyz, timestamp)
        rot = slerp(timestamp)
        P = np.vstack((np.hstack((rot, xyz.reshape(-1, 1))), [0, 0, 0, 1]))
        lidar_poses.append(P)
        dist_since_last_spin += np.sqrt(np.sum((xyz - prev_pose[:3, 3]) ** 2))
        if dist_since_last_spin > spin_spacing_m:
            num_spin_steps = int(spin_duration_s * fps)
            for a in np.linspace(0, 2 * np.pi, num_spin_steps):
                c, s = np.cos(a), np.sin(a)
                rel = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
                spin_idxs.append(len(lidar_poses))
                P = np.vstack((np.hstack((rot @ rel, xyz.reshape(-1, 1))), [0, 0, 0, 1]))
                spin_idxs.append(len(lidar_poses))
                lidar_poses.append(P)
            dist_since_last_spin = 0
        prev_pose = P
    if not lidar_poses:
        return np.zeros((0, 4, 4)), spin_idxs
    return np.stack(lidar_poses), spin_idxs


# ---------------------------------------------------------------- rendering
def timestamp_name(timestamp):
    """the reference's file-name rule (renderer.py:273): the first five characters of the time with '.' replaced by '_'"""
    value = timestamp.item() if hasattr(timestamp, "item") else timestamp
    return str(value).replace('.', '_')[:5]


class DepthRenderer:
    """The reference's renderer.py as a class in LidarMapRenderer's pattern: render_frame (one camera pose), render_stills (the
    checkpoint's keyframe poses) and render_flythrough (a trajectory).  calibration: the run's calibration settings
    (camera_intrinsic, lidar_to_camera), or None for lidar_only_calibration()."""

    def __init__(self, model, ckpt, world_cube, ray_range, calibration=None):
        self.model = model
        self.ckpt = ckpt
        self.world_cube = world_cube
        self.ray_range = ray_range
        self.calibration = lidar_only_calibration() if calibration is None else calibration
        self.ray_directions = CameraRayDirections(self.calibration, device=mapping_device())
        # (a configuration without a lidar_to_camera entry: the identity, as Pose.from_settings(None) gives)
        self.lidar_to_camera = Pose.from_settings(self.calibration["lidar_to_camera"] if "lidar_to_camera" in self.calibration else None)
        self.im_size = (self.ray_directions.im_height, self.ray_directions.im_width)

    def camera_pose(self, lidar_pose):
        """lidar pose (a Pose or a 4x4 matrix) -> camera Pose = lidar pose * lidar_to_camera, composed on the host as the reference
        does (renderer.py:278)"""
        lidar_pose = lidar_pose if isinstance(lidar_pose, Pose) else Pose(torch.as_tensor(lidar_pose))
        return Pose(lidar_pose.get_transformation_matrix().detach().cpu()) * self.lidar_to_camera

    def render_frame(self, camera_pose, ray_sampler, consistency=True, front_to_back=None):
        """-> (depth [1,1,H,W] in metres, peak_depth_consistency [1,1,H,W] in metres or None): render_dataset_frame
        (renderer.py:172-206) without the rgb.  The consistency image is |z of the sample of maximal weight - depth| per pixel.
        consistency=False renders the depth alone through Model.render_depth (front_to_back: its opt-in route; the peak is not
        available on it)."""
        H, W = self.im_size
        rays, _ = self.ray_directions.build_rays(None, camera_pose, None, self.world_cube, self.ray_range)
        if rays.shape[0] and bool((rays[0, :3].abs() > 1).any()):
            raise AssertionError("ray origins are outside the world cube")
        scale = torch.as_tensor(self.world_cube.scale_factor).detach().to(device=rays.device, dtype=torch.float32)
        if consistency:
            depth, peak = self.model.render_depth_peak(rays, ray_sampler, testing=True)
            peak_depth_consistency = (torch.abs(peak - depth)).reshape(1, 1, H, W) * scale
        else:
            depth = self.model.render_depth(rays, ray_sampler, testing=True, front_to_back=front_to_back)
            peak_depth_consistency = None
        return depth.reshape(1, 1, H, W) * scale, peak_depth_consistency

    def render_stills(self, ray_sampler, out_dir, skip_step=15, start_frame=0, use_gt_poses=False, only_last_frame=False, max_depth=75):
        """One predicted_depth_<timestamp>.png per selected keyframe pose of the checkpoint (renderer.py:229-243, :264-281): the
        poses from start_frame on, every skip_step-th (or the last one only), composed with lidar_to_camera.  Returns the paths."""
        poses = self.ckpt["poses"]
        selected = [poses[-1]] if only_last_frame else poses[start_frame:][::skip_step]
        key = "gt_lidar_pose" if use_gt_poses else "lidar_pose"
        os.makedirs(str(out_dir), exist_ok=True)
        dev = mapping_device()
        written = []
        for kf in selected:
            cam_pose = self.camera_pose(Pose(pose_tensor=kf[key].detach().cpu().clone()))
            depth, _ = self.render_frame(cam_pose.to(dev), ray_sampler, consistency=False)
            written.append(save_depth(depth, f"predicted_depth_{timestamp_name(kf['timestamp'])}.png", out_dir, max_depth=max_depth))
        return written

    def render_flythrough(self, trajectory, ray_sampler, out_dir, velocity=1.0, fps=5, spin_spacing_m=10.0, spin_duration_s=15.0,
                          render_global=False, interpolate=True, max_depth=50):
        """Renders flythrough_poses(trajectory, ...) through lidar_to_camera and writes flythrough_depth_<index, 5 digits>.png per
        pose, coloured as the stills are (save_depth: turbo over [1, max_depth]; the reference's save_video normalises by the 1st and
        99th percentile over all frames instead).  -> (paths, spin_idxs): the frames whose index is not in spin_idxs are the
        reference's "nospin" sequence.  There is no video encoder here, so video output is out of scope: the reference's mp4 and gif
        files (renderer.py:464-480) are not written - feed the frames to an encoder."""
        poses, spin_idxs = flythrough_poses(trajectory, velocity, fps, spin_spacing_m, spin_duration_s, render_global, interpolate)
        os.makedirs(str(out_dir), exist_ok=True)
        dev = mapping_device()
        written = []
        for idx, pose in enumerate(poses):
            depth, _ = self.render_frame(self.camera_pose(Pose(pose)).to(dev), ray_sampler, consistency=False)
            written.append(save_depth(depth, f"flythrough_depth_{idx:05d}.png", out_dir, max_depth=max_depth))
        return written, spin_idxs
