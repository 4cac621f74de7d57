"""WorldCube and 6-vector <-> 4x4 conversions.

Mirrors the part of the reference's src/common/pose_utils.py that the mapping hot path touches:
WorldCube (:24-57), tensor_to_transform (:288-302) and build_poses_from_df (:321-343).  The reference delegates the axis-angle ->
matrix map to pytorch3d 0.7.2 (absent here); pytorch3d's published algorithm (axis-angle -> unit
quaternion with the small-angle series, quaternion -> matrix) is written out in stock torch ops so
that the pose-Jacobian tail stays in torch autograd on whatever device the pose lives on.
"""
from dataclasses import dataclass

import numpy as np
import torch


@dataclass
class WorldCube:
    """Shift and scale that map the scene into the cube [-1,1]^3 (pose_utils.py:24-57)."""
    scale_factor: torch.Tensor
    shift: torch.Tensor

    def to(self, device, clone=False) -> "WorldCube":
        shift = self.shift if isinstance(self.shift, torch.Tensor) else torch.tensor(self.shift, dtype=torch.float32)
        scale = self.scale_factor if isinstance(self.scale_factor, torch.Tensor) else torch.tensor(float(self.scale_factor))
        if clone:
            return WorldCube(scale.to(device, copy=True), shift.to(device, copy=True))
        self.shift = shift.to(device)
        self.scale_factor = scale.to(device)
        return self

    def as_dict(self) -> dict:
        return {"scale_factor": float(self.scale_factor), "shift": [float(s) for s in self.shift.cpu()]}


def axis_angle_to_matrix(aa: torch.Tensor) -> torch.Tensor:
    """[...,3] -> [...,3,3]"""
    theta = torch.linalg.vector_norm(aa, dim=-1, keepdim=True)
    half = 0.5 * theta
    small = theta.abs() < 1e-6
    denom = torch.where(small, torch.ones_like(theta), theta)
    k = torch.where(small, 0.5 - theta * theta / 48.0, torch.sin(half) / denom)
    q = torch.cat([torch.cos(half), aa * k], dim=-1)
    r, i, j, kk = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    m = torch.stack([
        1 - two_s * (j * j + kk * kk), two_s * (i * j - kk * r), two_s * (i * kk + j * r),
        two_s * (i * j + kk * r), 1 - two_s * (i * i + kk * kk), two_s * (j * kk - i * r),
        two_s * (i * kk - j * r), two_s * (j * kk + i * r), 1 - two_s * (i * i + j * j)], dim=-1)
    return m.reshape(aa.shape[:-1] + (3, 3))


def matrix_to_axis_angle(R: torch.Tensor) -> torch.Tensor:
    """[3,3] -> [3] via the unit quaternion (largest-component branch), in float64.
    Used only when a Pose is created from a matrix; not on the hot path."""
    m = R.detach().double().cpu()
    t = m.trace()
    cand = torch.stack([1 + t, 1 + 2 * m[0, 0] - t, 1 + 2 * m[1, 1] - t, 1 + 2 * m[2, 2] - t])
    i = int(torch.argmax(cand))
    if i == 0:
        q = torch.stack([cand[0], m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]])
    elif i == 1:
        q = torch.stack([m[2, 1] - m[1, 2], cand[1], m[0, 1] + m[1, 0], m[0, 2] + m[2, 0]])
    elif i == 2:
        q = torch.stack([m[0, 2] - m[2, 0], m[0, 1] + m[1, 0], cand[2], m[1, 2] + m[2, 1]])
    else:
        q = torch.stack([m[1, 0] - m[0, 1], m[0, 2] + m[2, 0], m[1, 2] + m[2, 1], cand[3]])
    q = q / q.norm()
    if q[0] < 0:
        q = -q
    v = q[1:]
    n = v.norm()
    if n < 1e-12:
        return (2 * v).to(R.dtype).to(R.device)
    angle = 2 * torch.atan2(n, q[0])
    return (v / n * angle).to(R.dtype).to(R.device)


def tensor_to_transform(t: torch.Tensor) -> torch.Tensor:
    """[6] or [N,6] = [translation, axis-angle] -> [4,4] or [N,4,4] (pose_utils.py:288-302)."""
    single = t.dim() == 1
    if single:
        t = t[None]
    R = axis_angle_to_matrix(t[:, 3:])
    top = torch.cat([R, t[:, :3, None]], dim=2)
    bottom = torch.zeros(t.shape[0], 1, 4, dtype=t.dtype, device=t.device)
    bottom[:, 0, 3] = 1
    T = torch.cat([top, bottom], dim=1)
    return T[0] if single else T


def transform_to_tensor(T: torch.Tensor, device=None) -> torch.Tensor:
    """[4,4] -> [6] (pose_utils.py:255-282)."""
    out = torch.cat([T[:3, 3].detach(), matrix_to_axis_angle(T[:3, :3]).to(T.device)]).float()
    return out.to(device) if device is not None else out


def quat_to_matrix(quat) -> np.ndarray:
    """scipy's Rotation.from_quat(q).as_matrix() for rows q = (x, y, z, w), in numpy fp64: each quaternion normalised first."""
    q = np.asarray(quat, dtype=np.float64).reshape(-1, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = x2 - y2 - z2 + w2
    R[:, 1, 0] = 2 * (xy + zw)
    R[:, 2, 0] = 2 * (xz - yw)
    R[:, 0, 1] = 2 * (xy - zw)
    R[:, 1, 1] = -x2 + y2 - z2 + w2
    R[:, 2, 1] = 2 * (yz + xw)
    R[:, 0, 2] = 2 * (xz + yw)
    R[:, 1, 2] = 2 * (yz - xw)
    R[:, 2, 2] = -x2 - y2 + z2 + w2
    return R


def read_tum(path) -> np.ndarray:
    """The rows of a TUM trajectory file (ts x y z qx qy qz qw, space separated), fp64 [n, 8]; the reference reads it with
    pd.read_csv(path, delimiter=' ', header=None)."""
    return np.loadtxt(path, dtype=np.float64, ndmin=2, delimiter=" ")


def build_poses_from_df(df, zero_origin=False):
    """The reference's build_poses_from_df (pose_utils.py:321-343) without pandas or scipy: df is a [n, 8] array of TUM rows (or
    anything with .to_numpy()).  -> (poses fp32 [n,4,4], timestamps fp64 [n]); the poses are built in fp64 and rounded to fp32 at the
    end, as the reference's .float() does."""
    data = torch.from_numpy(np.asarray(df.to_numpy(dtype=np.float64) if hasattr(df, "to_numpy") else df, dtype=np.float64))
    ts = data[:, 0]
    xyz = data[:, 1:4]
    rots = torch.from_numpy(quat_to_matrix(data[:, 4:].numpy()))
    poses = torch.cat((rots, xyz.unsqueeze(2)), dim=2)
    homog = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).tile((poses.shape[0], 1, 1))
    poses = torch.cat((poses, homog), dim=1)
    if zero_origin:
        rot_inv = poses[0, :3, :3].T
        t_inv = -rot_inv @ poses[0, :3, 3]
        start_inv = torch.hstack((rot_inv, t_inv.reshape(-1, 1)))
        start_inv = torch.vstack((start_inv, torch.tensor([0, 0, 0, 1.0], dtype=torch.float64)))
        poses = start_inv.unsqueeze(0) @ poses
    return poses.float(), ts


def matrix_to_quaternion(R: torch.Tensor) -> torch.Tensor:
    """[n,3,3] -> [n,4] unit quaternions (w, x, y, z) with w >= 0, each from the largest of its four candidate components (the
    well-conditioned branch), in the matrices' type"""
    m = R.reshape(-1, 3, 3)
    t = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    cand = torch.stack([1 + t, 1 + 2 * m[:, 0, 0] - t, 1 + 2 * m[:, 1, 1] - t, 1 + 2 * m[:, 2, 2] - t], dim=1)
    rows = torch.stack([
        torch.stack([cand[:, 0], m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]], dim=1),
        torch.stack([m[:, 2, 1] - m[:, 1, 2], cand[:, 1], m[:, 0, 1] + m[:, 1, 0], m[:, 0, 2] + m[:, 2, 0]], dim=1),
        torch.stack([m[:, 0, 2] - m[:, 2, 0], m[:, 0, 1] + m[:, 1, 0], cand[:, 2], m[:, 1, 2] + m[:, 2, 1]], dim=1),
        torch.stack([m[:, 1, 0] - m[:, 0, 1], m[:, 0, 2] + m[:, 2, 0], m[:, 1, 2] + m[:, 2, 1], cand[:, 3]], dim=1)], dim=1)
    q = rows[torch.arange(m.shape[0]), torch.argmax(cand, dim=1)]
    q = q / torch.linalg.vector_norm(q, dim=1, keepdim=True)
    return torch.where(q[:, :1] < 0, -q, q)


def dump_trajectory_to_tum(transformation_matrices: torch.Tensor, timestamps: torch.Tensor, output_file: str) -> None:
    """[n,4,4] poses and [n] stamps -> a TUM file: one row `ts x y z qx qy qz qw` per pose, %.10f, space separated
    (pose_utils.py:308-318)."""
    T = transformation_matrices.detach().cpu().reshape(-1, 4, 4)
    quat = matrix_to_quaternion(T[:, :3, :3])
    rows = torch.hstack([timestamps.detach().cpu().reshape(-1, 1).to(T.dtype), T[:, :3, 3], quat[:, 1:4], quat[:, 0:1]])
    np.savetxt(output_file, rows.numpy(), delimiter=" ", fmt="%.10f")


def compute_world_cube(camera_to_lidar, intrinsic_mats, image_sizes, lidar_poses, ray_range, padding=0.1, traj_bounding_box=None) -> WorldCube:
    """The cube every ray of the run fits in (pose_utils.py:159-260), lidar only: the axis-aligned box around the sensor positions and,
    for every pose, the eight corners (+-d, +-d, +-d) of the sensor's reach d = ray_range[1] in the sensor's frame.  shift is minus
    the box's centre; scale_factor is the box's diagonal / (2 sqrt 3) (the half edge of the cube with that diagonal), widened by
    `padding`.  lidar_poses [n,4,4] are taken relative to the first (poses @ inv(poses[0]), as the reference writes it); without
    poses, traj_bounding_box {'x': [lo, hi], 'y': ..., 'z': ...} gives eight identity-rotation poses at its corners.  A
    camera_to_lidar raises: the colour path is not implemented here."""
    if not 0 <= padding < 1:
        raise ValueError(f"compute_world_cube: padding must lie in [0, 1), got {padding}")
    if camera_to_lidar is not None:
        raise NotImplementedError("compute_world_cube: the camera branch (view frustums) is not implemented; pass camera_to_lidar=None")
    if lidar_poses is None and traj_bounding_box is None:
        raise ValueError("compute_world_cube: lidar_poses or traj_bounding_box is needed")
    if lidar_poses is None:
        print("Computing world cube using supplied trajectory bounding box")
        axes = [torch.tensor([float(v) for v in traj_bounding_box[a]]) for a in ("x", "y", "z")]
        corners = torch.stack(torch.meshgrid(axes, indexing="ij"), dim=-1).reshape(-1, 3)
        poses = torch.eye(4).tile((8, 1, 1))
        poses[:, :3, 3] = corners
    else:
        print("Computing world cube with groundtruth poses")
        poses = torch.as_tensor(lidar_poses).float()
        poses = poses @ torch.linalg.inv(poses[0])
    reach = float(ray_range[1])
    signs = torch.tensor([[sx, sy, sz, 1.0] for sz in (-1, 1) for sx in (-1, 1) for sy in (-1, 1)])
    signs[:, :3] *= reach
    corners = (poses[:, :3, :] @ signs.T).transpose(1, 2).reshape(-1, 3)
    points = torch.cat([corners, poses[:, :3, 3]])
    lo, hi = points.min(dim=0)[0], points.max(dim=0)[0]
    origin = lo + (hi - lo) / 2
    scale_factor = (torch.linalg.norm(hi - lo) / (2 * torch.sqrt(torch.Tensor([3])))) * (1 + padding)
    return WorldCube(scale_factor, -origin)
