"""Ray construction: LiDAR rays (src/common/ray_utils.py:31-60 and :252-322 of the reference) and camera rays (:62-225).

`LidarRayDirections.build_lidar_rays` keeps the reference's signature and return value but runs on
the MI355X: the scan (the keyframe point buffer) is kept resident in HBM, rays are built by
`lnr_build_lidar_rays`, and the gradient with respect to the 4x4 lidar pose is produced by
`lnr_lidar_rays_backward`, so that the 6-vector pose tail stays in stock torch autograd
(tensor_to_transform) exactly as in the reference.

`CameraRayDirections` precomputes the pinhole directions of an image once per camera on the host and builds ray records with
`lnr_build_camera_rays`; it is the depth renderer's front end (analysis/renderer.py) and carries no gradient.
"""
import weakref

import numpy as np
import torch

from .. import ops
from .pose_utils import WorldCube
from .sensors import LidarScan


def mapping_device():
    """The HIP device the mapper runs on (the reference hard-codes device 0, mapper.py:62-66)."""
    if not torch.cuda.is_available():
        raise RuntimeError("loner_amd: no MI355X/HIP device visible - the mapping hot path has no CPU implementation")
    return torch.device("cuda", torch.cuda.current_device())


_scan_cache = weakref.WeakKeyDictionary()      # scan object -> (key, directions, distances) on the device


def device_scan(scan: LidarScan, device):
    """HBM-resident copy of a scan's SoA buffers (uploaded once per keyframe).  The cache lives HERE, keyed weakly by the scan
    object - nothing is written onto the caller's LidarScan (in an integration that is the reference's own class)."""
    key = (scan.ray_directions.data_ptr(), scan.distances.data_ptr(), str(device))
    try:
        cache = _scan_cache.get(scan)
    except TypeError:                  # an object that cannot be weakly referenced: no caching
        cache = None
    if cache is None or cache[0] != key:
        dirs = scan.ray_directions.detach().to(device=device, dtype=torch.float32).contiguous()
        dist = scan.distances.detach().to(device=device, dtype=torch.float32).contiguous()
        cache = (key, dirs, dist)
        try:
            _scan_cache[scan] = cache
        except TypeError:
            pass
    return cache[1], cache[2]


def get_far_val(pts_o: torch.Tensor, pts_d: torch.Tensor, no_nan: bool = False):
    """Distance to the exit of the cube [-1,1]^3 (ray_utils.py:31-60); small helper kept in torch ops."""
    if no_nan:
        pts_d = pts_d + 1e-15
    t_lo = ((-1.0 - pts_o) / pts_d).clamp(min=0)
    t_hi = ((1.0 - pts_o) / pts_d).clamp(min=0)
    return torch.maximum(t_lo, t_hi).min(dim=1, keepdim=True).values


class _BuildLidarRays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lidar_pose, dirs_dev, dist_dev, index_dev, ray_range, scale, shift):
        T12 = lidar_pose.detach()[:3, :4].to(device=dirs_dev.device, dtype=torch.float32).contiguous().reshape(12)
        rays, depths, keep = ops.build_lidar_rays(dirs_dev, dist_dev, index_dev, T12, ray_range, scale, shift)
        ctx.save_for_backward(rays, index_dev, dirs_dev, T12)
        ctx.scale = float(scale)
        ctx.pose_device = lidar_pose.device
        ctx.mark_non_differentiable(depths, keep)
        return rays, depths, keep

    @staticmethod
    def backward(ctx, d_rays, _d_depths, _d_keep):
        rays, index_dev, dirs_dev, T12 = ctx.saved_tensors
        n = rays.shape[0]
        seg = torch.tensor([0, n], device=rays.device, dtype=torch.int32)
        dT = ops.lidar_rays_backward(d_rays.contiguous(), rays, index_dev, seg, [dirs_dev], T12.reshape(1, 12), ctx.scale)
        grad = torch.zeros(4, 4, device=rays.device, dtype=torch.float32)
        grad[:3, :4] = dT.reshape(3, 4)
        return grad.to(ctx.pose_device), None, None, None, None, None, None


class LidarRayDirections:
    def __init__(self, lidar_scan: LidarScan, chunk_size=512):
        self.lidar_scan = lidar_scan
        self._chunk_size = chunk_size
        self.num_chunks = -(-self.lidar_scan.ray_directions.shape[1] // self._chunk_size)

    def __len__(self):
        return self.lidar_scan.ray_directions.shape[1]

    def fetch_chunk_rays(self, chunk_idx: int, pose, world_cube: WorldCube, ray_range, device=None):
        start = chunk_idx * self._chunk_size
        end = min(len(self), (chunk_idx + 1) * self._chunk_size)
        return self.build_lidar_rays(torch.arange(start, end), ray_range, world_cube, pose.get_transformation_matrix())[0]

    def build_lidar_rays(self, lidar_indices: torch.Tensor, ray_range: torch.Tensor, world_cube: WorldCube,
                         lidar_pose: torch.Tensor, ignore_world_cube: bool = False):
        """-> (rays [k,13], depths [k]) on the HIP device; rays carry the gradient w.r.t. lidar_pose."""
        dev = mapping_device()
        dirs_dev, dist_dev = device_scan(self.lidar_scan, dev)
        index_dev = lidar_indices.to(device=dev, dtype=torch.int64)
        shift = world_cube.shift.detach().cpu().reshape(-1).tolist()
        rr = [float(ray_range[0]), float(ray_range[1])]
        rays, depths, keep = _BuildLidarRays.apply(lidar_pose, dirs_dev, dist_dev, index_dev, rr,
                                                   float(world_cube.scale_factor), shift)
        if ignore_world_cube:
            return rays, depths
        # the reference asserts that origins are inside the cube (ray_utils.py:301-303)
        if rays.shape[0] and bool((rays[0, :3].abs() > 1).any()):
            raise AssertionError("ray origins are outside the world cube")
        valid = keep.bool()
        return rays[valid], depths[valid]


# ---------------------------------------------------------------- camera rays
def undistort_points(points, k, distortion, new_k, iterations=20, tolerance=1e-12):
    """Pixel coordinates [n,2] of a distorted image -> where the same rays land in an undistorted image with intrinsics new_k (fp64
    numpy in and out).  The reference calls kornia's undistort_points here (ray_utils.py:109); this is the definition used instead:
    normalise with k, invert the OpenCV plumb-bob model (distortion = k1, k2, p1, p2 and, when given, k3)
        x_d = x (1 + k1 r^2 + k2 r^4 + k3 r^6) + 2 p1 x y + p2 (r^2 + 2 x^2)
        y_d = y (1 + k1 r^2 + k2 r^4 + k3 r^6) + p1 (r^2 + 2 y^2) + 2 p2 x y
    by the fixed-point iteration x <- (x_d - tangential(x, y)) / radial(x, y) from x = x_d, in fp64, until no coordinate moves by
    `tolerance` or more, or `iterations` rounds have run, and re-project with new_k."""
    pts = np.asarray(points, dtype=np.float64)
    k, new_k = np.asarray(k, dtype=np.float64), np.asarray(new_k, dtype=np.float64)
    d = np.zeros(5)
    coeff = np.asarray(distortion, dtype=np.float64).reshape(-1)
    if coeff.size not in (4, 5):
        raise ValueError(f"undistort_points: 4 or 5 distortion coefficients (k1 k2 p1 p2 [k3]), got {coeff.size}")
    d[:coeff.size] = coeff
    k1, k2, p1, p2, k3 = d
    xd = (pts[:, 0] - k[0, 2]) / k[0, 0]
    yd = (pts[:, 1] - k[1, 2]) / k[1, 1]
    x, y = xd.copy(), yd.copy()
    for _ in range(int(iterations)):
        r2 = x * x + y * y
        radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        xn, yn = (xd - dx) / radial, (yd - dy) / radial
        step = max(float(np.abs(xn - x).max(initial=0.0)), float(np.abs(yn - y).max(initial=0.0)))
        x, y = xn, yn
        if step < tolerance:
            break
    return np.stack([new_k[0, 0] * x + new_k[0, 2], new_k[1, 1] * y + new_k[1, 2]], axis=1)


def get_ray_directions(H, W, newK, dist=None, K=None, sppd=1, with_indices=False):
    """Camera-frame ray directions of every pixel, fp32 [H*W,3] = ((x - cx') / fx', (y - cy') / fy', 1) with the intrinsics newK,
    pixels row-major (x = idx % W, y = idx // W) (ray_utils.py:62-125).  With dist (and K) the pixel grid is first moved to the
    undistorted image plane.  Zero distortion with newK == K leaves the grid as it is - the exact value; otherwise undistort_points
    above, computed in fp64 and rounded once to fp32, DEFINES the result here (the reference's kornia call iterates differently).
    with_indices: also the pixel coordinates x and y, fp32 [H*W,1] each, of the original (distorted) image."""
    newK = torch.as_tensor(newK, dtype=torch.float32).cpu()
    xs = torch.linspace(0, W - 1. / sppd, sppd * W)
    ys = torch.linspace(0, H - 1. / sppd, sppd * H)
    grid_x, grid_y = torch.meshgrid([xs, ys], indexing="ij")
    grid_x = grid_x.permute(1, 0).reshape(-1, 1)
    grid_y = grid_y.permute(1, 0).reshape(-1, 1)
    new_grid_x, new_grid_y = grid_x, grid_y
    if dist is not None:
        assert K is not None
        K = torch.as_tensor(K, dtype=torch.float32).cpu()
        coeff = torch.as_tensor(dist, dtype=torch.float32).reshape(-1).cpu()
        if bool((coeff != 0).any()) or not torch.equal(K, newK):
            und = undistort_points(torch.cat([grid_x, grid_y], dim=-1).double().numpy(), K.double().numpy(), coeff.double().numpy(),
                                   newK.double().numpy())
            und = torch.from_numpy(und).float()
            new_grid_x, new_grid_y = und[:, 0:1], und[:, 1:2]
    directions = torch.cat([(new_grid_x - newK[0, 2]) / newK[0, 0], (new_grid_y - newK[1, 2]) / newK[1, 1],
                            torch.ones_like(grid_x)], -1)
    if with_indices:
        return directions, grid_x, grid_y
    return directions


class CameraRayDirections:
    """Precomputed ray directions of a calibrated camera, and ray records in the reference's format from a camera pose
    (ray_utils.py:128-225).  `directions` [H*W,3], `i_meshgrid` (pixel x) and `j_meshgrid` (pixel y) [H*W,1] are fp32 on `device`
    (None: the mapping device); they are once-per-camera host work (get_ray_directions).  The records are built by
    lnr_build_camera_rays on the HIP device."""

    def __init__(self, calibration, samples_per_pixel: int = 1, device=None, chunk_size=512):
        assert samples_per_pixel == 1, "Only 1 sample per pixel currently supported"
        intrinsic = calibration.camera_intrinsic
        K = torch.as_tensor(intrinsic.k, dtype=torch.float32)
        distortion = torch.as_tensor(intrinsic.distortion, dtype=torch.float32)
        new_k = intrinsic.new_k
        if new_k is None:
            print("Warning: No New K provided. Using K")
            new_k = K
        device = mapping_device() if device is None else torch.device(device)
        self.im_width = int(intrinsic.width)
        self.im_height = int(intrinsic.height)
        directions, i_grid, j_grid = get_ray_directions(self.im_height, self.im_width, newK=new_k, dist=distortion, K=K,
                                                        sppd=samples_per_pixel, with_indices=True)
        self.directions = directions.contiguous().to(device)
        self.i_meshgrid = i_grid.to(device)
        self.j_meshgrid = j_grid.to(device)
        self._chunk_size = chunk_size
        self.num_chunks = -(-self.directions.shape[0] // self._chunk_size)
        self._device_directions = None

    def __len__(self):
        return self.directions.shape[0]

    def _directions_on(self, dev):
        if self.directions.device == dev:
            return self.directions
        if self._device_directions is None or self._device_directions.device != dev:
            self._device_directions = self.directions.to(dev)
        return self._device_directions

    def build_rays(self, camera_indices, pose, image, world_cube: WorldCube, ray_range):
        """-> (rays [n,13] on the HIP device, intensities [n,C] or None).  camera_indices: pixel indices in [0, H*W), or None for
        the whole image in order.  The pose is read, not modified (the reference shifts the matrix it is handed and its callers
        clone, analysis/renderer.py:185), and no gradient reaches it: a pose that requires grad is detached."""
        dev = mapping_device()
        T = pose.get_transformation_matrix() if hasattr(pose, "get_transformation_matrix") else torch.as_tensor(pose)
        T12 = T.detach()[:3, :4].to(device=dev, dtype=torch.float32).contiguous().reshape(12)
        index = None
        if camera_indices is not None:
            index = torch.as_tensor(camera_indices).detach().to(device=dev, dtype=torch.int64).reshape(-1)
            if index.numel() and (int(index.min()) < 0 or int(index.max()) >= len(self)):
                raise IndexError(f"camera_indices outside the image's {len(self)} pixels")
        shift = world_cube.shift.detach().cpu().reshape(-1).tolist()
        rays = ops.build_camera_rays(self._directions_on(dev), index, self.im_width, T12, float(ray_range[0]),
                                     float(world_cube.scale_factor), shift)
        intensities = None
        if image is not None:
            img = image.image
            flat = img.reshape(-1, img.shape[2])
            intensities = flat if camera_indices is None else flat[torch.as_tensor(camera_indices).to(flat.device)]
        return rays, intensities

    def fetch_chunk_rays(self, chunk_idx: int, pose, world_cube: WorldCube, ray_range):
        start = chunk_idx * self._chunk_size
        end = min(len(self), (chunk_idx + 1) * self._chunk_size)
        return self.build_rays(torch.arange(start, end, 1), pose, None, world_cube, ray_range)[0]
