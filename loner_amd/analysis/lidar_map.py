"""Rendered LiDAR maps and their accuracy / completion / F-score (the reference's analysis/renderer_lidar.py and
analysis/evaluate_lidar_map.py::compare_point_clouds), on HIP and without open3d.

LidarMapRenderer renders a dense synthetic scan from keyframe poses through Model.forward(testing=True, return_variance=True),
keeps the confident rays (ops.lidar_scan_points), voxel-down-samples each scan in the sensor frame, moves it to the world frame
while appending it to the merged cloud (ops.cloud_transform) and down-samples the merged cloud once more (renderer_lidar.py:71-91,
:296-349).  compare_point_clouds down-samples both clouds and takes exact nearest-neighbour distances both ways on the device
(ops.NNGrid) before deriving the reference's statistics (evaluate_lidar_map.py:58-80).  With refine_alignment=True it first refines
the alignment by point-to-plane ICP on the device (evaluate_lidar_map.py:23-53: registration_icp, ops.icp_point_to_plane), and
evaluate_lidar_map restates the script's entry point (:101-148) with the refinement on.  Differences from the reference, by intent:
  * the refinement is opt-in on compare_point_clouds (on in evaluate_lidar_map); its alignment subsets follow the ascending voxel
    order (open3d's follows its hash map), so the refined transform is not open3d's even in principle; the source normals, which no
    output reads, are not estimated; a degenerate or non-finite solve raises instead of propagating NaN;
  * no est_align.pcd / gt_align.pcd in the working directory;
  * voxel_down_sample returns its voxels in ascending (i_x, i_y, i_z) order; open3d's order is its hash map's;
  * a ray the cube test drops gives no point (the reference would fail to assign a shorter chunk into its fixed slice);
  * an empty cloud after down-sampling raises ValueError (the reference divides by zero), and the statistics are returned.
"""
import os

import numpy as np
import torch

from .. import ops
from ..common.pose import Pose
from ..common.ray_utils import device_scan, mapping_device
from .mesher import build_lidar_scan


def _device(device):
    if device is None:
        return mapping_device()
    return torch.device("cuda", device) if isinstance(device, int) else torch.device(device)


class PointCloud:
    """fp64 points [n,3] on the HIP device; the part of open3d's PointCloud the evaluation uses.  normals [n,3] and covariances
    [n,3,3] (fp64, on the device) are None until estimated."""

    def __init__(self, points=None, device=None):
        pts = torch.zeros(0, 3, dtype=torch.float64) if points is None else points
        pts = pts if torch.is_tensor(pts) else torch.from_numpy(np.asarray(pts, dtype=np.float64))
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"PointCloud: points [n,3], got {tuple(pts.shape)}")
        dev = pts.device if device is None and pts.is_cuda else _device(device)
        self.points = pts.to(device=dev, dtype=torch.float64).contiguous()
        self.normals = None
        self.covariances = None

    def has_normals(self):
        return self.normals is not None and len(self) > 0

    def estimate_normals(self, knn=30, cell_edge=None):
        """open3d's estimate_normals(KDTreeSearchParamKNN(knn)) (include/loner_hip.h: lnr_cloud_normals).  As open3d does, a normal
        that points against one already present is flipped.  cell_edge: the search grid's (the normals do not depend on it)."""
        normals = ops.NNGrid(self.points, cell_edge).normals(knn) if len(self) else torch.zeros(0, 3, dtype=torch.float64,
                                                                                                  device=self.points.device)
        if self.normals is not None and self.normals.shape == normals.shape:
            flip = (normals * self.normals).sum(1, keepdim=True) < 0
            normals = torch.where(flip, -normals, normals)
        self.normals = normals
        return self

    def estimate_covariances(self, knn=30, cell_edge=None):
        """open3d's estimate_covariances(KDTreeSearchParamKNN(knn)): the covariances of the k-nearest neighbourhoods."""
        if len(self):
            _, self.covariances = ops.NNGrid(self.points, cell_edge).normals(knn, want_covariances=True)
        else:
            self.covariances = torch.zeros(0, 3, 3, dtype=torch.float64, device=self.points.device)
        return self

    def _orient(self, what, **how):
        if self.normals is None:
            raise ValueError(f"{what}: the cloud has no normals (call estimate_normals())")
        from .registration import orient_normals
        orient_normals(self.normals, self.points, **how)
        return self

    def orient_normals_towards_location(self, location=(0.0, 0.0, 0.0)):
        """open3d's orient_normals_towards_camera_location, in place (include/loner_hip.h: lnr_cloud_orient_normals): a normal is
        flipped when it points away from `location`; non-finite normals are left as they are."""
        return self._orient("orient_normals_towards_location", location=location)

    def orient_normals_to_align_with_direction(self, direction=(0.0, 0.0, 1.0)):
        """open3d's orient_normals_to_align_with_direction, in place: a normal is flipped when its dot product with `direction` is
        negative."""
        return self._orient("orient_normals_to_align_with_direction", direction=direction)

    def compute_fpfh_feature(self, radius, max_nn=32, cell_edge=None):
        """open3d's compute_fpfh_feature(cloud, KDTreeSearchParamHybrid(radius, max_nn)) (include/loner_hip.h: lnr_cloud_fpfh) ->
        features [n,33] fp64 on the device, row i = point i (open3d's Feature.data transposed).  max_nn <= 32.  The cloud needs
        normals, consistently oriented: FPFH depends on their sign."""
        if self.normals is None:
            raise ValueError("compute_fpfh_feature: the cloud has no normals (call estimate_normals() and orient them)")
        if len(self) == 0:
            return torch.zeros(0, 33, dtype=torch.float64, device=self.points.device)
        from .registration import fpfh
        return fpfh(ops.NNGrid(self.points, cell_edge), self.normals, radius, max_nn)

    def uniform_down_sample(self, every_k_points):
        """A new cloud of the points whose index i satisfies i % every_k_points == 0, in order (with their normals and covariances)."""
        k = int(every_k_points)
        if k < 1:
            raise ValueError(f"uniform_down_sample: every_k_points must be >= 1, got {every_k_points!r}")
        out = PointCloud(self.points[::k].contiguous())
        out.normals = None if self.normals is None else self.normals[::k].contiguous()
        out.covariances = None if self.covariances is None else self.covariances[::k].contiguous()
        return out

    def remove_statistical_outlier(self, nb_neighbors=20, std_ratio=1.5, cell_edge=None):
        """open3d's remove_statistical_outlier -> (a new cloud of the kept points in input order, with their normals and covariances;
        their indices, int64 on the device).  A point is kept when the mean distance to its nb_neighbors nearest points (itself
        included) is > 0 and below mean + std_ratio * std over the cloud (include/loner_hip.h: lnr_cloud_knn_mean_distance,
        lnr_cloud_outlier_threshold).  cell_edge: the search grid's (the result does not depend on it)."""
        if nb_neighbors < 1 or not std_ratio > 0:
            raise ValueError(f"remove_statistical_outlier: nb_neighbors >= 1 and std_ratio > 0, got {nb_neighbors!r} and {std_ratio!r}")
        if len(self) == 0:
            return PointCloud(self.points.clone()), torch.zeros(0, dtype=torch.int64, device=self.points.device)
        grid = ops.NNGrid(self.points, cell_edge)
        avg = grid.knn_mean_distance(nb_neighbors)
        threshold = grid.outlier_threshold(avg, std_ratio)[2]
        index = ((avg > 0) & (avg < threshold)).nonzero().squeeze(1)
        out = PointCloud(self.points[index])
        out.normals = None if self.normals is None else self.normals[index].contiguous()
        out.covariances = None if self.covariances is None else self.covariances[index].contiguous()
        return out, index

    def select_by_index(self, index):
        """A new cloud of the points at `index` (int64 on the device), with their normals and covariances."""
        out = PointCloud(self.points[index])
        out.normals = None if self.normals is None else self.normals[index].contiguous()
        out.covariances = None if self.covariances is None else self.covariances[index].contiguous()
        return out

    def remove_radius_outlier(self, nb_points, radius):
        """open3d's remove_radius_outlier -> (a new cloud of the kept points in input order, with their normals and covariances;
        their indices, int64 on the device).  A point is kept when more than nb_points points lie within `radius` of it (d2 <
        radius^2, strict), itself counted as open3d counts it (include/loner_hip.h: lnr_cloud_radius_count).  The search grid's cell
        edge is the radius; the result does not depend on it."""
        from ..ops._common import _positive
        from .segmentation import radius_count
        r = _positive(radius, "remove_radius_outlier", "radius")
        if int(nb_points) != nb_points or nb_points < 0:
            raise ValueError(f"remove_radius_outlier: nb_points must be an integer >= 0, got {nb_points!r}")
        if len(self) == 0:
            return PointCloud(self.points.clone()), torch.zeros(0, dtype=torch.int64, device=self.points.device)
        index = (radius_count(ops.NNGrid(self.points, r), r) > int(nb_points)).nonzero().squeeze(1)
        return self.select_by_index(index), index

    def cluster_dbscan(self, eps, min_points, info=None):
        """open3d's cluster_dbscan -> labels int32 [n] on the device, -1 for noise (include/loner_hip.h: lnr_cloud_dbscan): clusters
        are the connected components of the core points (at least min_points points within eps, itself counted), numbered by their
        smallest core index; a border point takes the smallest label among the cores within eps.  These are open3d's labels, and
        two runs give the same bytes.  info (a dict, optional) receives {clusters, cores, border, noise} (one device -> host read).
        The search grid's cell edge is eps."""
        from .segmentation import dbscan, dbscan_args
        e, k = dbscan_args("cluster_dbscan", eps, min_points)
        if len(self) == 0:
            if info is not None:
                info.update(clusters=0, cores=0, border=0, noise=0)
            return torch.zeros(0, dtype=torch.int32, device=self.points.device)
        labels, words = dbscan(ops.NNGrid(self.points, e), e, k)
        if info is not None:
            w = [int(x) for x in words.cpu()]
            info.update(clusters=w[1], cores=w[2], border=w[3], noise=w[4])
        return labels

    def remove_small_clusters(self, eps, min_points, min_cluster_points):
        """The floaters of a cloud, as meshes have remove_small_components -> (a new cloud, the kept indices int64 on the device):
        the points whose DBSCAN cluster (cluster_dbscan(eps, min_points)) has at least min_cluster_points members; noise goes.  The
        cluster sizes are a histogram on the device."""
        if int(min_cluster_points) != min_cluster_points or min_cluster_points < 0:
            raise ValueError(f"remove_small_clusters: min_cluster_points must be an integer >= 0, got {min_cluster_points!r}")
        labels = self.cluster_dbscan(eps, min_points).to(torch.int64)
        if len(self) == 0:
            return PointCloud(self.points.clone()), labels
        sizes = torch.bincount(labels + 1)                       # slot 0: noise
        sizes[0] = -1
        index = (sizes[labels + 1] >= int(min_cluster_points)).nonzero().squeeze(1)
        return self.select_by_index(index), index

    def segment_plane(self, distance_threshold, num_iterations=1000, seed=0, refine=True, info=None):
        """open3d's segment_plane with ransac_n = 3 (include/loner_hip.h: lnr_cloud_segment_plane) -> (plane_model numpy fp64 [4]
        (a, b, c, d), the inliers' indices int64 on the device, ascending).  num_iterations is the fixed number of hypotheses (no
        probability-based stop) and the draws are counter-based: the result depends on the arguments only.  The inliers are the best
        hypothesis's, as open3d's are; with refine the model is refitted to them.  Fewer than 3 points, or no usable hypothesis:
        a zero model and no inliers.  info (a dict, optional) receives analysis.segmentation.plane_ransac's dictionary."""
        from .segmentation import plane_ransac
        out = plane_ransac(self.points, distance_threshold, num_iterations, seed, refine)
        if info is not None:
            info.update(out)
        return out["plane"], out["inlier"].nonzero().squeeze(1)

    def __len__(self):
        return int(self.points.shape[0])

    def numpy(self):
        return self.points.cpu().numpy()

    def voxel_down_sample(self, voxel_size):
        """A new cloud: one point per occupied voxel, the mean of its points, in ascending voxel order (include/loner_hip.h:
        lnr_voxel_down_sample)."""
        return PointCloud(ops.voxel_down_sample(self.points, voxel_size))

    def transform(self, T):
        """Applies the 4x4 affine T (widened to fp64) in place and returns self, as open3d does: normals are rotated by T[:3,:3]
        (with the same rounding, a zero translation) and covariances become R C R^T."""
        ops.cloud_transform(self.points, T, out=self.points)
        if self.normals is not None or self.covariances is not None:
            T = ops.affine_f64(T, "transform: T must be a 4x4 affine matrix with bottom row [0, 0, 0, 1]")
            R = np.eye(4)
            R[:3, :3] = T[:3, :3]
            if self.normals is not None:
                ops.cloud_transform(self.normals, R, out=self.normals)
            if self.covariances is not None:
                Rd = torch.from_numpy(R[:3, :3]).to(self.covariances.device)
                self.covariances = (Rd @ self.covariances @ Rd.T).contiguous()
        return self

    def compute_point_cloud_distance(self, target, cell_edge=None, stats=None):
        """numpy fp64 [n]: for every point the exact distance to its nearest point of `target` (0 when target is empty).
        cell_edge: the search grid's cell edge (None: the default rule; the distances do not depend on it); stats: an optional
        dict that receives the search's counters."""
        grid = ops.NNGrid(target.points.to(self.points.device), cell_edge)
        return grid.distance(self.points, stats=stats).cpu().numpy()


# ---------------------------------------------------------------- PCD v0.7
_PCD_TYPES = {("F", 4): "<f4", ("F", 8): "<f8", ("I", 1): "i1", ("I", 2): "<i2", ("I", 4): "<i4", ("I", 8): "<i8", ("U", 1): "u1",
              ("U", 2): "<u2", ("U", 4): "<u4", ("U", 8): "<u8"}


def read_point_cloud(path, device=None):
    """A PointCloud from a PCD v0.7 file (ascii or binary) whose x y z fields are F4 or F8; other fields are skipped."""
    return PointCloud(read_pcd(path), device)


def read_pcd(path):
    """float64 [n,3]: the x y z fields of a PCD v0.7 file (read_point_cloud without the device)."""
    with open(path, "rb") as f:
        head = {}
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: PCD header without DATA")
            line = line.decode("ascii", "replace").strip()
            if not line or line.startswith("#"):
                continue
            key, _, rest = line.partition(" ")
            head[key.upper()] = rest.split()
            if key.upper() == "DATA":
                break
        body = f.read()
    fields = head["FIELDS"]
    sizes = [int(s) for s in head.get("SIZE", ["4"] * len(fields))]
    types = head.get("TYPE", ["F"] * len(fields))
    counts = [int(c) for c in head.get("COUNT", ["1"] * len(fields))]
    n = int(head["POINTS"][0]) if "POINTS" in head else int(head["WIDTH"][0]) * int(head.get("HEIGHT", ["1"])[0])
    data = head["DATA"][0].lower()
    for a in "xyz":
        if a not in fields:
            raise ValueError(f"{path}: no {a} field")
        k = fields.index(a)
        if types[k] != "F" or sizes[k] not in (4, 8) or counts[k] != 1:
            raise ValueError(f"{path}: field {a} is {types[k]}{sizes[k]} x {counts[k]}; x y z must be F4 or F8")
    if data == "binary_compressed":
        raise ValueError(f"{path}: PCD DATA binary_compressed is not supported (ascii and binary are)")
    if data == "binary":
        dt = np.dtype([(f"f{k}", _PCD_TYPES[(t, s)], (c,)) for k, (t, s, c) in enumerate(zip(types, sizes, counts))])
        rec = np.frombuffer(body[:n * dt.itemsize], dtype=dt, count=n)
        pts = np.stack([rec[f"f{fields.index(a)}"][:, 0].astype(np.float64) for a in "xyz"], axis=1)
    elif data == "ascii":
        col = np.cumsum([0] + counts)
        rows = [r.split() for r in body.decode("ascii").splitlines() if r.strip()][:n]
        pts = np.empty((len(rows), 3), dtype=np.float64)
        for j, a in enumerate("xyz"):
            k = fields.index(a)
            v = np.array([float(r[col[k]]) for r in rows], dtype=np.float64)
            pts[:, j] = v.astype(np.float32).astype(np.float64) if sizes[k] == 4 else v
    else:
        raise ValueError(f"{path}: unknown PCD DATA {data!r}")
    return pts.reshape(-1, 3)


def write_point_cloud(path, cloud, write_ascii=False):
    """PCD v0.7 with x y z as F4 (the fields and type open3d writes for a cloud without colours or normals)."""
    pts = cloud.numpy() if isinstance(cloud, PointCloud) else np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    pts = pts.astype(np.float32)
    n = pts.shape[0]
    head = ["# .PCD v0.7 - Point Cloud Data file format", "VERSION 0.7", "FIELDS x y z", "SIZE 4 4 4", "TYPE F F F", "COUNT 1 1 1",
            f"WIDTH {n}", "HEIGHT 1", "VIEWPOINT 0 0 0 1 0 0 0", f"POINTS {n}", f"DATA {'ascii' if write_ascii else 'binary'}"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if write_ascii:
            f.write("".join(f"{x!r} {y!r} {z!r}\n" for x, y, z in pts.astype(np.float64).tolist()).encode("ascii"))
        else:
            f.write(np.ascontiguousarray(pts, dtype="<f4").tobytes())
    return True


# ---------------------------------------------------------------- rendering
class LidarMapRenderer:
    """The reference's renderer_lidar.py as a class in Mesher's pattern: render_scan (sensor frame) and render_map (world frame,
    metres, merged over keyframe poses)."""

    def __init__(self, model, ckpt, world_cube, ray_range, lidar_vertical_fov=[-22.5, 22.5], resolution=0.1):
        self.model = model
        self.ckpt = ckpt
        self.world_cube = world_cube
        self.ray_range = ray_range
        self.lidar_vertical_fov = lidar_vertical_fov
        self.resolution = resolution
        self._scans = {}

    def _scan(self, device):
        scan = self._scans.get(str(device))
        if scan is None:
            scan = self._scans[str(device)] = build_lidar_scan({"vertical_fov": self.lidar_vertical_fov, "vertical_resolution": self.resolution,
                                                                "horizontal_resolution": self.resolution}, device)
        return scan

    def scan_rays(self, lidar_pose, device=None):
        """-> (rays [m,13] of the rays the cube test keeps, their scan indices int64 [m], the scan's directions [3,N] fp32), all on
        the device: the input of render_scan's one Model.forward call."""
        dev = _device(device)
        dirs, dist = device_scan(self._scan(dev), dev)
        T = lidar_pose.get_transformation_matrix() if isinstance(lidar_pose, Pose) else torch.as_tensor(lidar_pose)
        T12 = T.detach()[:3, :4].to(device=dev, dtype=torch.float32).contiguous().reshape(12)
        rr = [float(self.ray_range[0]), float(self.ray_range[1])]
        shift = self.world_cube.shift.detach().cpu().reshape(-1).tolist()
        index = torch.arange(dirs.shape[1], device=dev, dtype=torch.int64)
        rays, _, keep = ops.build_lidar_rays(dirs, dist, index, T12, rr, float(self.world_cube.scale_factor), shift)
        if rays.shape[0] and bool((rays[0, :3].abs() > 1).any()):
            raise AssertionError("ray origins are outside the world cube")
        kept = keep.bool().nonzero().squeeze(1)
        return rays[kept], kept, dirs

    def _thresholds(self, var_threshold):
        """fp32 (scale, variance bound, depth bound): the reference's fp32 products and compares (renderer_lidar.py:83-88)"""
        scale = float(np.float32(float(self.world_cube.scale_factor)))
        return scale, float(np.float32(var_threshold)), float(np.float32(float(self.ray_range[1]) - 0.25))

    def _scan_points(self, lidar_pose, ray_sampler, var_threshold, device=None):
        rays, kept, dirs = self.scan_rays(lidar_pose, device)
        scale, var_max, depth_max = self._thresholds(var_threshold)
        if rays.shape[0] == 0:
            return torch.zeros(0, 3, device=dirs.device, dtype=torch.float64), torch.zeros(1, device=dirs.device, dtype=torch.int32)
        with torch.no_grad():
            out = self.model(rays, ray_sampler, self.world_cube.scale_factor, testing=True, return_variance=True, camera=False)
        return ops.lidar_scan_points(out["depth_fine"], out["variance"], kept, dirs, scale, var_max, depth_max)

    def render_scan(self, lidar_pose, ray_sampler, var_threshold=1e-2, device=None):
        """PointCloud of one pose in the sensor frame (metres): the kept rays' points in ray order (renderer_lidar.py:71-91)."""
        pts, count = self._scan_points(lidar_pose, ray_sampler, var_threshold, device)
        return PointCloud(pts[:int(count.item())])

    def render_map(self, device, ray_sampler, voxel_size, skip_step=5, var_threshold=1e-2, use_gt_poses=False, only_last_frame=False):
        """PointCloud of the map in the world frame (metres): every selected pose's scan, down-sampled in the sensor frame, transformed
        and merged in pose order, then down-sampled once more (renderer_lidar.py:278-290, :296-349).  voxel_size None: no
        down-sampling, as in the reference."""
        dev = _device(device)
        poses = self.ckpt["poses"]
        selected = [poses[-1]] if only_last_frame else poses[::skip_step]
        key = "gt_lidar_pose" if use_gt_poses else "lidar_pose"
        merged = torch.empty(0, 3, device=dev, dtype=torch.float64)
        total = 0
        for pose_state in selected:
            lidar_pose = Pose(pose_tensor=pose_state[key]).to(dev) if isinstance(pose_state, dict) else Pose(pose_state).to(dev)
            pts, count = self._scan_points(lidar_pose, ray_sampler, var_threshold, dev)
            scan = ops.voxel_down_sample(pts, voxel_size, count) if voxel_size is not None else pts[:int(count.item())]
            k = scan.shape[0]
            if total + k > merged.shape[0]:
                grown = torch.empty(max(2 * merged.shape[0], total + k), 3, device=dev, dtype=torch.float64)
                grown[:total] = merged[:total]
                merged = grown
            ops.cloud_transform(scan, lidar_pose.get_transformation_matrix(), out=merged[total:total + k])
            total += k
        cloud = PointCloud(merged[:total])
        return cloud.voxel_down_sample(voxel_size) if voxel_size is not None else cloud


# ---------------------------------------------------------------- alignment
class RegistrationResult:
    """open3d's RegistrationResult: transformation (numpy fp64 4x4), fitness, inlier_rmse, and n_correspondences and iterations
    (rounds run)."""

    def __init__(self, transformation, fitness, inlier_rmse, n_correspondences, iterations):
        self.transformation = transformation
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.n_correspondences = n_correspondences
        self.iterations = iterations

    def as_dict(self):
        return {"transformation": self.transformation.tolist(), "fitness": self.fitness, "inlier_rmse": self.inlier_rmse,
                "n_correspondences": self.n_correspondences, "iterations": self.iterations}


def registration_icp(source, target, max_correspondence_distance, init=np.eye(4), relative_fitness=1e-6, relative_rmse=1e-6,
                     max_iteration=30):
    """open3d's registration_icp(source, target, d, init, TransformationEstimationPointToPlane(),
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)) on the device (ops.icp_point_to_plane).  The target needs
    normals (ValueError otherwise, as open3d); the source's are not read.  The search grid's cell edge is the correspondence
    distance."""
    if target.normals is None:
        raise ValueError("registration_icp: point-to-plane ICP needs the target's normals (call target.estimate_normals())")
    r = float(max_correspondence_distance)
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"registration_icp: max_correspondence_distance must be finite and > 0, got {max_correspondence_distance!r}")
    grid = ops.NNGrid(target.points, r)
    out = ops.icp_point_to_plane(grid, target.normals, source.points.to(target.points.device), r, init, relative_fitness, relative_rmse,
                                 max_iteration)
    return RegistrationResult(out["transformation"], out["fitness"], out["inlier_rmse"], out["n_correspondences"], out["iterations"])


def alignment_skip(n):
    """evaluate_lidar_map.py:26-29: the uniform_down_sample step of a cloud of n points."""
    return int(n / 1_000_000) if n > 1_000_000 else 1


def refine_alignment_icp(est_scan, gt_scan, kernel=None):
    """evaluate_lidar_map.py:23-53 on down-sampled clouds: the alignment subsets, the target's normals (knn 30), and 10 rounds of
    point-to-plane ICP at 0.125 m from the identity with criteria 1e-12.  -> RegistrationResult (est_scan is not moved).  kernel: an
    analysis.registration.RobustKernel on the residuals (the clouds hold gross outliers by construction: unobserved ground truth and
    floaters); None is the reference's plain L2 call."""
    gt_alignment = gt_scan.uniform_down_sample(alignment_skip(len(gt_scan)))
    est_alignment = est_scan.uniform_down_sample(alignment_skip(len(est_scan)))
    print("Estimating point cloud normals")
    gt_alignment.estimate_normals(30)
    print("Refining alignment")
    if kernel is not None:
        from .registration import registration_icp_robust
        return registration_icp_robust(est_alignment, gt_alignment, 0.125, np.eye(4), 1e-12, 1e-12, 10, kernel)
    return registration_icp(est_alignment, gt_alignment, 0.125, np.eye(4), 1e-12, 1e-12, 10)


# ---------------------------------------------------------------- evaluation
def compare_point_clouds(est_scan, gt_scan, output_dir, f_score_threshold, voxel_size=0.05, write_pointclouds=False,
                         write_gt_cloud=False, id_str=None, refine_alignment=False, alignment=None, alignment_kernel=None,
                         global_alignment=False, min_cluster_points=0, cluster_eps=None, cluster_min_points=4):
    """Accuracy, completion, Chamfer distance, precision, recall and F-score of est_scan against gt_scan after down-sampling both
    (evaluate_lidar_map.py:16-98).  refine_alignment: first move the down-sampled estimate by point-to-plane ICP
    (refine_alignment_icp; evaluate_lidar_map.py:23-53); alignment (a dict, optional) receives the ICP result; alignment_kernel (an
    analysis.registration.RobustKernel, optional) is the refinement's loss.  global_alignment: before that, move the down-sampled
    estimate onto the ground truth by analysis.registration.global_registration (for maps that are metres or a half turn apart, where
    ICP from the identity finds nothing): True for its defaults at 10 voxel_size, or a dict of its keyword arguments (voxel_size,
    orient, hypotheses, seed); alignment["global"] receives its result.  min_cluster_points > 0: before anything else the floaters
    of the *estimated* cloud go (PointCloud.remove_small_clusters(cluster_eps or 2 * voxel_size, cluster_min_points,
    min_cluster_points) on the cloud as given), and the statistics gain "removed_floaters", the number of points removed; with 0
    nothing changes.  Writes
    {output_dir}/metrics/statistics{_id}.yaml and, when asked, lidar_renders/rendered{_id}.pcd and gt{_id}.pcd; returns the
    statistics.  Quirks kept: precision = TP / len(accuracy), recall = TP / (TP + FN) with TP counted on the estimate and FN on the
    ground truth, and 1e-8 in the F-score's denominator."""
    import yaml
    removed = None
    if min_cluster_points > 0:
        eps = 2.0 * voxel_size if cluster_eps is None else cluster_eps
        print(f"Removing clusters of fewer than {min_cluster_points} points (eps {eps})")
        kept, _ = est_scan.remove_small_clusters(eps, cluster_min_points, min_cluster_points)
        removed = len(est_scan) - len(kept)
        est_scan = kept
    print("Downsampling clouds to voxel size", voxel_size)
    est_scan = est_scan.voxel_down_sample(voxel_size)
    gt_scan = gt_scan.voxel_down_sample(voxel_size)
    if len(est_scan) == 0 or len(gt_scan) == 0:
        raise ValueError(f"compare_point_clouds: {len(est_scan)} estimated and {len(gt_scan)} ground-truth points after down-sampling")
    if global_alignment:
        from .registration import global_registration
        print("Aligning the clouds globally")
        how = dict(global_alignment) if isinstance(global_alignment, dict) else {}
        how.setdefault("voxel_size", 10.0 * voxel_size)
        rough = global_registration(est_scan, gt_scan, kernel=alignment_kernel, **how)
        est_scan.transform(rough.transformation)
        if alignment is not None:
            alignment["global"] = rough.as_dict()
    if refine_alignment:
        reg = refine_alignment_icp(est_scan, gt_scan, alignment_kernel)
        est_scan.transform(reg.transformation)
        if alignment is not None:
            alignment.update(reg.as_dict())
    print("Computing metrics")
    edge = 2.0 * voxel_size          # a cell then meets at most 27 occupied voxels of either cloud
    accuracy = est_scan.compute_point_cloud_distance(gt_scan, cell_edge=edge)
    completion = gt_scan.compute_point_cloud_distance(est_scan, cell_edge=edge)
    chamfer_distance = accuracy.mean() + completion.mean()

    false_negatives = (completion > f_score_threshold).sum().item()
    false_positives = (accuracy > f_score_threshold).sum().item()
    true_positives = (len(accuracy) - false_positives)

    precision = true_positives / (true_positives + false_positives)
    recall = true_positives / (true_positives + false_negatives)
    f_score = 2 * (precision * recall) / (precision + recall + 1e-8)

    stats = {
        "accuracy": accuracy.mean().item(),
        "completion": completion.mean().item(),
        "chamfer_distance": chamfer_distance.item(),
        "recall": recall,
        "precision": precision,
        "f-score": f_score,
        "num_points": len(accuracy)
    }
    if removed is not None:
        stats["removed_floaters"] = removed

    metrics_dir = f"{output_dir}/metrics"
    os.makedirs(metrics_dir, exist_ok=True)
    id_suffix = f"_{id_str}" if id_str is not None else ""
    if write_pointclouds:
        renders_dir = f"{output_dir}/lidar_renders/"
        os.makedirs(renders_dir, exist_ok=True)
        write_point_cloud(f"{renders_dir}/rendered{id_suffix}.pcd", est_scan)
        if write_gt_cloud:
            write_point_cloud(f"{renders_dir}/gt{id_suffix}.pcd", gt_scan)
    with open(f"{metrics_dir}/statistics{id_suffix}.yaml", 'w+') as yaml_stats_f:
        yaml.dump(stats, yaml_stats_f, indent=2)
    return stats


def evaluate_lidar_map(experiment_directory, gt_map, gt_trajectory=None, estimated_map=None, f_score_threshold=0.1, voxel_size=0.05,
                       initial_transform=None, est_traj=None, alignment=None, global_alignment=False, min_cluster_points=0,
                       cluster_eps=None):
    """The entry point of evaluate_lidar_map.py (:101-148) with the refinement on: reads the estimated map (default
    {experiment_directory}/lidar_renders/render_full.pcd, else {experiment_directory}/{estimated_map}) and gt_map, rough-aligns the
    ground truth by the inverse of initial_transform (16 numbers, row-major) or of the first pose of the TUM trajectory gt_trajectory,
    and the estimate by the inverse of est_traj's first pose when given, then scores them (compare_point_clouds, refine_alignment=True).
    The reference's rounding is kept: both start poses are fp32 (torch.tensor of the list; build_poses_from_df's .float()), inverted in
    fp32 and widened.  global_alignment: compare_point_clouds', for maps without a trajectory to rough-align them by; min_cluster_points and
    cluster_eps: compare_point_clouds' floater removal (off at 0).  Returns the statistics."""
    from ..common.pose_utils import build_poses_from_df, read_tum
    est_map_path = (f"{experiment_directory}/lidar_renders/render_full.pcd" if estimated_map is None
                    else f"{experiment_directory}/{estimated_map}")
    if gt_trajectory is None and initial_transform is None:
        print("Warning: No GT trajectory provided. Can't rough align maps")
        start_pose = torch.eye(4)
    elif initial_transform is not None:
        print("Using supplied initial guess to rough-align clouds")
        start_pose = torch.tensor([float(x) for x in np.asarray(initial_transform, dtype=np.float64).reshape(-1)]).reshape(4, 4)
    else:
        print("Using GT Trajectory to rough-align clouds")
        start_pose = build_poses_from_df(read_tum(gt_trajectory), False)[0][0]
    est_map = read_point_cloud(est_map_path)
    gt_map = read_point_cloud(gt_map)
    if est_traj is not None:
        start_est_pose = build_poses_from_df(read_tum(est_traj), False)[0][0]
        est_map.transform(start_est_pose.inverse().cpu().numpy())
    gt_map.transform(start_pose.inverse().cpu().numpy())
    return compare_point_clouds(est_map, gt_map, experiment_directory, f_score_threshold, voxel_size, refine_alignment=True,
                                alignment=alignment, global_alignment=global_alignment, min_cluster_points=min_cluster_points,
                                cluster_eps=cluster_eps)
