"""Scoring a mesh against a ground-truth cloud (the reference's analysis/compute_metrics/maps/mesh_to_pcd.py followed by
evaluate_lidar_map.py::compare_point_clouds), on HIP and without open3d.

mesh_to_point_cloud samples the mesh's surface uniformly (TriangleMesh.sample_points_uniformly: include/loner_hip.h,
lnr_mesh_sample_points) and voxel-down-samples the result; evaluate_mesh hands that cloud to compare_point_clouds.  Differences from
the reference, by intent:
  * the draws are Philox4x32-10 by point index, not open3d's mt19937 sequence: the sampled cloud is a function of (mesh, count, seed)
    and the same on every run, but it is not open3d's cloud;
  * the cumulative area is summed as a 64-ary tree, open3d's one addition after the other; the two differ in the last bits, which can
    move a triangle's share by one point;
  * the script's unused camera-to-LiDAR constants (T_lc) are not restated.

evaluate_mesh_to_mesh has no counterpart in the reference: where the ground truth is a mesh (a simulated sequence's, a survey's) it
scores against the surface itself - the exact point-to-triangle distance of analysis/raycast.py - so the ground truth is not sampled
into a cloud and no figure carries that cloud's density or a voxel size.  cloud_to_mesh_distance is its building block.
"""
import os

from .lidar_map import compare_point_clouds, write_point_cloud
from .mesher import TriangleMesh


def mesh_to_point_cloud(mesh_or_ply_path, resolution, number_of_points=50_000_000, seed=0, device=None):
    """mesh_to_pcd.py: number_of_points uniform samples of the mesh, then voxel_down_sample(resolution) -> PointCloud.  Given a path,
    the mesh is read from the .ply and the cloud is also written to <path without its extension>_sampled.pcd, as the script does."""
    path = mesh_or_ply_path if isinstance(mesh_or_ply_path, (str, os.PathLike)) else None
    mesh = TriangleMesh.read_ply(path) if path is not None else mesh_or_ply_path
    cloud = mesh.sample_points_uniformly(number_of_points, seed=seed, device=device)
    if len(cloud):
        cloud = cloud.voxel_down_sample(resolution)
    print(f"Downsampled from {number_of_points} to {len(cloud)}.")
    if path is not None:
        out = f"{os.path.splitext(os.fspath(path))[0]}_sampled.pcd"
        print(f"Saving to {out}")
        write_point_cloud(out, cloud)
    return cloud


def evaluate_mesh(mesh, gt_cloud, output_dir, f_score_threshold=0.1, voxel_size=0.05, resolution=None, number_of_points=50_000_000,
                  seed=0, min_component_triangles=None, **compare_kwargs):
    """Accuracy, completion and F-score of a mesh (a TriangleMesh or a .ply path) against the PointCloud gt_cloud: the mesh is sampled
    (mesh_to_point_cloud at `resolution`, default voxel_size, with its number_of_points and seed) and scored by compare_point_clouds,
    whose statistics are returned.  min_component_triangles = k: a copy of the mesh without its connected components of fewer than k
    triangles (TriangleMesh.remove_small_components) is scored; the caller's mesh and file stay as they are."""
    if min_component_triangles is not None:
        given = TriangleMesh.read_ply(mesh) if isinstance(mesh, (str, os.PathLike)) else mesh
        mesh = TriangleMesh(given.vertices, given.triangles)
        mesh.remove_small_components(min_triangles=min_component_triangles, device=gt_cloud.points.device)
    cloud = mesh_to_point_cloud(mesh, voxel_size if resolution is None else resolution, number_of_points, seed,
                                device=gt_cloud.points.device)
    return compare_point_clouds(cloud, gt_cloud, output_dir, f_score_threshold, voxel_size, **compare_kwargs)


def cloud_to_mesh_distance(cloud_or_points, scene, max_distance=float("inf")):
    """The exact distance fp64 [n], on the device, from every point of a PointCloud (or of points [n,3]) to the surface of scene (a
    RaycastingScene): RaycastingScene.compute_distance.  +inf where no triangle lies within max_distance."""
    from .raycast import RaycastingScene
    if not isinstance(scene, RaycastingScene):
        raise ValueError(f"cloud_to_mesh_distance: scene must be a RaycastingScene, got {type(scene).__name__}")
    points = cloud_or_points.points if hasattr(cloud_or_points, "points") else cloud_or_points
    if len(getattr(points, "shape", ())) != 2 or points.shape[1] != 3:
        raise ValueError(f"cloud_to_mesh_distance: a PointCloud or points [n,3], got {tuple(getattr(points, 'shape', ()))}")
    return scene.compute_distance(points, max_distance)


def evaluate_mesh_to_mesh(est_mesh, gt_mesh, f_score_threshold=0.1, number_of_points=1_000_000, seed=0, device=None):
    """Accuracy, completion and F-score of a mesh against the mesh it should be, with the exact point-to-surface distance on both
    sides: number_of_points uniform samples of each mesh (TriangleMesh.sample_points_uniformly's rule and seed), each sample's
    distance to the OTHER mesh's surface.  The ground truth is neither sampled into a cloud to search in nor down-sampled, so no
    figure carries a sampling density or a voxel size.  est_mesh, gt_mesh: TriangleMesh, .ply path or RaycastingScene.
    -> {"accuracy": the mean distance of the estimate's samples to the ground truth, "completion": the ground truth's samples to the
    estimate, "chamfer": their sum, "precision" / "recall": the share of each side's samples within f_score_threshold, "f_score":
    2 p r / (p + r), 0 when both are 0, "n_est", "n_gt": the samples drawn}.  A side without area has no samples: its mean is NaN and
    its share 0.  The sums run in fp64 on the device (torch) and are read in one host read, after the sampler's own one per mesh."""
    import torch
    from .. import ops
    from .raycast import RaycastingScene
    threshold, n = float(f_score_threshold), int(number_of_points)
    if not threshold >= 0:
        raise ValueError(f"evaluate_mesh_to_mesh: f_score_threshold must be >= 0, got {f_score_threshold!r}")
    if n <= 0:
        raise ValueError(f"evaluate_mesh_to_mesh: number_of_points must be > 0, got {number_of_points!r}")
    scenes = []
    for mesh in (est_mesh, gt_mesh):
        if isinstance(mesh, RaycastingScene):
            scenes.append(mesh)
            continue
        if isinstance(mesh, (str, os.PathLike)):
            mesh = TriangleMesh.read_ply(mesh)
        if not (hasattr(mesh, "vertices") and hasattr(mesh, "triangles")):
            raise ValueError(f"evaluate_mesh_to_mesh: a TriangleMesh, a .ply path or a RaycastingScene, got {type(mesh).__name__}")
        scenes.append(RaycastingScene(mesh, device=device))
    est, gt = scenes
    if est.device != gt.device:
        raise ValueError(f"evaluate_mesh_to_mesh: the meshes live on {est.device} and {gt.device}")
    sums, counts = [], []
    for own, other in ((est, gt), (gt, est)):
        samples = ops.mesh_sample_points(own.vertices, own.triangles, n, seed)
        d = other.compute_distance(samples)
        sums += [d.sum(), (d <= threshold).sum().double()]
        counts.append(d.shape[0])
    out = torch.stack(sums).cpu().tolist()
    n_est, n_gt = counts
    accuracy = out[0] / n_est if n_est else float("nan")
    completion = out[2] / n_gt if n_gt else float("nan")
    precision = out[1] / n_est if n_est else 0.0
    recall = out[3] / n_gt if n_gt else 0.0
    f_score = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return {"accuracy": accuracy, "completion": completion, "chamfer": accuracy + completion, "precision": precision, "recall": recall,
            "f_score": f_score, "n_est": n_est, "n_gt": n_gt}


def mesh_depth_l1(est_scene, gt_scene, poses, directions, ray_range):
    """The "Depth L1" of the mesh-based SLAM literature: both meshes (RaycastingScenes, analysis/raycast.py) are seen from the same
    poses along the same rays, and the depths are compared.  poses: 4x4 sensor-to-world transforms (Poses, tensors or arrays);
    directions [3,n] in the sensor frame (a scan's layout; depth is t times the direction's length); ray_range = (min, max) metres.
    A ray returns when it hits with min <= depth <= max.  -> {"depth_l1": the mean |depth_est - depth_gt| over the rays both meshes
    return (NaN when there is none), "n_rays", "n_valid", "est_miss_ratio", "gt_miss_ratio": the share of all rays each mesh does not
    return}.  The sum runs in fp64 on the device (torch); one host read."""
    import torch
    lo, hi = (float(x) for x in ray_range)
    if not (lo >= 0 and hi > lo):
        raise ValueError(f"mesh_depth_l1: ray_range must be 0 <= min < max, got {ray_range!r}")
    d = torch.as_tensor(directions)
    if d.dim() != 2 or d.shape[0] != 3:
        raise ValueError(f"mesh_depth_l1: directions [3,n], got {tuple(d.shape)}")
    if len(poses) == 0:
        raise ValueError("mesh_depth_l1: at least one pose is needed")
    if est_scene.device != gt_scene.device:
        raise ValueError(f"mesh_depth_l1: the scenes live on {est_scene.device} and {gt_scene.device}")
    dev = gt_scene.device
    d = d.to(device=dev, dtype=torch.float64).T
    rays = []
    for pose in poses:
        T = pose.get_transformation_matrix() if hasattr(pose, "get_transformation_matrix") else torch.as_tensor(pose)
        T = T.detach().to(device=dev, dtype=torch.float64)
        if tuple(T.shape) != (4, 4):
            raise ValueError(f"mesh_depth_l1: a pose must be a 4x4 transform, got {tuple(T.shape)}")
        world = (d[:, 0:1] * T[:3, 0] + d[:, 1:2] * T[:3, 1]) + d[:, 2:3] * T[:3, 2]
        rays.append(torch.cat([T[:3, 3].expand_as(world), world], dim=1))
    rays = torch.cat(rays).contiguous()
    length = torch.linalg.norm(rays[:, 3:], dim=1)
    depth = [scene.cast_rays(rays)["t_hit"] * length for scene in (est_scene, gt_scene)]
    back = [(x >= lo) & (x <= hi) for x in depth]
    both = back[0] & back[1]
    diff = torch.where(both, (depth[0] - depth[1]).abs(), torch.zeros_like(length))
    n = rays.shape[0]
    out = torch.stack([diff.sum(), both.sum().double(), back[0].sum().double(), back[1].sum().double()]).cpu()
    n_valid = int(out[1])
    return {"depth_l1": float(out[0]) / n_valid if n_valid else float("nan"), "n_rays": n, "n_valid": n_valid,
            "est_miss_ratio": (1.0 - float(out[2]) / n) if n else 0.0, "gt_miss_ratio": (1.0 - float(out[3]) / n) if n else 0.0}
