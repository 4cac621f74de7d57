"""Taking a point cloud apart on the device: radius counts, DBSCAN clusters and RANSAC planes (open3d's remove_radius_outlier,
cluster_dbscan and segment_plane; include/loner_hip.h, "segmentation").  The wrappers of the three entry points live here, beside
analysis.registration's (radius_count and dbscan take an ops.NNGrid, plane_ransac takes points); PointCloud's methods call them, and
cluster_dbscan / segment_plane offer those methods as free functions.  segment_planes peels one plane after another off a cloud.
ValueError: an argument the caller got wrong, refused before a launch."""
import numpy as np
import torch

from .. import hip
from ..hip import _ptr, _stream, check, load
from ..ops._common import _U64, _f64_points, _positive, _scratch


def dbscan_args(what, eps, min_points):
    """(eps as a float, min_points as an int), or ValueError"""
    e = _positive(eps, what, "eps")
    if int(min_points) != min_points or int(min_points) < 1 or int(min_points) > 2 ** 31 - 1:
        raise ValueError(f"{what}: min_points must be an integer >= 1, got {min_points!r}")
    return e, int(min_points)


def plane_args(what, distance_threshold, num_iterations):
    """(distance_threshold as a float, num_iterations as an int), or ValueError"""
    t = _positive(distance_threshold, what, "distance_threshold")
    if int(num_iterations) != num_iterations or not 1 <= int(num_iterations) <= hip.RANSAC_MAX_HYPOTHESES:
        raise ValueError(f"{what}: num_iterations must be in [1, {hip.RANSAC_MAX_HYPOTHESES}], got {num_iterations!r}")
    return t, int(num_iterations)


def radius_count(grid, radius, stats=None):
    """For every target of the ops.NNGrid the number of targets within `radius` of it, itself included: d2 < radius^2, strict
    (include/loner_hip.h: lnr_cloud_radius_count) -> int32 [n] in the targets' order; stats (a dict, optional) receives {"shells":
    shells walked}.  The counts do not depend on the grid's cell edge.  One device -> host read."""
    r = _positive(radius, "radius_count", "radius")
    dev = grid.buf.device
    counts = torch.empty(grid.n, device=dev, dtype=torch.int32)
    counters = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_cloud_radius_count(_ptr(grid.buf), grid.n, r, _ptr(counts), _ptr(counters), _stream()), "lnr_cloud_radius_count")
    c = counters.cpu()
    if int(c[1]):
        raise RuntimeError("radius_count: the grid is unusable (non-finite targets)")
    if stats is not None:
        stats.update(shells=int(c[2]))
    return counts


def dbscan(grid, eps, min_points):
    """open3d's cluster_dbscan over the targets of an ops.NNGrid (include/loner_hip.h: lnr_cloud_dbscan) -> (labels int32 [n] in the
    targets' order, -1 for noise; info int64 [8] on the device: {status, clusters, cores, border points, noise points}).  No host
    read."""
    e, k = dbscan_args("dbscan", eps, min_points)
    dev = grid.buf.device
    labels = torch.empty(grid.n, device=dev, dtype=torch.int32)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    ws, need = _scratch(load().lnr_cloud_dbscan_workspace(grid.n), dev, f"dbscan: {grid.n} points, the limit is 2^31 - 4096")
    check(load().lnr_cloud_dbscan(_ptr(grid.buf), grid.n, e, k, _ptr(labels), _ptr(ws), need, _ptr(info), _stream()), "lnr_cloud_dbscan")
    return labels, info


def plane_ransac(points, distance_threshold, num_iterations=1000, seed=0, refine=True):
    """open3d's segment_plane with ransac_n = 3 and a fixed number of hypotheses (include/loner_hip.h: lnr_cloud_segment_plane).
    points [n,3] on the device -> dict with plane (numpy fp64 [4]: a, b, c, d of the returned model), hypothesis_plane (the best
    hypothesis's own model), inlier (uint8 [n] on the device: the best hypothesis's mask), status, best_hypothesis, n_inliers,
    survivors, rejected_repeated, rejected_degenerate, nonfinite, n.  A status bit (1: fewer than 3 points, 2: no hypothesis survived)
    is reported, not raised: the plane is then zeros and the mask empty.  One device -> host read."""
    t, H = plane_args("segment_plane", distance_threshold, num_iterations)
    pts = _f64_points(points, "segment_plane")
    n, dev = pts.shape[0], pts.device
    lib = load()
    ws, need = _scratch(lib.lnr_plane_workspace(n, H), dev, f"segment_plane: {n} points, the limit is 2^31 - 4096")
    plane = torch.empty(8, device=dev, dtype=torch.float64)
    inlier = torch.empty(n, device=dev, dtype=torch.uint8)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    check(lib.lnr_cloud_segment_plane(_ptr(pts), n, t, H, int(seed) & _U64, 1 if refine else 0, _ptr(plane), _ptr(inlier), _ptr(ws), need,
                                      _ptr(info), _stream()), "lnr_cloud_segment_plane")
    p = plane.cpu().numpy()
    i = [int(x) for x in info.cpu()]
    return {"plane": p[:4].copy(), "hypothesis_plane": p[4:].copy(), "inlier": inlier, "status": i[0], "best_hypothesis": i[1],
            "n_inliers": i[2], "survivors": i[3], "rejected_repeated": i[4], "rejected_degenerate": i[5], "nonfinite": i[6], "n": i[7]}


def cluster_dbscan(cloud, eps, min_points, info=None):
    """PointCloud.cluster_dbscan as a free function -> labels int32 [n] on the device, -1 for noise."""
    return cloud.cluster_dbscan(eps, min_points, info=info)


def segment_plane(cloud, distance_threshold, num_iterations=1000, seed=0, refine=True, info=None):
    """PointCloud.segment_plane as a free function -> (plane_model numpy fp64 [4], inlier indices int64 on the device, ascending)."""
    return cloud.segment_plane(distance_threshold, num_iterations, seed, refine, info=info)


def segment_planes(cloud, distance_threshold, max_planes, min_inliers, num_iterations=1000, seed=0, refine=True):
    """The planes of a cloud, largest first as RANSAC finds them: segment a plane, remove its inliers, repeat on the rest.  It stops
    after max_planes planes, or at the first plane with fewer than min_inliers inliers (which is not kept), or when fewer than 3
    points are left.  Every round uses the same seed on the points that are left, in their input order.
    -> (models numpy fp64 [k,4], labels int32 [n] on the device: the plane of every input point, -1 for points on no plane)."""
    if int(max_planes) != max_planes or max_planes < 0:
        raise ValueError(f"segment_planes: max_planes must be an integer >= 0, got {max_planes!r}")
    if int(min_inliers) != min_inliers or min_inliers < 0:
        raise ValueError(f"segment_planes: min_inliers must be an integer >= 0, got {min_inliers!r}")
    plane_args("segment_planes", distance_threshold, num_iterations)
    n = len(cloud)
    labels = torch.full((n,), -1, dtype=torch.int32, device=cloud.points.device)
    left = torch.arange(n, dtype=torch.int64, device=cloud.points.device)       # input index of every point still on no plane
    models = []
    while len(models) < int(max_planes) and left.shape[0] >= 3:
        out = plane_ransac(cloud.points[left], distance_threshold, num_iterations, seed, refine)
        if out["status"] or out["n_inliers"] < max(int(min_inliers), 1):
            break
        on = out["inlier"].bool()
        labels[left[on]] = len(models)
        models.append(out["plane"])
        left = left[~on]
    return np.array(models, dtype=np.float64).reshape(-1, 4), labels
