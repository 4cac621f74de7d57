"""Point clouds: scan points, voxel down-sampling, transforms, the nearest-neighbour grid, ICP, trajectories.
Offline tools: points of any float dtype are widened to fp64, and most calls read status and counts back once (their docstrings say so).
ValueError: an argument the caller got wrong, refused before a launch.  RuntimeError: what only the data shows (non-finite points, a
size over the library's limit, a status bit)."""
import ctypes as C
import math

import numpy as np
import torch

from .. import hip
from ..hip import _ptr, _stream, check, load, require_device
from ._common import _f32c, _f64_points, _positive, _raise_status, _scratch

_CLOUD_STATUS = {1: "non-finite input coordinates", 2: "voxel_size is too small", 4: "the voxel key needs more than 64 bits"}
_ICP_STATUS = {1: "non-finite source points", 2: "the target grid is unusable (non-finite targets)", 4: "non-finite target normals",
               8: "the update is not finite (a degenerate system)"}


def _cloud_workspace(n, device):
    """lnr_cloud_workspace(n) bytes on `device`: one buffer per device, grown on demand (calls on one stream reuse it in order)."""
    return _scratch(load().lnr_cloud_workspace(int(n)), device, f"point clouds: {n} points, the limit per call is 2^31 - 4096",
                    held="cloud")


def _tools_workspace(n, device):
    """lnr_cloud_tools_workspace(n) bytes: a buffer per call (the caching allocator's, so calls on different streams never share one)"""
    return _scratch(load().lnr_cloud_tools_workspace(int(n)), device, f"{n} points, the limit is 2^31 - 4096")


def _cloud_status(what, info, noun="points"):
    status = int(info[0])
    if status & 1:
        raise RuntimeError(f"{what}: {int(info[2])} {noun} with non-finite coordinates")
    _raise_status(what, status, _CLOUD_STATUS)


def lidar_scan_points(depth, variance, ray_index, directions, scale, var_max, depth_max):
    """Scan points of one rendered pose (include/loner_hip.h: lnr_lidar_scan_points) -> (points [m,3] fp64, count int32 [1]); the
    first count rows hold the kept rays' points in ray order, and the count stays on the device."""
    require_device(depth, variance, ray_index, directions)
    depth, variance, directions = _f32c(depth).reshape(-1), _f32c(variance).reshape(-1), _f32c(directions)
    ray_index = ray_index.to(torch.int64).contiguous()
    assert directions.dim() == 2 and directions.shape[0] == 3, "lidar_scan_points: directions [3, N]"
    m = depth.shape[0]
    assert variance.shape[0] == m and ray_index.shape[0] == m
    dev = depth.device
    ws, need = _cloud_workspace(m, dev)
    points = torch.empty(m, 3, device=dev, dtype=torch.float64)
    count = torch.empty(1, device=dev, dtype=torch.int32)
    check(load().lnr_lidar_scan_points(_ptr(depth), _ptr(variance), _ptr(ray_index), m, _ptr(directions), directions.shape[1], float(scale), float(var_max),
                                       float(depth_max), _ptr(ws), need, _ptr(points), _ptr(count), _stream()), "lnr_lidar_scan_points")
    return points, count


def voxel_down_sample(points, voxel_size, count=None):
    """open3d's VoxelDownSample with a defined order (include/loner_hip.h: lnr_voxel_down_sample): points [n,3] (fp64), count
    (optional int32 [1] on the device) the live rows -> [k,3] fp64, one point per occupied voxel in ascending (i_x, i_y, i_z)
    order.  One device -> host read."""
    v = _positive(voxel_size, "voxel_down_sample", "voxel_size")
    pts = _f64_points(points, "voxel_down_sample")
    require_device(count)
    n, dev = pts.shape[0], pts.device
    ws, need = _cloud_workspace(n, dev)
    out = torch.empty(n, 3, device=dev, dtype=torch.float64)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    check(load().lnr_voxel_down_sample(_ptr(pts), n, _ptr(count), v, _ptr(ws), need, _ptr(out), _ptr(info), _stream()), "lnr_voxel_down_sample")
    info = info.cpu()
    _cloud_status("voxel_down_sample", info)
    return out[:int(info[1])]


def affine_f64(T, what, finite=False):
    """T (a tensor or an array of any float dtype) as a numpy fp64 4x4 whose bottom row is [0, 0, 0, 1] (and finite, when asked);
    ValueError(f"{what}, got ...") otherwise."""
    T = np.asarray(T.detach().cpu().numpy() if torch.is_tensor(T) else T, dtype=np.float64)
    if T.shape != (4, 4) or not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) or (finite and not np.isfinite(T).all()):
        raise ValueError(f"{what}, got {T.tolist()}")
    return T


def cloud_transform(points, T, out=None):
    """out[i] = T[:3,:3] p_i + T[:3,3] in fp64 without fma (include/loner_hip.h: lnr_cloud_append_transformed).  T: a 4x4 affine
    (tensor or array, any float dtype, widened to fp64); out (optional, [n,3] fp64, may be `points` itself or a slice of a larger
    cloud) receives the result."""
    T = affine_f64(T, "transform: T must be a 4x4 affine matrix with bottom row [0, 0, 0, 1]")
    pts = _f64_points(points, "transform")
    out = torch.empty_like(pts) if out is None else out
    assert out.dtype == torch.float64 and out.is_contiguous() and out.shape == pts.shape
    t12 = (C.c_double * 12)(*[float(x) for x in T[:3].reshape(-1)])
    check(load().lnr_cloud_append_transformed(_ptr(pts), pts.shape[0], t12, _ptr(out), _stream()), "lnr_cloud_append_transformed")
    return out


def _grid_query(device, call, what, bad, stats):
    """The int64 [4] counters of a grid query: allocated on `device`, filled by call(pointer), read once.  Word 1 counts the non-finite
    inputs: RuntimeError(bad.format(that count)) when set.  stats (a dict or None) receives {"fallback": word 0, "shells": word 2}."""
    counters = torch.empty(4, device=device, dtype=torch.int64)
    check(call(_ptr(counters)), what)
    c = counters.cpu()
    if int(c[1]):
        raise RuntimeError(bad.format(int(c[1])))
    if stats is not None:
        stats.update(fallback=int(c[0]), shells=int(c[2]))


class NNGrid:
    """The nearest-neighbour grid over a target cloud (include/loner_hip.h: lnr_nn_grid_build), reusable for any number of query
    batches.  cell_edge: None for the default rule.  .edge, .n_cells, .dims: what the build chose (one host read)."""

    def __init__(self, targets, cell_edge=None):
        pts = _f64_points(targets, "NNGrid")
        self.n = pts.shape[0]
        dev = pts.device
        lib = load()
        self.buf, gbytes = _scratch(lib.lnr_nn_grid_bytes(self.n), dev, f"NNGrid: {self.n} targets, the limit is 2^31 - 4096")
        ws, need = _cloud_workspace(self.n, dev)
        info = torch.empty(8, device=dev, dtype=torch.int64)
        edge = 0.0 if cell_edge is None else float(cell_edge)
        if not math.isfinite(edge) or edge < 0:
            raise ValueError(f"NNGrid: cell_edge must be finite and > 0, got {cell_edge!r}")
        check(lib.lnr_nn_grid_build(_ptr(pts), self.n, edge, _ptr(ws), need, _ptr(self.buf), gbytes, _ptr(info), _stream()), "lnr_nn_grid_build")
        info = info.cpu()
        _cloud_status("NNGrid", info)
        self.n_cells = int(info[1])
        self.edge = float(info[4:5].view(torch.float64)[0])
        self.dims = tuple(int(x) for x in info[5:8])

    def distance(self, queries, want_sq=False, stats=None):
        """-> distance [m] fp64 to the nearest target (and d2 when want_sq); stats (a dict, optional) receives the counters
        {"fallback": queries that took the exact pass, "shells": shells visited}.  One device -> host read."""
        q = _f64_points(queries, "NNGrid.distance")
        m, dev = q.shape[0], q.device
        dist = torch.empty(m, device=dev, dtype=torch.float64)
        d2 = torch.empty(m, device=dev, dtype=torch.float64) if want_sq else None
        ws, need = _cloud_workspace(m, dev)
        _grid_query(dev, lambda counters: load().lnr_nn_distance(_ptr(self.buf), self.n, _ptr(q), m, _ptr(dist), _ptr(d2), _ptr(ws), need,
                                                                 counters, _stream()),
                    "lnr_nn_distance", "compute_point_cloud_distance: {} queries with non-finite coordinates", stats)
        return (dist, d2) if want_sq else dist

    def normals(self, knn=30, want_covariances=False, stats=None):
        """open3d's EstimateNormals(KDTreeSearchParamKNN(knn)) over the grid's own targets (include/loner_hip.h: lnr_cloud_normals)
        -> normals [n,3] fp64 in the targets' order, and covariances [n,3,3] when asked; stats (a dict, optional) receives
        {"fallback", "shells"}.  One device -> host read."""
        knn = int(knn)
        if not 1 <= knn <= hip.KNN_MAX:
            raise ValueError(f"normals: knn must be in [1, {hip.KNN_MAX}], got {knn}")
        dev = self.buf.device
        normals = torch.empty(self.n, 3, device=dev, dtype=torch.float64)
        cov = torch.empty(self.n, 3, 3, device=dev, dtype=torch.float64) if want_covariances else None
        ws, need = _cloud_workspace(self.n, dev)
        _grid_query(dev, lambda counters: load().lnr_cloud_normals(_ptr(self.buf), self.n, knn, _ptr(normals), _ptr(cov), _ptr(ws), need,
                                                                   counters, _stream()),
                    "lnr_cloud_normals", "normals: the grid is unusable (non-finite targets)", stats)
        return (normals, cov) if want_covariances else normals

    def knn_mean_distance(self, nb_neighbors=20, stats=None):
        """The mean distance of every target to its nb_neighbors nearest targets, itself included (include/loner_hip.h:
        lnr_cloud_knn_mean_distance) -> fp64 [n] in the targets' order; stats as normals'.  One device -> host read."""
        k = int(nb_neighbors)
        if not 1 <= k <= hip.KNN_MAX:
            raise ValueError(f"knn_mean_distance: nb_neighbors must be in [1, {hip.KNN_MAX}], got {nb_neighbors}")
        dev = self.buf.device
        avg = torch.empty(self.n, device=dev, dtype=torch.float64)
        ws, need = _tools_workspace(self.n, dev)
        _grid_query(dev, lambda counters: load().lnr_cloud_knn_mean_distance(_ptr(self.buf), self.n, k, _ptr(avg), _ptr(ws), need,
                                                                             counters, _stream()),
                    "lnr_cloud_knn_mean_distance", "knn_mean_distance: the grid is unusable (non-finite targets)", stats)
        return avg

    def outlier_threshold(self, mean_distance, std_ratio):
        """open3d's statistical-outlier threshold over knn_mean_distance's values (include/loner_hip.h: lnr_cloud_outlier_threshold)
        -> fp64 [4] on the device: {mean, std, threshold, valid}.  No host read."""
        avg = mean_distance
        require_device(avg)
        if avg.dtype != torch.float64 or avg.shape != (self.n,) or not avg.is_contiguous():
            raise ValueError(f"outlier_threshold: mean_distance fp64 [{self.n}], got {tuple(avg.shape)} {avg.dtype}")
        ratio = float(std_ratio)
        if not math.isfinite(ratio):
            raise ValueError(f"outlier_threshold: std_ratio must be finite, got {std_ratio!r}")
        ws, need = _tools_workspace(self.n, avg.device)
        res = torch.empty(4, device=avg.device, dtype=torch.float64)
        check(load().lnr_cloud_outlier_threshold(_ptr(self.buf), _ptr(avg), self.n, ratio, _ptr(ws), need, _ptr(res),
                                                 _stream()), "lnr_cloud_outlier_threshold")
        return res

    def correspondences(self, queries, max_distance):
        """-> (index int32 [m]: the nearest target with d2 < max_distance^2, lower index on ties, -1 for none; d2 [m] fp64, +inf for
        none) (include/loner_hip.h: lnr_icp_correspondences)."""
        q = _f64_points(queries, "NNGrid.correspondences")
        r = _positive(max_distance, "correspondences", "max_distance")
        m = q.shape[0]
        index = torch.empty(m, device=q.device, dtype=torch.int32)
        d2 = torch.empty(m, device=q.device, dtype=torch.float64)
        _grid_query(q.device, lambda counters: load().lnr_icp_correspondences(_ptr(self.buf), self.n, _ptr(q), m, r, _ptr(index), _ptr(d2),
                                                                             counters, _stream()),
                    "lnr_icp_correspondences", "correspondences: {} queries with non-finite coordinates", None)
        return index, d2


def icp_point_to_plane(grid, target_normals, source, max_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6,
                       max_iteration=30):
    """open3d's registration_icp with TransformationEstimationPointToPlane (include/loner_hip.h: lnr_icp_point_to_plane).  grid: an
    NNGrid over the targets; target_normals [n,3] in the targets' order; source [m,3]; init 4x4 (default identity).  -> dict with
    transformation (numpy fp64 4x4), fitness, inlier_rmse, n_correspondences, iterations, and the last solved system (JTJ 6x6, JTr,
    sum_d2, x).  Every round is enqueued at once; one device -> host read.  Raises RuntimeError on a status bit."""
    src = _f64_points(source, "icp_point_to_plane")
    nrm = _f64_points(target_normals, "icp_point_to_plane")
    if nrm.shape[0] != grid.n:
        raise ValueError(f"icp_point_to_plane: {nrm.shape[0]} normals for {grid.n} targets")
    r = _positive(max_distance, "icp_point_to_plane", "max_correspondence_distance")
    T0 = affine_f64(np.eye(4) if init is None else init, "icp_point_to_plane: init must be a finite 4x4 affine matrix", finite=True)
    dev = src.device
    lib = load()
    ws, need = _scratch(lib.lnr_icp_workspace(src.shape[0]), dev)
    result = torch.empty(hip.ICP_RESULT, device=dev, dtype=torch.float64)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    t16 = (C.c_double * 16)(*[float(x) for x in T0.reshape(-1)])
    check(lib.lnr_icp_point_to_plane(_ptr(grid.buf), grid.n, _ptr(nrm), _ptr(src), src.shape[0], r, t16, float(relative_fitness), float(relative_rmse),
                                     int(max_iteration), _ptr(ws), need, _ptr(result), _ptr(info), _stream()), "lnr_icp_point_to_plane")
    res = result.cpu().numpy()
    info = [int(x) for x in info.cpu()]
    _raise_status("icp_point_to_plane", info[0], _ICP_STATUS)
    JTJ = np.zeros((6, 6))
    JTJ[np.triu_indices(6)] = res[18:39]
    JTJ = JTJ + np.triu(JTJ, 1).T
    return {"transformation": res[:16].reshape(4, 4).copy(), "fitness": float(res[16]), "inlier_rmse": float(res[17]),
            "n_correspondences": info[1], "iterations": info[2], "JTJ": JTJ, "JTr": res[39:45].copy(), "sum_d2": float(res[45]),
            "x": res[46:52].copy(), "system_correspondences": info[5]}


class Trajectory:
    """A ground-truth trajectory on the device, in the form lnr_cloud_trajectory_transform takes: times [K] (strictly increasing),
    positions [K,3], rotations [K,3,3] and the rotation vectors log(R_k^T R_k+1) [K-1,3], all fp64 host arrays here."""

    def __init__(self, times, positions, rotations, rotvecs, device):
        t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        K = t.shape[0]
        if K < 2:
            raise ValueError(f"Trajectory: at least 2 poses are needed, got {K}")
        P = np.ascontiguousarray(positions, dtype=np.float64)
        R = np.ascontiguousarray(rotations, dtype=np.float64)
        W = np.ascontiguousarray(rotvecs, dtype=np.float64)
        if P.shape != (K, 3) or R.shape != (K, 3, 3) or W.shape != (K - 1, 3):
            raise ValueError(f"Trajectory: positions [{K},3], rotations [{K},3,3] and rotvecs [{K - 1},3], got {P.shape}, {R.shape}, {W.shape}")
        if not (np.isfinite(t).all() and np.isfinite(P).all() and np.isfinite(R).all() and np.isfinite(W).all()):
            raise ValueError("Trajectory: a pose or a pose time is not finite")
        if not (np.diff(t) > 0).all():
            raise ValueError("Trajectory: the pose times must be strictly increasing")
        self.n_poses = K
        self.t0, self.t1 = float(t[0]), float(t[-1])
        self.times, self.positions, self.rotations, self.rotvecs = (torch.from_numpy(a).to(device) for a in (t, P, R, W))


def trajectory_transform(points, timestamps, trajectory, min_range):
    """Every point moved by the trajectory's pose at its own time (include/loner_hip.h: lnr_cloud_trajectory_transform): points [n,3]
    (sensor frame), timestamps [n] (absolute, fp64), trajectory a Trajectory on the same device -> (out [n,3] fp64 whose first `kept`
    rows hold the kept points in input order, info int64 [8] on the device: {status, kept, below range, outside, non-finite})."""
    pts = _f64_points(points, "trajectory_transform")
    require_device(timestamps)
    n = pts.shape[0]
    if timestamps.shape != (n,):
        raise ValueError(f"trajectory_transform: timestamps [{n}], got {tuple(timestamps.shape)}")
    stamps = timestamps.to(torch.float64).contiguous()
    r = float(min_range)
    if math.isnan(r):
        raise ValueError("trajectory_transform: min_range is NaN")
    dev = pts.device
    ws, need = _tools_workspace(n, dev)
    out = torch.empty(n, 3, device=dev, dtype=torch.float64)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    tr = trajectory
    check(load().lnr_cloud_trajectory_transform(_ptr(pts), _ptr(stamps), n, _ptr(tr.times), _ptr(tr.positions), _ptr(tr.rotations), _ptr(tr.rotvecs),
                                                tr.n_poses, r, _ptr(ws), need, _ptr(out), _ptr(info), _stream()), "lnr_cloud_trajectory_transform")
    return out, info
