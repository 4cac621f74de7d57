"""Generalized (plane-to-plane) ICP and robust loss kernels on the device: open3d's registration_generalized_icp and its RobustKernel
family (include/loner_hip.h, "robust kernels and generalized ICP"), beside lidar_map.registration_icp, which stays the plain
point-to-plane estimator.

  RobustKernel(kind, k)             "l2" | "huber" | "cauchy" | "tukey" with the scale k
  plane_covariances(normals, eps)   the covariance of a point on a plane, from its unit normal
  registration_generalized_icp      Segal et al.'s estimator on two PointClouds -> RegistrationResult
  registration_icp_robust           point-to-plane ICP with a RobustKernel on the scalar residual -> RegistrationResult
  icp_generalized, icp_point_to_plane_robust   the entry points on tensors, with the last solved system in the result (as
                                    ops.icp_point_to_plane)

Global registration, for two clouds without a starting pose (include/loner_hip.h, "global registration"):

  orient_normals, fpfh, feature_nearest, ransac_correspondence, fpfh_bin_edges   the entry points on tensors
  correspondences_from_features     the nearest target feature of every source feature, exact -> int32 [m,2]
  registration_ransac_based_on_correspondence, registration_ransac_based_on_feature_matching   open3d's, with a fixed number of
                                    hypotheses and triangle-frame poses -> RegistrationResult
  global_registration               down-sample, normals, orientation, FPFH, RANSAC, two rounds of point-to-plane ICP

The information matrix of a registered pair, for the pose graph (analysis/pose_graph.py; include/loner_hip.h, "pose graph"):

  icp_information, get_information_matrix_from_point_clouds     open3d's GetInformationMatrixFromPointClouds -> 6x6 fp64

Limits of the global path, by intent: FPFH takes at most 32 neighbours (max_nn <= 32) and the feature search at most 64 dimensions
(dim <= 64); the search is brute force and exact; the number of hypotheses is fixed (no confidence-based early stop), so the answer
depends on the arguments and the seed only; a hypothesis' pose comes from the two triangle frames, not from a Kabsch fit; FPFH depends
on the sign of the normals, and orienting them consistently is the caller's responsibility (global_registration's default, towards each
cloud's own centroid, is rigid-equivariant but only sound for clouds seen from one side); the tracker does not fall back on it.

Differences from open3d, by intent: the normal equations are J^T W J and J^T W d without the matrix square root of W = M^-1 (the same
least-squares problem with L2), and a robust weight is taken once per correspondence on the Mahalanobis residual sqrt(d^T W d), not
once per whitened row, so it does not depend on the frame.  A cloud's covariances are taken in open3d's order of preference (its
covariances, else the plane rule on its normals, else on normals estimated for the call), and neither cloud is filled in place.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import hip, ops
from ..hip import _ptr, _stream, check, load, require_device
from ..ops._common import _U64, _f64_points, _positive, _raise_status, _scratch
from .lidar_map import RegistrationResult

_STATUS = {1: "non-finite source points", 2: "the target grid is unusable (non-finite targets)", 4: "non-finite target normals",
           8: "the update is not finite (a degenerate system)", 16: "a combined covariance is singular or not finite"}
_ENTRY = {"plane": "lnr_icp_point_to_plane", "plane_robust": "lnr_icp_point_to_plane_robust", "generalized": "lnr_icp_generalized"}


class RobustKernel:
    """open3d's RobustKernel: kind "l2" (w = 1), "huber" (k / max(m, k)), "cauchy" (1 / (1 + (m/k)^2)) or "tukey"
    ((1 - (m/k)^2)^2 up to k, then 0), with the scale k (finite and > 0; not read by "l2")."""

    def __init__(self, kind="l2", k=1.0):
        kind = str(kind).lower()
        if kind not in hip.ROBUST_KERNELS:
            raise ValueError(f"RobustKernel: kind must be one of {sorted(hip.ROBUST_KERNELS)}, got {kind!r}")
        k = float(k)
        if kind != "l2" and not (math.isfinite(k) and k > 0):
            raise ValueError(f"RobustKernel: k must be finite and > 0, got {k!r}")
        self.kind = kind
        self.k = k

    @property
    def code(self):
        return hip.ROBUST_KERNELS[self.kind]

    def __repr__(self):
        return f"RobustKernel({self.kind!r}, {self.k!r})"


def _kernel(kernel):
    if kernel is None:
        return RobustKernel()
    if not isinstance(kernel, RobustKernel):
        raise ValueError(f"kernel must be a RobustKernel or None, got {kernel!r}")
    return kernel


def plane_covariances(normals, epsilon=1e-3):
    """[n,3,3] fp64: C = I - (1 - epsilon) n n^T per unit normal (include/loner_hip.h: lnr_cloud_plane_covariances); no host read"""
    nrm = _f64_points(normals, "plane_covariances")
    eps = _positive(epsilon, "plane_covariances", "epsilon")
    cov = torch.empty(nrm.shape[0], 3, 3, device=nrm.device, dtype=torch.float64)
    check(load().lnr_cloud_plane_covariances(_ptr(nrm), nrm.shape[0], eps, _ptr(cov), _stream()), "lnr_cloud_plane_covariances")
    return cov


def cloud_covariances(cloud, epsilon=1e-3, knn=20):
    """The covariances generalized ICP takes of a PointCloud, which is left as it is: its own, else the plane rule on its normals, else
    on normals estimated for this call (estimate_normals(knn))."""
    if cloud.covariances is not None:
        return cloud.covariances
    if len(cloud) == 0:
        return torch.zeros(0, 3, 3, dtype=torch.float64, device=cloud.points.device)
    normals = cloud.normals if cloud.normals is not None else ops.NNGrid(cloud.points).normals(knn)
    return plane_covariances(normals, epsilon)


def _covariances(t, n, what, name):
    hip.require_device(t)
    if t.dim() != 3 or tuple(t.shape) != (n, 3, 3):
        raise ValueError(f"{what}: {name} [{n},3,3], got {tuple(t.shape)}")
    return t.to(torch.float64).contiguous()


def _run(entry, grid, attr, src, src_cov, r, init, relative_fitness, relative_rmse, max_iteration, kernel):
    """One call of an ICP entry point -> (result fp64 [ICP_RESULT], info int64 [8]) as numpy arrays; one device -> host read"""
    what = _ENTRY[entry]
    T0 = ops.affine_f64(np.eye(4) if init is None else init, f"{what[4:]}: init must be a finite 4x4 affine matrix", finite=True)
    dev = src.device
    lib = load()
    ws, need = _scratch(lib.lnr_icp_workspace(src.shape[0]), dev)
    result = torch.empty(hip.ICP_RESULT, device=dev, dtype=torch.float64)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    t16 = (C.c_double * 16)(*[float(x) for x in T0.reshape(-1)])
    head = (_ptr(grid.buf), grid.n, _ptr(attr), _ptr(src)) + ((_ptr(src_cov),) if entry == "generalized" else ())
    crit = (src.shape[0], r, t16, float(relative_fitness), float(relative_rmse), int(max_iteration))
    robust = () if entry == "plane" else (kernel.code, kernel.k)
    check(getattr(lib, what)(*head, *crit, *robust, _ptr(ws), need, _ptr(result), _ptr(info), _stream()), what)
    return result.cpu().numpy(), info.cpu().numpy()


def _as_dict(what, res, info):
    _raise_status(what, int(info[0]), _STATUS)
    JTJ = np.zeros((6, 6))
    JTJ[np.triu_indices(6)] = res[18:39]
    JTJ = JTJ + np.triu(JTJ, 1).T
    return {"transformation": res[:16].reshape(4, 4).copy(), "fitness": float(res[16]), "inlier_rmse": float(res[17]),
            "n_correspondences": int(info[1]), "iterations": int(info[2]), "JTJ": JTJ, "JTr": res[39:45].copy(), "sum_d2": float(res[45]),
            "x": res[46:52].copy(), "system_correspondences": int(info[5])}


def icp_generalized(grid, target_covariances, source, source_covariances, max_distance, init=None, relative_fitness=1e-6,
                    relative_rmse=1e-6, max_iteration=30, kernel=None):
    """include/loner_hip.h: lnr_icp_generalized.  grid: an ops.NNGrid over the targets; target_covariances [n,3,3] in the targets'
    order; source [m,3] and its covariances [m,3,3] as they are before init.  -> the dict of ops.icp_point_to_plane.  Raises
    RuntimeError on a status bit."""
    src = _f64_points(source, "icp_generalized")
    tc = _covariances(target_covariances, grid.n, "icp_generalized", "target_covariances")
    sc = _covariances(source_covariances, src.shape[0], "icp_generalized", "source_covariances")
    r = _positive(max_distance, "icp_generalized", "max_correspondence_distance")
    return _as_dict("icp_generalized", *_run("generalized", grid, tc, src, sc, r, init, relative_fitness, relative_rmse, max_iteration,
                                             _kernel(kernel)))


def icp_point_to_plane_robust(grid, target_normals, source, max_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6,
                              max_iteration=30, kernel=None):
    """include/loner_hip.h: lnr_icp_point_to_plane_robust; ops.icp_point_to_plane with a RobustKernel on |r|"""
    src = _f64_points(source, "icp_point_to_plane_robust")
    nrm = _f64_points(target_normals, "icp_point_to_plane_robust")
    if nrm.shape[0] != grid.n:
        raise ValueError(f"icp_point_to_plane_robust: {nrm.shape[0]} normals for {grid.n} targets")
    r = _positive(max_distance, "icp_point_to_plane_robust", "max_correspondence_distance")
    return _as_dict("icp_point_to_plane_robust", *_run("plane_robust", grid, nrm, src, None, r, init, relative_fitness, relative_rmse,
                                                       max_iteration, _kernel(kernel)))


def _result(out):
    return RegistrationResult(out["transformation"], out["fitness"], out["inlier_rmse"], out["n_correspondences"], out["iterations"])


def registration_generalized_icp(source, target, max_correspondence_distance, init=np.eye(4), relative_fitness=1e-6, relative_rmse=1e-6,
                                 max_iteration=30, kernel=None, epsilon=1e-3, knn=20):
    """open3d's registration_generalized_icp(source, target, d, init, TransformationEstimationForGeneralizedICP(epsilon, kernel),
    ICPConvergenceCriteria(...)) on the device -> RegistrationResult.  Each cloud's covariances: cloud_covariances (its own, else
    from its normals, else from normals estimated with knn neighbours); neither cloud is changed.  The search grid's cell edge is the
    correspondence distance."""
    r = _positive(max_correspondence_distance, "registration_generalized_icp", "max_correspondence_distance")
    kernel = _kernel(kernel)
    dev = target.points.device
    grid = ops.NNGrid(target.points, r)
    tc = cloud_covariances(target, epsilon, knn)
    sc = cloud_covariances(source, epsilon, knn).to(dev)
    return _result(icp_generalized(grid, tc, source.points.to(dev), sc, r, init, relative_fitness, relative_rmse, max_iteration, kernel))


def registration_icp_robust(source, target, max_correspondence_distance, init=np.eye(4), relative_fitness=1e-6, relative_rmse=1e-6,
                            max_iteration=30, kernel=None):
    """lidar_map.registration_icp with a RobustKernel: open3d's TransformationEstimationPointToPlane(kernel).  With kernel None or
    "l2" the result is registration_icp's, bit for bit."""
    if target.normals is None:
        raise ValueError("registration_icp_robust: point-to-plane ICP needs the target's normals (call target.estimate_normals())")
    r = _positive(max_correspondence_distance, "registration_icp_robust", "max_correspondence_distance")
    grid = ops.NNGrid(target.points, r)
    return _result(icp_point_to_plane_robust(grid, target.normals, source.points.to(target.points.device), r, init, relative_fitness,
                                             relative_rmse, max_iteration, kernel))


# ---------------------------------------------------------------- global registration
# The tensor-level wrappers of the entry points live here, beside icp_generalized, not in loner_amd.ops.
_RANSAC_STATUS = {1: "fewer than 3 correspondences", 2: "no hypothesis survived", 4: "a correspondence index out of range"}


def fpfh_bin_edges():
    """numpy fp64 [10,2]: (cos, sin) of the ten inner edges of the FPFH angle bins (include/loner_hip.h: lnr_fpfh_bin_edges); host only"""
    out = np.zeros(20, dtype=np.float64)
    check(load().lnr_fpfh_bin_edges(out.ctypes.data_as(C.c_void_p)), "lnr_fpfh_bin_edges")
    return out.reshape(10, 2)


def _vec3(v, what, name):
    a = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{what}: {name} must be 3 finite numbers, got {a.tolist()}")
    return (C.c_double * 3)(*[float(x) for x in a])


def orient_normals(normals, points=None, location=None, direction=None, stats=None):
    """Flips normals [n,3] (fp64, contiguous, on the device) in place (include/loner_hip.h: lnr_cloud_orient_normals): towards
    `location` as seen from points [n,3], or to align with `direction`; exactly one of the two.  Non-finite normals are left as they
    are.  stats (a dict, optional) receives {"nonfinite", "flipped"} (one device -> host read, only then).  -> normals"""
    if (location is None) == (direction is None):
        raise ValueError("orient_normals: give exactly one of location and direction")
    require_device(normals)
    if normals.dim() != 2 or normals.shape[1] != 3 or normals.dtype != torch.float64 or not normals.is_contiguous():
        raise ValueError(f"orient_normals: normals fp64 [n,3] contiguous (flipped in place), got {tuple(normals.shape)} {normals.dtype}")
    n = normals.shape[0]
    if location is not None:
        if points is None:
            raise ValueError("orient_normals: a location needs the points")
        pts = _f64_points(points, "orient_normals")
        if pts.shape[0] != n:
            raise ValueError(f"orient_normals: {pts.shape[0]} points for {n} normals")
        mode, ref = hip.ORIENT_LOCATION, _vec3(location, "orient_normals", "location")
    else:
        pts, mode, ref = None, hip.ORIENT_DIRECTION, _vec3(direction, "orient_normals", "direction")
    counters = torch.empty(4, device=normals.device, dtype=torch.int64)
    check(load().lnr_cloud_orient_normals(_ptr(pts), n, _ptr(normals), mode, ref, _ptr(counters), _stream()), "lnr_cloud_orient_normals")
    if stats is not None:
        c = counters.cpu()
        stats.update(nonfinite=int(c[0]), flipped=int(c[1]))
    return normals

def fpfh(grid, normals, radius, max_nn=32, stats=None):
    """open3d's compute_fpfh_feature(KDTreeSearchParamHybrid(radius, max_nn)) over the targets of an ops.NNGrid with their normals
    [n,3] in the targets' order (include/loner_hip.h: lnr_cloud_fpfh) -> features [n,33] fp64, row i = target i; max_nn in [2, 32].
    The sign of a normal matters: orient the normals first.  stats (a dict, optional) receives {"fallback", "shells",
    "nonfinite_normals"}.  One device -> host read."""
    max_nn = int(max_nn)
    if not 2 <= max_nn <= hip.KNN_MAX:
        raise ValueError(f"fpfh: max_nn must be in [2, {hip.KNN_MAX}], got {max_nn}")
    r = _positive(radius, "fpfh", "radius")
    nrm = _f64_points(normals, "fpfh")
    if nrm.shape[0] != grid.n:
        raise ValueError(f"fpfh: {nrm.shape[0]} normals for {grid.n} targets")
    dev = grid.buf.device
    features = torch.empty(grid.n, hip.FPFH_DIM, device=dev, dtype=torch.float64)
    ws, need = _scratch(load().lnr_cloud_fpfh_workspace(grid.n), dev, f"fpfh: {grid.n} points, the limit is 2^31 - 4096")
    counters = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_cloud_fpfh(_ptr(grid.buf), grid.n, _ptr(nrm), r, max_nn, _ptr(features), _ptr(ws), need, _ptr(counters), _stream()),
          "lnr_cloud_fpfh")
    c = counters.cpu()
    if int(c[1]):
        raise RuntimeError("fpfh: the grid is unusable (non-finite targets)")
    if stats is not None:
        stats.update(fallback=int(c[0]), shells=int(c[2]), nonfinite_normals=int(c[3]))
    return features


def _features(t, what, name):
    require_device(t)
    if t.dim() != 2 or not 1 <= t.shape[1] <= hip.FEATURE_DIM_MAX or not t.dtype.is_floating_point:
        raise ValueError(f"{what}: {name} [n,dim] of a float dtype with dim in [1, {hip.FEATURE_DIM_MAX}], got {tuple(t.shape)} {t.dtype}")
    return t.to(torch.float64).contiguous()


def feature_nearest(targets, queries, split=0):
    """-> (index int32 [n_q]: the target with the smallest (d2, index), -1 for none; d2 fp64 [n_q], +inf for none), exact and brute
    force (include/loner_hip.h: lnr_feature_nearest).  targets [n_t,dim], queries [n_q,dim], dim in [1, 64].  split: 0 for the
    library's rule, else the slices of the targets wanted (the result does not depend on it).  No host read."""
    tgt = _features(targets, "feature_nearest", "targets")
    qry = _features(queries, "feature_nearest", "queries")
    if tgt.shape[1] != qry.shape[1]:
        raise ValueError(f"feature_nearest: targets of dim {tgt.shape[1]}, queries of dim {qry.shape[1]}")
    split = int(split)
    if not 0 <= split <= 512:
        raise ValueError(f"feature_nearest: split must be in [0, 512], got {split}")
    n_q, dev = qry.shape[0], qry.device
    index = torch.empty(n_q, device=dev, dtype=torch.int32)
    d2 = torch.empty(n_q, device=dev, dtype=torch.float64)
    ws, need = _scratch(load().lnr_feature_nearest_workspace(n_q), dev)
    check(load().lnr_feature_nearest(_ptr(tgt), tgt.shape[0], _ptr(qry), n_q, tgt.shape[1], split, _ptr(index), _ptr(d2), _ptr(ws), need,
                                     _stream()), "lnr_feature_nearest")
    return index, d2


def ransac_correspondence(source, target, corr, max_distance, edge_similarity=0.9, hypotheses=65536, seed=0, strict=True):
    """RANSAC over given correspondences with a fixed number of hypotheses (include/loner_hip.h: lnr_ransac_correspondence).
    source [n_s,3], target [n_t,3], corr int [m,2] (source index, target index) on the device.  -> dict with transformation (numpy
    fp64 4x4), fitness, inlier_rmse (over the correspondences), best_hypothesis (-1 for none), n_inliers, survivors,
    rejected_repeated, rejected_edge, rejected_frame, n_correspondences, status.  strict: RuntimeError on a status bit (fewer than 3
    correspondences, no survivor, an index out of range); otherwise the bits are the caller's to read.  One device -> host read."""
    src = _f64_points(source, "ransac_correspondence")
    tgt = _f64_points(target, "ransac_correspondence")
    require_device(corr)
    if corr.dim() != 2 or corr.shape[1] != 2 or corr.dtype.is_floating_point:
        raise ValueError(f"ransac_correspondence: corr [m,2] of an integer dtype, got {tuple(corr.shape)} {corr.dtype}")
    d = _positive(max_distance, "ransac_correspondence", "max_distance")
    e = float(edge_similarity)
    if not (math.isfinite(e) and 0.0 <= e <= 1.0):
        raise ValueError(f"ransac_correspondence: edge_similarity must be in [0, 1], got {edge_similarity!r}")
    H = int(hypotheses)
    if not 1 <= H <= hip.RANSAC_MAX_HYPOTHESES:
        raise ValueError(f"ransac_correspondence: hypotheses must be in [1, {hip.RANSAC_MAX_HYPOTHESES}], got {hypotheses!r}")
    corr = corr.to(torch.int32).contiguous()
    m, dev = corr.shape[0], src.device
    lib = load()
    ws, need = _scratch(lib.lnr_ransac_workspace(m, H), dev, f"ransac_correspondence: {m} correspondences, the limit is 2^31 - 4096")
    result = torch.empty(18, device=dev, dtype=torch.float64)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    check(lib.lnr_ransac_correspondence(_ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), m, H, int(seed) & _U64, d, e, _ptr(ws), need,
                                        _ptr(result), _ptr(info), _stream()), "lnr_ransac_correspondence")
    res = result.cpu().numpy()
    info = [int(x) for x in info.cpu()]
    if strict and info[0]:
        raise RuntimeError("ransac_correspondence: " + ", ".join(t for b, t in _RANSAC_STATUS.items() if info[0] & b))
    return {"transformation": res[:16].reshape(4, 4).copy(), "fitness": float(res[16]), "inlier_rmse": float(res[17]), "status": info[0],
            "best_hypothesis": info[1], "n_inliers": info[2], "survivors": info[3], "rejected_repeated": info[4], "rejected_edge": info[5],
            "rejected_frame": info[6], "n_correspondences": info[7]}


def correspondences_from_features(source_feature, target_feature, mutual_filter=False):
    """int32 [m,2] on the device: (i, c(i)) with c(i) the target whose feature is nearest to source feature i under (d2, index)
    (include/loner_hip.h: lnr_feature_nearest), for every i that has one.  mutual_filter: the same search the other way, and i is kept
    only where back[c(i)] == i.  Features [n,dim], dim <= 64."""
    index, _ = feature_nearest(target_feature, source_feature)
    i = torch.arange(index.shape[0], device=index.device, dtype=torch.int32)
    keep = index >= 0
    if mutual_filter:
        back, _ = feature_nearest(source_feature, target_feature)
        keep = keep & (back[index.clamp(min=0).long()] == i)
    return torch.stack([i[keep], index[keep]], dim=1).contiguous()


def _evaluated(source, target, T, max_correspondence_distance, hypotheses):
    """RegistrationResult of T on the real clouds: fitness and inlier_rmse through NNGrid.correspondences, as open3d re-evaluates"""
    dev = target.points.device
    moved = ops.cloud_transform(source.points.to(dev), T)
    index, d2 = ops.NNGrid(target.points, max_correspondence_distance).correspondences(moved, max_correspondence_distance)
    hit = index >= 0
    k = int(hit.sum())
    n = len(source)
    rmse = float(torch.sqrt(d2[hit].sum() / k)) if k else 0.0
    return RegistrationResult(T, k / n if n else 0.0, rmse, k, hypotheses)


def registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance, edge_length_similarity=0.9,
                                                hypotheses=65536, seed=0):
    """open3d's registration_ransac_based_on_correspondence on the device (include/loner_hip.h: lnr_ransac_correspondence) ->
    RegistrationResult; .iterations holds the number of hypotheses.  corres int [m,2] (source index, target index) on the device.
    Differences by intent: `hypotheses` is a fixed count (no confidence-based early stop), each pose comes from the sample's two
    triangle frames (no Kabsch fit, no refit on the inliers), and the draws are Philox under `seed`.  RuntimeError with fewer than 3
    correspondences or when no hypothesis survives."""
    r = _positive(max_correspondence_distance, "registration_ransac_based_on_correspondence", "max_correspondence_distance")
    dev = target.points.device
    out = ransac_correspondence(source.points.to(dev), target.points, corres.to(dev), r, edge_length_similarity, hypotheses, seed)
    return _evaluated(source, target, out["transformation"], r, int(hypotheses))


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter,
                                                  max_correspondence_distance, edge_length_similarity=0.9, hypotheses=65536, seed=0):
    """open3d's registration_ransac_based_on_feature_matching: correspondences_from_features, then
    registration_ransac_based_on_correspondence.  Fitness and inlier_rmse are re-evaluated on the real clouds."""
    dev = target.points.device
    corres = correspondences_from_features(source_feature.to(dev), target_feature.to(dev), mutual_filter)
    return registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance, edge_length_similarity,
                                                       hypotheses, seed)


def global_registration(source, target, voxel_size, orient=None, refine=True, kernel=None, hypotheses=65536, seed=0):
    """A pose of `source` on `target` from the two PointClouds alone -> RegistrationResult.  In order: both down-sampled at
    voxel_size; normals with knn 30; orientation, towards each cloud's own centroid by default (rigid-equivariant), or towards the
    viewpoints orient = (source viewpoint, target viewpoint); FPFH at radius 5 voxel_size and max_nn 32; RANSAC on the feature
    matches at 1.5 voxel_size; with refine, point-to-plane ICP at 3 voxel_size and then 1.5 voxel_size from the result (kernel: a
    RobustKernel on the residuals, optional).  Neither cloud is changed."""
    v = _positive(voxel_size, "global_registration", "voxel_size")
    if orient is not None and len(orient) != 2:
        raise ValueError("global_registration: orient must be None or (source viewpoint, target viewpoint)")
    from .lidar_map import registration_icp
    dev = target.points.device
    clouds, features = [], []
    for k, cloud in enumerate((source, target)):
        down = cloud.voxel_down_sample(v)
        if len(down) < 3:
            raise ValueError(f"global_registration: {len(down)} points after down-sampling at {v}")
        down.points = down.points.to(dev)
        down.estimate_normals(30)
        down.orient_normals_towards_location(down.points.mean(0) if orient is None else orient[k])
        clouds.append(down)
        features.append(down.compute_fpfh_feature(5.0 * v, 32))
    result = registration_ransac_based_on_feature_matching(clouds[0], clouds[1], features[0], features[1], False, 1.5 * v, 0.9, hypotheses, seed)
    if refine:
        for r in (3.0 * v, 1.5 * v):
            if kernel is None:
                result = registration_icp(clouds[0], clouds[1], r, result.transformation)
            else:
                result = registration_icp_robust(clouds[0], clouds[1], r, result.transformation, kernel=kernel)
    return result


# ---------------------------------------------------------------- information matrix of a registered pair
_INFORMATION_STATUS = {1: "non-finite source points", 2: "the target grid is unusable (non-finite targets)"}


def icp_information(grid, source, max_distance, transformation, stats=None):
    """include/loner_hip.h: lnr_icp_information.  grid: an ops.NNGrid over the targets; source [m,3] as it is before
    `transformation` (4x4, finite, affine).  -> the 6x6 fp64 information matrix on the device: sum of G^T G, G = [-[q]x | I], over
    the correspondences within max_distance; zeros without one.  stats (a dict, optional) receives {"status", "n_correspondences",
    "nonfinite_source"} (one device -> host read, only then; nothing is raised here)."""
    src = _f64_points(source, "icp_information")
    r = _positive(max_distance, "icp_information", "max_correspondence_distance")
    T = ops.affine_f64(transformation, "icp_information: transformation must be a finite 4x4 affine matrix", finite=True)
    dev = src.device
    lib = load()
    ws, need = _scratch(lib.lnr_icp_workspace(src.shape[0]), dev)
    result = torch.empty(36, device=dev, dtype=torch.float64)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    t16 = (C.c_double * 16)(*[float(x) for x in T.reshape(-1)])
    check(lib.lnr_icp_information(_ptr(grid.buf), grid.n, _ptr(src), src.shape[0], t16, r, _ptr(ws), need, _ptr(result), _ptr(info),
                                  _stream()), "lnr_icp_information")
    if stats is not None:
        c = info.cpu()
        stats.update(status=int(c[0]), n_correspondences=int(c[1]), nonfinite_source=int(c[2]))
    return result.reshape(6, 6)


def get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation):
    """open3d's get_information_matrix_from_point_clouds on the device -> numpy fp64 6x6 (rotation columns first, as the ICP's x).
    The search grid's cell edge is the correspondence distance.  RuntimeError on a status bit; no correspondence gives zeros."""
    r = _positive(max_correspondence_distance, "get_information_matrix_from_point_clouds", "max_correspondence_distance")
    T = ops.affine_f64(transformation, "get_information_matrix_from_point_clouds: transformation must be a finite 4x4 affine matrix",
                       finite=True)
    stats = {}
    out = icp_information(ops.NNGrid(target.points, r), source.points.to(target.points.device), r, T, stats)
    _raise_status("get_information_matrix_from_point_clouds", stats["status"], _INFORMATION_STATUS)
    return out.cpu().numpy()
