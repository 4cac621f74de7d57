"""Generalized (plane-to-plane) ICP and robust loss kernels on the device: open3d's registration_generalized_icp and its RobustKernel
family (include/loner_hip.h, "robust kernels and generalized ICP"), beside lidar_map.registration_icp, which stays the plain
point-to-plane estimator.

  RobustKernel(kind, k)             "l2" | "huber" | "cauchy" | "tukey" with the scale k
  plane_covariances(normals, eps)   the covariance of a point on a plane, from its unit normal
  registration_generalized_icp      Segal et al.'s estimator on two PointClouds -> RegistrationResult
  registration_icp_robust           point-to-plane ICP with a RobustKernel on the scalar residual -> RegistrationResult
  icp_generalized, icp_point_to_plane_robust   the entry points on tensors, with the last solved system in the result (as
                                    ops.icp_point_to_plane)

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
from ..hip import _ptr, _stream, check, load
from ..ops._common import _f64_points, _positive, _raise_status, _scratch
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
