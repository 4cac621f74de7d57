"""Multiway registration on the device: open3d's PoseGraph, global_optimization (Levenberg-Marquardt with the line process of Choi et
al., CVPR 2015) and the workflow that builds a pose graph from clouds (include/loner_hip.h, "pose graph"; the kernels are
loner_amd/csrc/lnr_pose_graph.hip).

  PoseGraphNode, PoseGraphEdge, PoseGraph      open3d's containers: numpy fp64 4x4 poses and transformations, 6x6 information
  GlobalOptimizationConvergenceCriteria, GlobalOptimizationOption      open3d's, plus the linear solver's rtol and max_cg
  DeviceGraph                the tensors of one graph on the device and the four entry points on them (build, linearize, solve, optimize)
  global_optimization        in place: optimise, drop uncertain edges whose line-process value fell below edge_prune_threshold, optimise
  multiway_registration      clouds and initial poses -> a PoseGraph: odometry edges between consecutive clouds (certain), loop candidates
                             from pose proximity (uncertain), each refined by ICP and weighted by its information matrix
  refine_trajectory          scans and a TUM trajectory -> the optimised TUM trajectory

Conventions: node i's pose takes its frame to the world; an edge's transformation takes source-frame points to the target frame, so a
consistent graph has inv(pose_t) @ pose_s == transformation.  A step is pose <- M(delta) pose with the ICP's Rz Ry Rx rule.

Limits, by intent.  The linear systems are solved by block-Jacobi preconditioned conjugate gradients to a relative residual rtol, not
by a direct factorisation: a step carries an error of the order of cond(H + lambda I) rtol, and a small graph is bound by its launches
(five per conjugate-gradient iteration), not by arithmetic.  There is no place recognition: loop candidates come from the initial poses
alone, so a trajectory that has drifted by more than loop_radius finds no loop.  No marginal covariances are computed.  The neural map
is not trained again on the corrected poses.  The relative-increment test measures the step against the norm of the node positions
(open3d: against its 6 n parameter vector), and the gain ratio's denominator has no damping constant added."""
import math

import numpy as np
import torch

from .. import hip
from ..hip import _ptr, _stream, check, load
from ..ops._common import _positive, _raise_status, _scratch

_STATUS = {1: "an edge names a node out of range", 2: "a self edge", 4: "a non-finite pose", 8: "a non-finite measurement or information matrix",
           16: "the conjugate gradients broke down (the system is not positive definite)"}
STOP_REASONS = ("trials ran out", "max_iteration", "min_relative_increment", "min_right_term", "min_residual", "max_iteration_lm", "status")


def _mat(a, shape, what):
    a = np.array(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{what}: expected {shape[0]}x{shape[1]}, got {a.shape}")
    return a


class PoseGraphNode:
    def __init__(self, pose=None):
        self.pose = _mat(np.eye(4) if pose is None else pose, (4, 4), "PoseGraphNode: pose")


class PoseGraphEdge:
    def __init__(self, source_node_id=-1, target_node_id=-1, transformation=None, information=None, uncertain=False, confidence=1.0):
        self.source_node_id = int(source_node_id)
        self.target_node_id = int(target_node_id)
        self.transformation = _mat(np.eye(4) if transformation is None else transformation, (4, 4), "PoseGraphEdge: transformation")
        self.information = _mat(np.eye(6) if information is None else information, (6, 6), "PoseGraphEdge: information")
        self.uncertain = bool(uncertain)
        self.confidence = float(confidence)


class PoseGraph:
    def __init__(self, nodes=None, edges=None):
        self.nodes = list(nodes) if nodes is not None else []
        self.edges = list(edges) if edges is not None else []

    def poses(self):
        return np.stack([n.pose for n in self.nodes]) if self.nodes else np.zeros((0, 4, 4))


class GlobalOptimizationConvergenceCriteria:
    """open3d's defaults; rtol and max_cg (None: 6 n, at most 2000) belong to the conjugate gradients of every trial."""

    def __init__(self, max_iteration=100, min_relative_increment=1e-6, min_right_term=1e-6, min_residual=1e-6, max_iteration_lm=20,
                 rtol=1e-10, max_cg=None):
        self.max_iteration = int(max_iteration)
        self.min_relative_increment = float(min_relative_increment)
        self.min_right_term = float(min_right_term)
        self.min_residual = float(min_residual)
        self.max_iteration_lm = int(max_iteration_lm)
        self.rtol = float(rtol)
        self.max_cg = None if max_cg is None else int(max_cg)

    def check(self, what):
        if not 0 <= self.max_iteration <= 10000:
            raise ValueError(f"{what}: max_iteration must be in [0, 10000], got {self.max_iteration}")
        if not 1 <= self.max_iteration_lm <= 1000:
            raise ValueError(f"{what}: max_iteration_lm must be in [1, 1000], got {self.max_iteration_lm}")
        for name in ("min_relative_increment", "min_right_term", "min_residual", "rtol"):
            v = getattr(self, name)
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"{what}: {name} must be finite and >= 0, got {v!r}")
        if self.max_cg is not None and not 1 <= self.max_cg <= 100000:
            raise ValueError(f"{what}: max_cg must be in [1, 100000], got {self.max_cg}")


class GlobalOptimizationOption:
    def __init__(self, max_correspondence_distance=0.075, edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=-1):
        self.max_correspondence_distance = float(max_correspondence_distance)
        self.edge_prune_threshold = float(edge_prune_threshold)
        self.preference_loop_closure = float(preference_loop_closure)
        self.reference_node = int(reference_node)

    def check(self, what, n_nodes):
        _positive(self.max_correspondence_distance, what, "max_correspondence_distance")
        _positive(self.preference_loop_closure, what, "preference_loop_closure")
        if not (math.isfinite(self.edge_prune_threshold) and 0.0 <= self.edge_prune_threshold <= 1.0):
            raise ValueError(f"{what}: edge_prune_threshold must be in [0, 1], got {self.edge_prune_threshold!r}")
        if not -1 <= self.reference_node < n_nodes:
            raise ValueError(f"{what}: reference_node must be -1 or a node in [0, {n_nodes}), got {self.reference_node}")


def _default_device():
    from ..common.ray_utils import mapping_device
    return mapping_device()


class DeviceGraph:
    """One graph's arrays on the device.  source, target int [m]; poses [n,4,4]; transformations [m,4,4]; information [m,6,6];
    uncertain bool [m] (numpy or tensors).  The adjacency is built at once; `status` (a host read) holds its status word."""

    def __init__(self, n_nodes, source, target, transformations=None, information=None, uncertain=None, poses=None, device=None):
        n, src = int(n_nodes), np.asarray(source, dtype=np.int64).reshape(-1)
        tgt = np.asarray(target, dtype=np.int64).reshape(-1)
        m = len(src)
        if not 1 <= n <= hip.PG_MAX_NODES or m > hip.PG_MAX_EDGES:
            raise ValueError(f"DeviceGraph: {n} nodes and {m} edges; nodes must be in [1, {hip.PG_MAX_NODES}] and edges in [0, {hip.PG_MAX_EDGES}]")
        if len(tgt) != m:
            raise ValueError(f"DeviceGraph: {m} source ids and {len(tgt)} target ids")
        if m and (np.abs(src).max() >= 2 ** 31 or np.abs(tgt).max() >= 2 ** 31):
            raise ValueError("DeviceGraph: a node id does not fit 32 bits")
        X = np.tile(np.eye(4), (m, 1, 1)) if transformations is None else np.asarray(transformations, dtype=np.float64)
        L = np.tile(np.eye(6), (m, 1, 1)) if information is None else np.asarray(information, dtype=np.float64)
        P = np.tile(np.eye(4), (n, 1, 1)) if poses is None else np.asarray(poses, dtype=np.float64)
        u = np.zeros(m, dtype=bool) if uncertain is None else np.asarray(uncertain).astype(bool).reshape(-1)
        if X.shape != (m, 4, 4) or L.shape != (m, 6, 6) or P.shape != (n, 4, 4) or u.shape != (m,):
            raise ValueError(f"DeviceGraph: transformations [{m},4,4], information [{m},6,6], uncertain [{m}] and poses [{n},4,4]; got "
                             f"{X.shape}, {L.shape}, {u.shape} and {P.shape}")
        dev = _default_device() if device is None else torch.device(device)
        self.n, self.m, self.device = n, m, dev
        self.source = torch.from_numpy(src.astype(np.int32)).to(dev)
        self.target = torch.from_numpy(tgt.astype(np.int32)).to(dev)
        self.transformations = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        self.information = torch.from_numpy(np.ascontiguousarray(L)).to(dev)
        self.uncertain = torch.from_numpy(u.astype(np.int32)).to(dev)
        self.poses = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
        self.line = torch.ones(m, dtype=torch.float64, device=dev)
        lib = load()
        self.graph, self.graph_bytes = _scratch(lib.lnr_pose_graph_bytes(n, m), dev)
        self.ws, self.ws_bytes = _scratch(lib.lnr_pose_graph_workspace(n, m), dev)
        info = torch.empty(4, device=dev, dtype=torch.int64)
        check(lib.lnr_pose_graph_build(_ptr(self.source), _ptr(self.target), n, m, _ptr(self.graph), self.graph_bytes, _ptr(self.ws),
                                       self.ws_bytes, _ptr(info), _stream()), "lnr_pose_graph_build")
        self.build_info = info

    @property
    def status(self):
        return int(self.build_info[0].cpu())

    def adjacency(self):
        """(row_start int64 [n+1], slots int64 [2m]) as numpy: slot = 2 k + role"""
        raw = self.graph.cpu().numpy()
        rs = 256
        row = raw[rs:rs + 4 * (self.n + 1)].view(np.uint32).astype(np.int64)
        so = (rs + 4 * (self.n + 1) + 255) // 256 * 256
        return row, raw[so:so + 8 * self.m].view(np.uint32).astype(np.int64)

    def _reference(self, reference_node, what):
        r = int(reference_node)
        if not -1 <= r < self.n:
            raise ValueError(f"{what}: reference_node must be -1 or a node in [0, {self.n}), got {reference_node!r}")
        return r

    def linearize(self, reference_node=-1):
        """-> dict of device tensors e [m,6], q [m], W [m,6,6], g [m,6], H_diag [n,6,6], b [n,6] and "status" (one host read)"""
        r = self._reference(reference_node, "linearize")
        dev, n, m = self.device, self.n, self.m
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float64)     # noqa: E731
        out = {"e": f(m, 6), "q": f(m), "W": f(m, 6, 6), "g": f(m, 6), "H_diag": f(n, 6, 6), "b": f(n, 6)}
        info = torch.empty(4, device=dev, dtype=torch.int64)
        check(load().lnr_pose_graph_linearize(_ptr(self.graph), n, m, _ptr(self.source), _ptr(self.target), _ptr(self.poses),
                                              _ptr(self.transformations), _ptr(self.information), _ptr(self.uncertain), _ptr(self.line), r,
                                              _ptr(out["e"]), _ptr(out["q"]), _ptr(out["W"]), _ptr(out["g"]), _ptr(out["H_diag"]),
                                              _ptr(out["b"]), _ptr(self.ws), self.ws_bytes, _ptr(info), _stream()),
              "lnr_pose_graph_linearize")
        out["status"] = int(info[0].cpu())
        return out

    def solve(self, lin, lam, reference_node=-1, rtol=1e-10, max_cg=None):
        """(H + lam I) delta = lin["b"] -> (delta [n,6] on the device, {"status", "iterations", "converged"}); one host read"""
        r = self._reference(reference_node, "solve")
        lam, rtol = float(lam), float(rtol)
        if not (math.isfinite(lam) and lam >= 0):
            raise ValueError(f"solve: lambda must be finite and >= 0, got {lam!r}")
        max_cg = _max_cg(max_cg, self.n)
        delta = torch.empty(self.n, 6, device=self.device, dtype=torch.float64)
        info = torch.empty(4, device=self.device, dtype=torch.int64)
        check(load().lnr_pose_graph_solve(_ptr(self.graph), self.n, self.m, _ptr(self.source), _ptr(self.target), _ptr(lin["W"]),
                                          _ptr(self.uncertain), _ptr(self.line), _ptr(lin["H_diag"]), _ptr(lin["b"]), lam, r, rtol, max_cg,
                                          _ptr(self.ws), self.ws_bytes, _ptr(delta), _ptr(info), _stream()), "lnr_pose_graph_solve")
        c = info.cpu()
        return delta, {"status": int(c[0]), "iterations": int(c[1]), "converged": bool(c[2])}

    def optimize(self, criteria, option):
        """Levenberg-Marquardt on self.poses and self.line, in place -> the counters (host reads: one word per trial, then the result)"""
        c = criteria
        trials = c.max_iteration * (c.max_iteration_lm + 1)
        history = torch.zeros(max(trials, 1), device=self.device, dtype=torch.int32)
        result = torch.empty(4, device=self.device, dtype=torch.float64)
        info = torch.empty(8, device=self.device, dtype=torch.int64)
        check(load().lnr_pose_graph_optimize(_ptr(self.graph), self.n, self.m, _ptr(self.source), _ptr(self.target), _ptr(self.poses),
                                             _ptr(self.transformations), _ptr(self.information), _ptr(self.uncertain), _ptr(self.line),
                                             option.reference_node, option.max_correspondence_distance, option.preference_loop_closure,
                                             c.max_iteration, c.max_iteration_lm, c.min_relative_increment, c.min_right_term, c.min_residual,
                                             c.rtol, _max_cg(c.max_cg, self.n), _ptr(self.ws), self.ws_bytes, _ptr(history), trials,
                                             _ptr(result), _ptr(info), _stream()), "lnr_pose_graph_optimize")
        res, words = result.cpu().numpy(), [int(x) for x in info.cpu()]
        return {"status": words[0], "trials": words[1], "cg_iterations": words[2], "accepted": words[3], "rejected": words[4],
                "stop_reason": STOP_REASONS[words[5]], "cg_capped": words[7], "F": float(res[0]), "b_inf": float(res[1]), "lambda": float(res[2]),
                "mu": float(res[3]), "history": history[:words[1]].cpu().numpy().tolist()}


def _max_cg(max_cg, n):
    if max_cg is None:
        return min(max(6 * n, 16), 2000)
    if not 1 <= int(max_cg) <= 100000:
        raise ValueError(f"max_cg must be in [1, 100000], got {max_cg!r}")
    return int(max_cg)


def _device_graph(pose_graph, device):
    e = pose_graph.edges
    return DeviceGraph(len(pose_graph.nodes), [x.source_node_id for x in e], [x.target_node_id for x in e],
                       np.stack([x.transformation for x in e]) if e else None, np.stack([x.information for x in e]) if e else None,
                       [x.uncertain for x in e], pose_graph.poses(), device)


def global_optimization(pose_graph, criteria=None, option=None, info=None, device=None):
    """open3d's global_optimization(pose_graph, GlobalOptimizationLevenbergMarquardt(), criteria, option), in place: optimise; drop
    every uncertain edge whose line-process value ended below option.edge_prune_threshold; optimise what is left.  The nodes' poses
    and the edges' confidence (the line-process value; 1 for certain edges) are updated.  info (a dict, optional) receives "first" and
    "second" (the counters of the two passes; "cg_capped" counts the trials whose solve ran into max_cg before rtol, so that their
    steps are inexact: raise max_cg, or distrust a result that did not stop on min_right_term) and "pruned" (the indices, in the graph as given, of the edges dropped).  RuntimeError
    on a status bit (an edge naming a missing node, a self edge, non-finite input, a breakdown of the conjugate gradients)."""
    what = "global_optimization"
    if not isinstance(pose_graph, PoseGraph):
        raise ValueError(f"{what}: pose_graph must be a PoseGraph, got {type(pose_graph).__name__}")
    criteria = GlobalOptimizationConvergenceCriteria() if criteria is None else criteria
    option = GlobalOptimizationOption() if option is None else option
    n = len(pose_graph.nodes)
    if n < 1:
        raise ValueError(f"{what}: the pose graph has no node")
    criteria.check(what)
    option.check(what, n)
    for k, e in enumerate(pose_graph.edges):
        if not (0 <= e.source_node_id < n and 0 <= e.target_node_id < n) or e.source_node_id == e.target_node_id:
            raise ValueError(f"{what}: edge {k} joins nodes {e.source_node_id} and {e.target_node_id} of {n}")
    passes = {}
    kept = list(range(len(pose_graph.edges)))
    pruned = []
    for name in ("first", "second"):
        g = _device_graph(pose_graph, device)
        out = g.optimize(criteria, option)
        _raise_status(what, out["status"], _STATUS)
        passes[name] = out
        poses, line = g.poses.cpu().numpy(), g.line.cpu().numpy()
        for node, T in zip(pose_graph.nodes, poses):
            node.pose = T.copy()
        for e, l in zip(pose_graph.edges, line):
            e.confidence = float(l) if e.uncertain else 1.0
        if name == "first":
            keep = [not (e.uncertain and e.confidence < option.edge_prune_threshold) for e in pose_graph.edges]
            pruned = [k for k, ok in zip(kept, keep) if not ok]
            pose_graph.edges = [e for e, ok in zip(pose_graph.edges, keep) if ok]
    if info is not None:
        info.update(passes, pruned=pruned)
    return pose_graph


def multiway_registration(clouds, init_poses, max_correspondence_distance, loop_radius, min_gap=2, estimation="GENERALIZED", kernel=None,
                          min_fitness=0.3, max_iteration=30, info=None):
    """A PoseGraph over `clouds` (PointClouds, each in its own sensor frame) from their initial poses (numpy [n,4,4], frame to world).
    Odometry edges join consecutive clouds (k -> k + 1) and are certain.  Loop candidates join every pair whose initial positions lie
    within loop_radius of each other and whose indices differ by at least min_gap (>= 2); they are uncertain.  There is no place
    recognition: candidates come from pose proximity only, so drift beyond loop_radius hides a loop.  Each edge starts from
    inv(pose_t) @ pose_s, is refined by the ICP entry points (estimation "GENERALIZED" or "POINT_TO_PLANE", kernel: a RobustKernel
    or None) at max_correspondence_distance and gets the information matrix of the refined pair
    (get_information_matrix_from_point_clouds).  An edge whose refined fitness is below min_fitness is not added (an odometry edge
    too: the graph may then fall apart, and info says so).  info (a dict, optional) receives "edges" (per edge tried: source, target,
    uncertain, fitness, inlier_rmse, added)."""
    from .. import ops
    from . import registration as REG
    from .lidar_map import PointCloud
    what = "multiway_registration"
    d = _positive(max_correspondence_distance, what, "max_correspondence_distance")
    radius = _positive(loop_radius, what, "loop_radius")
    min_gap = int(min_gap)
    if min_gap < 2:
        raise ValueError(f"{what}: min_gap must be >= 2 (consecutive clouds are odometry edges), got {min_gap}")
    estimation = str(estimation).upper()
    if estimation not in ("GENERALIZED", "POINT_TO_PLANE"):
        raise ValueError(f"{what}: estimation must be GENERALIZED or POINT_TO_PLANE, got {estimation!r}")
    min_fitness = float(min_fitness)
    if not 0.0 <= min_fitness <= 1.0:
        raise ValueError(f"{what}: min_fitness must be in [0, 1], got {min_fitness!r}")
    poses = np.asarray(init_poses, dtype=np.float64)
    n = len(clouds)
    if poses.shape != (n, 4, 4) or n < 1:
        raise ValueError(f"{what}: {n} clouds need init_poses [{n},4,4], got {poses.shape}")
    if not np.isfinite(poses).all():
        raise ValueError(f"{what}: init_poses must be finite")
    pairs = [(k, k + 1, False) for k in range(n - 1)]
    pos = poses[:, :3, 3]
    pairs += [(i, j, True) for i in range(n) for j in range(i + min_gap, n) if np.linalg.norm(pos[i] - pos[j]) <= radius]
    prepared = {}

    def prepare(k):
        """per cloud, once: a copy with normals, its covariances for GENERALIZED, and the search grid every edge into it shares"""
        if k not in prepared:
            c = PointCloud(clouds[k].points)
            c.normals, c.covariances = clouds[k].normals, clouds[k].covariances
            if c.normals is None:
                c.estimate_normals(20)
            cov = REG.cloud_covariances(c) if estimation == "GENERALIZED" else None
            prepared[k] = (c, cov, None)
        return prepared[k]

    def grid_of(k):                                          # only targets need one
        c, cov, grid = prepare(k)
        if grid is None:
            grid = ops.NNGrid(c.points, d)
            prepared[k] = (c, cov, grid)
        return grid

    graph = PoseGraph([PoseGraphNode(T) for T in poses])
    tried = []
    for s, t, uncertain in pairs:
        (src, src_cov, _), (tgt, tgt_cov, _) = prepare(s), prepare(t)
        grid = grid_of(t)
        init = np.linalg.inv(poses[t]) @ poses[s]
        init[3] = [0.0, 0.0, 0.0, 1.0]
        if estimation == "GENERALIZED":
            r = REG.icp_generalized(grid, tgt_cov, src.points, src_cov, d, init, max_iteration=max_iteration, kernel=kernel)
        elif kernel is None:
            r = ops.icp_point_to_plane(grid, tgt.normals, src.points, d, init, max_iteration=max_iteration)
        else:
            r = REG.icp_point_to_plane_robust(grid, tgt.normals, src.points, d, init, max_iteration=max_iteration, kernel=kernel)
        added = r["fitness"] >= min_fitness
        if added:
            stats = {}
            L = REG.icp_information(grid, src.points, d, r["transformation"], stats)
            _raise_status(what, stats["status"], REG._INFORMATION_STATUS)
            graph.edges.append(PoseGraphEdge(s, t, r["transformation"], L, uncertain))
        tried.append({"source": s, "target": t, "uncertain": uncertain, "fitness": r["fitness"], "inlier_rmse": r["inlier_rmse"],
                      "added": added})
    if info is not None:
        info["edges"] = tried
    return graph


def refine_trajectory(scans, trajectory_file, out_file, max_correspondence_distance=0.5, loop_radius=3.0, min_gap=4,
                      estimation="GENERALIZED", kernel=None, min_fitness=0.3, voxel_size=None, criteria=None, option=None, info=None):
    """scans: LidarScans (or (xyz [n,3], ...) pairs) in their sensor frames, one per row of the TUM file `trajectory_file` in order;
    each becomes a cloud (down-sampled at voxel_size when given), multiway_registration builds the graph from the file's poses,
    global_optimization (reference node 0 unless option says otherwise) optimises it, and the poses are written to out_file as TUM
    rows with the file's stamps (dump_trajectory_to_tum's format).  -> the rows written [n,8]."""
    from ..common.pose_utils import dump_trajectory_to_tum, quat_to_matrix, read_tum
    from .lidar_map import PointCloud
    rows = read_tum(trajectory_file) if isinstance(trajectory_file, (str, bytes)) or hasattr(trajectory_file, "__fspath__") \
        else np.asarray(trajectory_file, dtype=np.float64)
    scans = list(scans)
    if rows.ndim != 2 or rows.shape[1] != 8 or len(rows) != len(scans):
        raise ValueError(f"refine_trajectory: {len(scans)} scans need {len(scans)} TUM rows [n,8], got {rows.shape}")
    poses = np.tile(np.eye(4), (len(rows), 1, 1))
    poses[:, :3, :3] = quat_to_matrix(rows[:, 4:])
    poses[:, :3, 3] = rows[:, 1:4]
    clouds = []
    for scan in scans:
        xyz = (scan.ray_directions.double() * scan.distances.double()).T if hasattr(scan, "ray_directions") else scan[0]
        cloud = PointCloud(xyz.contiguous() if torch.is_tensor(xyz) else xyz)
        clouds.append(cloud.voxel_down_sample(voxel_size) if voxel_size else cloud)
    graph = multiway_registration(clouds, poses, max_correspondence_distance, loop_radius, min_gap, estimation, kernel, min_fitness, info=info)
    option = GlobalOptimizationOption(max_correspondence_distance, reference_node=0) if option is None else option
    global_optimization(graph, criteria, option, info)
    P = torch.from_numpy(graph.poses())
    dump_trajectory_to_tum(P, torch.from_numpy(rows[:, 0].copy()), out_file)
    return read_tum(out_file)
