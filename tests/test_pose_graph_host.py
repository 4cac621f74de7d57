"""The pose graph on the CPU: the library's symbols, the argument errors raised before a device is touched, the analytic Jacobians
of the restatement (tests/pose_graph_restatement.py) against central differences, and the conditions the GPU tests' graphs rest on."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import pose_graph_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lnr_icp_information", "lnr_pose_graph_bytes", "lnr_pose_graph_workspace", "lnr_pose_graph_build", "lnr_pose_graph_linearize",
           "lnr_pose_graph_solve", "lnr_pose_graph_optimize")
RTOL = 1e-13                     # the conjugate gradients' tolerance in the GPU tests of the solve and the optimiser


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from loner_amd import hip
    return hip.load()


def test_the_new_symbols_are_declared_bound_and_exported(lib):
    from loner_amd import build, hip
    header = open(os.path.join(ROOT, "include", "loner_hip.h")).read()
    declared = set(re.findall(r"\b(lnr_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/loner_hip.h"
        assert name in hip.declared_symbols(), f"{name} is not in the ctypes table"
        assert hasattr(lib, name), f"{name} is not exported"
    assert "lnr_pose_graph.hip" in build.EXACT and any(s[0] == "lnr_pose_graph.hip" for s in build.SOURCES)
    assert int(re.search(r"#define LNR_PG_MAX_NODES \(1 << (\d+)\)", header).group(1)) == 24 and hip.PG_MAX_NODES == 1 << 24
    assert int(re.search(r"#define LNR_PG_MAX_EDGES \(1 << (\d+)\)", header).group(1)) == 26 and hip.PG_MAX_EDGES == 1 << 26
    assert lib.lnr_pose_graph_bytes(0, 0) == 0 and lib.lnr_pose_graph_bytes((1 << 24) + 1, 0) == 0 and lib.lnr_pose_graph_bytes(1, -1) == 0
    assert lib.lnr_pose_graph_bytes(1, 0) > 0 and lib.lnr_pose_graph_workspace(8, 8) > lib.lnr_pose_graph_workspace(8, 0) > 0
    assert lib.lnr_pose_graph_workspace(1, (1 << 26) + 1) == 0


def test_host_entries_refuse_bad_arguments(lib):
    eye = (torch.eye(4, dtype=torch.float64).reshape(-1).numpy()).ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_double))
    for r, word in ((0.0, b"max_distance"), (float("nan"), b"max_distance"), (float("inf"), b"max_distance")):
        assert lib.lnr_icp_information(None, 0, None, 0, eye, r, None, 0, None, None, None) != 0 and word in lib.lnr_last_error()
    assert lib.lnr_icp_information(None, 0, None, 0, eye, 1.0, None, 0, None, None, None) != 0 and b"null" in lib.lnr_last_error()
    assert lib.lnr_pose_graph_build(None, None, 0, 0, None, 0, None, 0, None, None) != 0 and b"nodes" in lib.lnr_last_error()
    assert lib.lnr_pose_graph_build(None, None, 4, 0, None, 0, None, 0, None, None) != 0 and b"null" in lib.lnr_last_error()
    lin = lambda ref: lib.lnr_pose_graph_linearize(None, 4, 0, None, None, None, None, None, None, None, ref, None, None, None, None, None,   # noqa: E731
                                                   None, None, 0, None, None)
    assert lin(4) != 0 and b"reference_node" in lib.lnr_last_error()
    assert lin(-2) != 0 and b"reference_node" in lib.lnr_last_error()
    solve = lambda lam, rtol, max_cg: lib.lnr_pose_graph_solve(None, 4, 0, None, None, None, None, None, None, None, lam, -1, rtol, max_cg,   # noqa: E731
                                                               None, 0, None, None, None)
    for args, word in (((-1.0, 1e-10, 10), b"lambda"), ((float("nan"), 1e-10, 10), b"lambda"), ((0.0, -1.0, 10), b"rtol"),
                       ((0.0, 1e-10, 0), b"max_cg"), ((0.0, 1e-10, 100001), b"max_cg")):
        assert solve(*args) != 0 and word in lib.lnr_last_error()

    def optimize(d=0.1, pref=1.0, it=10, lm=5, inc=1e-6, cap=0):
        return lib.lnr_pose_graph_optimize(None, 4, 0, None, None, None, None, None, None, None, -1, d, pref, it, lm, inc, 1e-6, 1e-6, 1e-10,
                                           10, None, 0, None, cap, None, None, None)
    for kw, word in ((dict(d=0.0), b"max_correspondence_distance"), (dict(pref=-1.0), b"preference_loop_closure"),
                     (dict(it=-1), b"max_iteration"), (dict(lm=0), b"max_iteration_lm"), (dict(inc=-1.0), b"min_relative_increment"),
                     (dict(cap=4), b"history")):
        assert optimize(**kw) != 0 and word in lib.lnr_last_error()


def test_wrappers_refuse_bad_arguments_before_touching_a_device():
    from loner_amd.analysis import pose_graph as PG
    from loner_amd.analysis import registration as REG
    from loner_amd.analysis.lidar_map import PointCloud
    g = PG.PoseGraph([PG.PoseGraphNode(), PG.PoseGraphNode()], [PG.PoseGraphEdge(0, 1)])
    with pytest.raises(ValueError, match="no node"):
        PG.global_optimization(PG.PoseGraph())
    with pytest.raises(ValueError, match="PoseGraph"):
        PG.global_optimization([1, 2])
    for opt, word in ((PG.GlobalOptimizationOption(0.0), "max_correspondence_distance"), (PG.GlobalOptimizationOption(0.1, 1.5), "edge_prune"),
                      (PG.GlobalOptimizationOption(0.1, 0.25, 0.0), "preference_loop_closure"),
                      (PG.GlobalOptimizationOption(0.1, reference_node=2), "reference_node")):
        with pytest.raises(ValueError, match=word):
            PG.global_optimization(g, None, opt)
    for crit, word in ((PG.GlobalOptimizationConvergenceCriteria(max_iteration=-1), "max_iteration"),
                       (PG.GlobalOptimizationConvergenceCriteria(max_iteration_lm=0), "max_iteration_lm"),
                       (PG.GlobalOptimizationConvergenceCriteria(rtol=float("nan")), "rtol"),
                       (PG.GlobalOptimizationConvergenceCriteria(max_cg=0), "max_cg")):
        with pytest.raises(ValueError, match=word):
            PG.global_optimization(g, crit, PG.GlobalOptimizationOption(0.1))
    for s, t in ((0, 0), (0, 2), (-1, 1)):
        with pytest.raises(ValueError, match="joins nodes"):
            PG.global_optimization(PG.PoseGraph(g.nodes, [PG.PoseGraphEdge(s, t)]), None, PG.GlobalOptimizationOption(0.1))
    with pytest.raises(ValueError, match="4x4"):
        PG.PoseGraphNode(np.eye(3))
    with pytest.raises(ValueError, match="6x6"):
        PG.PoseGraphEdge(0, 1, np.eye(4), np.eye(4))
    with pytest.raises(ValueError, match="nodes must be"):
        PG.DeviceGraph(0, [], [])
    with pytest.raises(ValueError, match="target ids"):
        PG.DeviceGraph(2, [0], [])
    with pytest.raises(ValueError, match="poses"):
        PG.DeviceGraph(2, [0], [1], poses=np.zeros((3, 4, 4)))
    cloud = PointCloud.__new__(PointCloud)
    cloud.points, cloud.normals, cloud.covariances = torch.zeros(4, 3, dtype=torch.float64), None, None
    poses = np.tile(np.eye(4), (2, 1, 1))
    for kw, word in ((dict(max_correspondence_distance=0.0), "max_correspondence_distance"), (dict(loop_radius=float("nan")), "loop_radius"),
                     (dict(min_gap=1), "min_gap"), (dict(estimation="POINT"), "estimation"), (dict(min_fitness=2.0), "min_fitness")):
        args = dict(max_correspondence_distance=0.5, loop_radius=1.0)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            PG.multiway_registration([cloud, cloud], poses, **args)
    with pytest.raises(ValueError, match="init_poses"):
        PG.multiway_registration([cloud, cloud], poses[:1], 0.5, 1.0)
    for d in (0.0, float("inf")):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            REG.get_information_matrix_from_point_clouds(cloud, cloud, d, np.eye(4))
    bad = np.eye(4)
    bad[3, 0] = 1.0
    with pytest.raises(ValueError, match="affine"):
        REG.get_information_matrix_from_point_clouds(cloud, cloud, 0.1, bad)


def test_analytic_jacobians_agree_with_central_differences():
    """Central differences of the restated residual with the step h = 1e-5 on poses of order 1 to 10: the truncation error is
    h^2 / 6 times a third derivative of order |E| <= 20, about 3e-10; the rounding error 2^-52 |E| / h, about 5e-10.  Tolerance 5e-9."""
    h, tol = 1e-5, 5e-9
    rng = np.random.default_rng(0)
    worst = 0.0
    for trial in range(20):
        Ts, Tt, X = (PR.step_matrix(np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-10, 10, 3)])) for _ in range(3))
        Js, Jt = PR.jacobians(Ts, Tt, X)
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            ns = (PR.residual(PR.step_matrix(d) @ Ts, Tt, X) - PR.residual(PR.step_matrix(-d) @ Ts, Tt, X)) / (2 * h)
            nt = (PR.residual(Ts, PR.step_matrix(d) @ Tt, X) - PR.residual(Ts, PR.step_matrix(-d) @ Tt, X)) / (2 * h)
            worst = max(worst, np.abs(ns - Js[:, c]).max(), np.abs(nt - Jt[:, c]).max())
    print(f"analytic Jacobians against central differences: max |difference| {worst:.3e}")
    assert worst < tol


TIGHT = dict(min_right_term=1e-12, min_residual=1e-24, min_relative_increment=1e-14)     # exact measurements: run to the rounding floor


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (graph, reference node, max_correspondence_distance, criteria): the graphs of the GPU tests of the solve and the optimiser"""
    return {"ring 8": (PR.ring_graph(8, 0), 0, 0.5, TIGHT), "ring 65": (PR.ring_graph(65, 1), 0, 0.5, TIGHT),
            "noisy": (PR.noisy_graph(), 0, PR.NOISY["max_correspondence_distance"], {})}


@functools.lru_cache(maxsize=None)
def restated(name):
    g, ref, d, crit = scenes()[name]
    if name == "noisy":
        return PR.global_optimization(g, d, reference=ref, **crit)
    return (PR.optimize(g, d, reference=ref, **crit),)


def condition(name):
    run = restated(name)[0]
    return float(np.linalg.cond(run["H0"] + run["lambda0"] * np.eye(len(run["H0"]))))


@pytest.mark.parametrize("name", ["ring 8", "ring 65", "noisy"])
def test_the_gpu_scenes_meet_their_conditions(name):
    kappa = condition(name)
    runs = restated(name)
    print(f"{name}: cond(H + lambda0 I) {kappa:.3e}; " + "; ".join(
        f"{len(r['history'])} trials {r['history']}, stop {r['reason']}, F {r['F']:.3e}, |b|inf {r['b_inf']:.3e}, min |rho| "
        f"{min((abs(x) for x in r['rhos']), default=float('nan')):.3e}" for r in runs[:2]))
    assert 10 * kappa * RTOL < 1e-6
    for r in runs[:2]:
        line = r["line"]                                     # every edge's; a certain edge carries 1
        assert not np.any((line >= 0.15) & (line <= 0.35)), np.sort(line)
        assert all(abs(x) > 1e-3 for x in r["rhos"]), r["rhos"]
    if name == "noisy":
        g = scenes()[name][0]
        first, second, pruned = runs
        print(f"noisy: pruned {pruned}, false edges {g.false_edges}, line values {np.round(first['line'][g.uncertain], 4)}")
        assert pruned == g.false_edges                                          # the three false loops, and only they
        assert second["b_inf"] < 1e-6 and second["reason"] == "min_right_term"
    else:
        g = scenes()[name][0]
        r = runs[0]
        rel = np.stack([PR.rigid_inverse(r["poses"][0]) @ T for T in r["poses"]]) - np.stack([PR.rigid_inverse(g.truth[0]) @ T for T in g.truth])
        print(f"{name}: max |pose - truth| relative to node 0 {np.abs(rel).max():.3e}")
        assert np.abs(rel).max() < 1e-9
