"""Timings of the pose graph's entry points on the device (profiles/pose_graph.txt); none of this is a test.

    python tools/pose_graph_probe.py [--repeats 10] [--skip-large] [--skip-information] [--graphs 64 1024 16384]

information   lnr_icp_information beside lnr_icp_correspondences alone and one round of point-to-plane ICP (max_iteration 0: one search
              and its 29 sums) on the same pair, in the same run, on the pairs of tools/gicp_probe.py: the tracker's default frame
              (two consecutive motion-distorted 64 x 1024 scans thinned to about 5 000 points) and the 1.2 M x 1.3 M room pair
optimise      global_optimization's first pass on a ring of n nodes with a loop edge from every fourth node, noisy measurements,
              beside the numpy restatement's schedule with a scipy sparse direct solve where scipy is present
Every figure is the median of --repeats device-event timings after two warm-up calls, with the spread (min, max)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loner_amd import ops                                                   # noqa: E402
from loner_amd.analysis import pose_graph as PG                             # noqa: E402
from loner_amd.analysis import registration as REG                          # noqa: E402
from tests import pose_graph_restatement as PR                              # noqa: E402

DEV = "cuda"


def timed(fn, repeats):
    for _ in range(2):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return f"median {np.median(out):9.3f} ms (min {min(out):9.3f}, max {max(out):9.3f})"


def pairs(skip_large):
    """The pairs of tools/gicp_probe.py, so that the figures sit beside profiles/gicp.txt's: -> (name, target, source, radius)"""
    from loner_amd.analysis.lidar_map import PointCloud, alignment_skip
    from loner_amd.common.frame import Frame
    from loner_amd.common.sensors import LidarScan
    from loner_amd.common.settings import default_tracking_settings
    from loner_amd.common.signals import Signal
    from loner_amd.tracking.tracker import Tracker
    from tests import icp_restatement as IR
    from tests import track_restatement as TR
    tracker = Tracker(default_tracking_settings(), Signal(), Signal(), Signal(), device=DEV)
    clouds = []
    for k in range(2):
        dirs, dist, ts = TR.distorted_scan(k, 64, 1024)
        clouds.append(tracker.frame_cloud(Frame(None, LidarScan(dirs, dist, ts)).to(DEV)).points)
    yield "tracker frame (64 x 1024 scan, UNIFORM 5000)", clouds[0], clouds[1], 1.5
    yield "tracker frame (64 x 1024 scan, UNIFORM 5000)", clouds[0], clouds[1], 0.125
    if not skip_large:
        rng = np.random.default_rng(0)
        T = IR.rigid(0.2, [0.03, 0.0, -0.01])
        raw = IR.box_scene(0.03)
        gt = PointCloud(raw, DEV).voxel_down_sample(0.03)
        est = PointCloud(raw @ T[:3, :3].T + T[:3, 3] + rng.normal(size=raw.shape) * 0.002, DEV).voxel_down_sample(0.03)
        yield ("alignment pair (box 0.03 m)", gt.uniform_down_sample(alignment_skip(len(gt))).points,
               est.uniform_down_sample(alignment_skip(len(est))).points, 0.125)


def information(name, tgt, src, r, repeats):
    T = np.eye(4)
    grid = ops.NNGrid(tgt, r)
    normals = grid.normals(30)
    stats = {}
    REG.icp_information(grid, src, r, T, stats)
    print(f"information, {name}: {len(tgt)} targets, {len(src)} sources, r = {r} m: {stats['n_correspondences']} correspondences")
    print("  lnr_icp_correspondences      " + timed(lambda: grid.correspondences(src, r), repeats))
    print("  one point-to-plane round     " + timed(lambda: ops.icp_point_to_plane(grid, normals, src, r, T, max_iteration=0), repeats))
    print("  lnr_icp_information          " + timed(lambda: REG.icp_information(grid, src, r, T), repeats))


def loop_graph(n, seed=0):
    rng = np.random.default_rng(seed)
    truth = PR.ring_truth(n)
    noise = lambda: PR.step_matrix(np.concatenate([rng.normal(0, 0.002, 3), rng.normal(0, 0.003, 3)]))      # noqa: E731
    pairs = [(i, i + 1, False) for i in range(n - 1)] + [(i, (i + n // 3) % n, True) for i in range(0, n, 4)]
    X = np.stack([noise() @ PR.measure(truth, a, b) for a, b, _ in pairs])
    poses = [truth[0]]
    for k in range(n - 1):
        poses.append(poses[-1] @ PR.rigid_inverse(X[k]))
    L = np.tile(np.eye(6), (len(pairs), 1, 1))
    return PR.Graph(np.stack(poses), [p[0] for p in pairs], [p[1] for p in pairs], X, L, [p[2] for p in pairs], truth)


def optimise(n, repeats):
    g = loop_graph(n)
    crit, opt = PG.GlobalOptimizationConvergenceCriteria(), PG.GlobalOptimizationOption(0.1, reference_node=0)
    out = {}

    def run():
        dg = PG.DeviceGraph(g.n, g.source, g.target, g.X, g.L, g.uncertain, g.poses, DEV)
        out.update(dg.optimize(crit, opt))
    line = timed(run, repeats)
    cg = PG._max_cg(None, n)
    print(f"optimise, ring of {n} nodes, {g.m} edges: {line}")
    print(f"  {out['trials']} trials ({out['accepted']} accepted), stop {out['stop_reason']}, F {out['F']:.6e}, |b|inf {out['b_inf']:.3e}; "
          f"{out['cg_iterations']} conjugate-gradient iterations ({out['cg_iterations'] / max(out['trials'], 1):.0f} per trial); launches "
          f"enqueued per trial: 2 + 5 * {cg} (max_cg) + 7 = {9 + 5 * cg}, of which {9 + 5 * out['cg_iterations'] // max(out['trials'], 1)} do work; "
          f"{out['cg_capped']} trials ended their solve on max_cg")
    try:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
    except ImportError:
        print("  scipy is not present: no host comparison")
        return
    if n > 2048:
        print("  host comparison skipped above 2048 nodes (the restatement builds a dense H)")
        return
    solve = np.linalg.solve
    np.linalg.solve = lambda A, b: spl.spsolve(sp.csc_matrix(A), b)
    try:
        t0 = time.perf_counter()
        ref = PR.optimize(g, 0.1, reference=0)
        dt = time.perf_counter() - t0
    finally:
        np.linalg.solve = solve
    print(f"  numpy restatement with scipy's sparse solve: {dt * 1e3:.1f} ms, {len(ref['history'])} trials, F {ref['F']:.6e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--skip-information", action="store_true")
    ap.add_argument("--graphs", type=int, nargs="*", default=[64, 1024, 16384])
    a = ap.parse_args()
    if not a.skip_information:
        for pair in pairs(a.skip_large):
            information(*pair, a.repeats)
    for n in a.graphs:
        optimise(n, a.repeats)
