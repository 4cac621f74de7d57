"""Generalized ICP beside point-to-plane ICP (profiles/gicp.txt): the cost of a round of lnr_icp_generalized with L2 and with Tukey
next to a round of lnr_icp_point_to_plane on the same clouds in the same process, on
  1. the tracker's default frame: two consecutive motion-distorted 64 x 1024 scans thinned to about 5 000 points (UNIFORM), at both
     thresholds of the default schedule (1.5 m and 0.125 m);
  2. the alignment pair of profiles/icp.txt: the box scene at 0.03 m, down-sampled and sub-sampled as evaluate_lidar_map.py does
     (1.2 M targets, 1.3 M sources), at 0.125 m.
A round costs (t10 - t0) / 10 with criteria 0 (no round stops early), t by device events around whole calls (one host read each)
after a warm-up; the three estimators alternate within each of 5 repeats, and the median and the spread of the repeats are printed.
The search is shared, so the expectation is a ratio near 1; no gate.  The covariances' cost (kNN normals and the plane rule) is
printed beside the point-to-plane target's normals.

    python tools/gicp_probe.py [--out FILE] [--append FILE] [--skip-large]

--append: a text file (the closed-loop runs' APE lines) copied to the end of the report.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def round_times(calls, reps, repeats=5):
    """calls: name -> fn(max_iteration).  -> name -> list of per-round ms, one per repeat; the names alternate within a repeat"""
    for fn in calls.values():
        fn(0), fn(10)
    torch.cuda.synchronize()
    out = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            t0 = statistics.median(call_ms(lambda: fn(0)) for _ in range(reps))
            t10 = statistics.median(call_ms(lambda: fn(10)) for _ in range(reps))
            out[name].append((t10 - t0) / 10)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", default=None)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    from loner_amd import ops
    from loner_amd.analysis.lidar_map import PointCloud, alignment_skip
    from loner_amd.analysis.registration import RobustKernel, icp_generalized, plane_covariances
    from loner_amd.common.frame import Frame
    from loner_amd.common.sensors import LidarScan
    from loner_amd.common.settings import default_tracking_settings
    from loner_amd.common.signals import Signal
    from loner_amd.tracking.tracker import Tracker
    from tests import icp_restatement as IR
    from tests import track_restatement as TR
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def pair(name, tgt, src, radii, reps):
        g0 = ops.NNGrid(tgt)
        normals = g0.normals(30)
        t_n30 = statistics.median(call_ms(lambda: g0.normals(30)) for _ in range(5))
        t_cov = statistics.median(call_ms(lambda: plane_covariances(g0.normals(20), 1e-3)) for _ in range(5))
        tc = plane_covariances(g0.normals(20), 1e-3)
        sc = plane_covariances(ops.NNGrid(src).normals(20), 1e-3)
        say(f"\n{name}: {len(tgt)} targets, {len(src)} sources; target normals (knn 30) {t_n30:.3f} ms, target covariances (knn 20 normals "
            f"+ plane rule) {t_cov:.3f} ms")
        for r in radii:
            g = ops.NNGrid(tgt, r)
            crit = dict(relative_fitness=0.0, relative_rmse=0.0)
            calls = {"point to plane": lambda k: ops.icp_point_to_plane(g, normals, src, r, max_iteration=k, **crit),
                     "generalized L2": lambda k: icp_generalized(g, tc, src, sc, r, max_iteration=k, **crit),
                     "generalized Tukey k=3": lambda k: icp_generalized(g, tc, src, sc, r, max_iteration=k, kernel=RobustKernel("tukey", 3.0),
                                                                        **crit)}
            times = round_times(calls, reps)
            base = statistics.median(times["point to plane"])
            for what, ts in times.items():
                out = calls[what](10)
                say(f"  r = {r} m, {what}: {statistics.median(ts):.4f} ms per round (repeats {min(ts):.4f} .. {max(ts):.4f}), "
                    f"{statistics.median(ts) / base:.3f} x point to plane; after 10 rounds fitness {out['fitness']:.4f} rmse "
                    f"{out['inlier_rmse']:.4g}")

    tracker = Tracker(default_tracking_settings(), Signal(), Signal(), Signal(), device="cuda")
    clouds = []
    for k in range(2):
        dirs, dist, ts = TR.distorted_scan(k, 64, 1024)
        clouds.append(tracker.frame_cloud(Frame(None, LidarScan(dirs, dist, ts)).to("cuda")).points)
    pair("tracker frame (64 x 1024 scan, UNIFORM 5000)", clouds[0], clouds[1], (1.5, 0.125), 9)
    if not args.skip_large:
        rng = np.random.default_rng(0)
        T = IR.rigid(0.2, [0.03, 0.0, -0.01])
        raw = IR.box_scene(0.03)
        gt = PointCloud(raw, "cuda").voxel_down_sample(0.03)
        est = PointCloud(raw @ T[:3, :3].T + T[:3, 3] + rng.normal(size=raw.shape) * 0.002, "cuda").voxel_down_sample(0.03)
        pair("alignment pair (box 0.03 m)", gt.uniform_down_sample(alignment_skip(len(gt))).points,
             est.uniform_down_sample(alignment_skip(len(est))).points, (0.125,), 3)
    if args.append and os.path.exists(args.append):
        say("\n# the closed loop: examples/simulate_sequence.py, then examples/run_sequence.py --gt on its folder with --icp-estimation / "
            "--icp-kernel")
        for line in open(args.append).read().splitlines():
            say(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
