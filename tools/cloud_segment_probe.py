"""Segmentation (profiles/cloud_segment.txt): what the radius count, DBSCAN and the RANSAC plane cost on one MI355X, beside the same
work on 16 CPU threads, on
  1. the tracker's default frame: a motion-distorted 64 x 1024 scan thinned to about 5 000 points (voxel 0.3 m);
  2. the synthetic room at 0.05 m (the box scene down-sampled, 1.2-1.4 M points).
Each device figure is the median (and the spread) of 5 calls after two warm-up calls, timed by events around the whole wrapper call.
The count and the plane include their one host read; dbscan reads nothing back, and its grid build is timed apart.  The passes
of DBSCAN are the kernels' own durations from one profiled call (torch.profiler), so they do not add up to the event time of the
call, which also holds the launches and three memsets.  CPU baselines: the restatement (tests/segment_restatement.py: cKDTree with
16 workers and the sequential walk; the same bytes), scikit-learn's DBSCAN with n_jobs=16 where it imports, and the restatement's
vectorised numpy RANSAC.  Nothing is gated: no throughput was promised for these fp64 kernels.

    python tools/cloud_segment_probe.py [--out FILE] [--skip-large]
"""
import argparse
import os
import re
import statistics
import sys
import time

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


def timed(fn, repeats=5):
    fn(), fn()
    torch.cuda.synchronize()
    ts = [call_ms(fn) for _ in range(repeats)]
    return statistics.median(ts), min(ts), max(ts)


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_times(fn):
    """{kernel name: device microseconds} of one call"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None)
        t = getattr(e, "cuda_time_total", 0.0) if t is None else t
        if t:
            out[e.key] = out.get(e.key, 0.0) + float(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    from loner_amd import ops
    from loner_amd.analysis import segmentation as SEG
    from loner_amd.analysis.lidar_map import PointCloud
    from tests import icp_restatement as IR
    from tests import segment_restatement as SR
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(t):
        return f"{t[0]:.3f} ms (repeats {t[1]:.3f} .. {t[2]:.3f})"

    def cloud(name, pts, voxel, min_points, cpu_eps, cpu_planes):
        """pts: fp64 [n,3] on the device"""
        n = len(pts)
        P = pts.cpu().numpy()
        say(f"\n{name}: {n} points, voxel {voxel} m, min_points {min_points}")
        for f in (2, 5):
            eps = f * voxel
            grid = ops.NNGrid(pts, eps)
            stats = {}
            counts = SEG.radius_count(grid, eps, stats=stats)
            t_g, t_c = timed(lambda: ops.NNGrid(pts, eps)), timed(lambda: SEG.radius_count(grid, eps))
            say(f"  eps = {f} voxels = {eps:g} m: grid build (edge = eps) {fmt(t_g)}; count pass {fmt(t_c)}, mean count "
                f"{float(counts.double().mean()):.1f}, {stats['shells'] / n:.2f} shells per point, {n / t_c[0] / 1e3:.2f} M points/s")
            labels, info = SEG.dbscan(grid, eps, min_points)
            t_d = timed(lambda: SEG.dbscan(grid, eps, min_points))
            w = [int(x) for x in info.cpu()]
            say(f"    DBSCAN (no host read, grid apart) {fmt(t_d)}: {w[1]} clusters, {w[2]} cores, {w[3]} border, {w[4]} noise")
            try:
                k = kernel_times(lambda: SEG.dbscan(grid, eps, min_points))
                ours = {}
                for name, us in k.items():
                    m = re.search(r"\b((?:seg|db)_[a-z_]+(?:<[a-z]+>)?)", name)
                    if m:
                        ours[m.group(1)] = ours.get(m.group(1), 0.0) + us
                say("    its passes: " + ", ".join(f"{name} {us / 1e3:.3f} ms" for name, us in sorted(ours.items(), key=lambda kv: -kv[1])))
            except Exception as err:                    # the profiler is a convenience of the probe
                say(f"    its passes: not measured ({type(err).__name__}: {err})")
            if f in cpu_eps:
                t_n, nbrs = host_ms(lambda: SR.radius_neighbours(P, eps))
                t_w, (ref, _) = host_ms(lambda: SR.dbscan(P, eps, min_points, nbrs))
                say(f"    CPU restatement: neighbours (cKDTree, 16 workers, exact filter) {t_n:.0f} ms + sequential walk {t_w:.0f} ms; "
                    f"same bytes: {np.array_equal(ref, labels.cpu().numpy())}; counts equal: "
                    f"{np.array_equal(SR.radius_counts(P, eps, nbrs), counts.cpu().numpy())}")
                try:
                    from sklearn.cluster import DBSCAN
                    t_s, sk = host_ms(lambda: DBSCAN(eps=eps, min_samples=min_points, n_jobs=16).fit(P))
                    say(f"    scikit-learn DBSCAN (n_jobs=16; d <= eps, another border rule): {t_s:.0f} ms, {int(sk.labels_.max()) + 1} clusters")
                except ImportError:
                    say("    scikit-learn does not import here")
        t = 0.4 * voxel
        for H in (100, 1000, 65536):
            out = SEG.plane_ransac(pts, t, H, 0, True)
            t_p = timed(lambda: SEG.plane_ransac(pts, t, H, 0, True))
            say(f"  segment_plane, threshold {t:g} m, H = {H}: {fmt(t_p)} with the refit and one host read; {out['n_inliers']} inliers, "
                f"{out['survivors']} survivors, {H * n / t_p[0] / 1e6:.2f} G point-plane tests/s")
            if H in cpu_planes:
                t_r, r = host_ms(lambda: SR.segment_plane(P, t, H, 0, True))
                say(f"    numpy RANSAC (the restatement, vectorised over hypotheses): {t_r:.0f} ms; same best hypothesis and mask: "
                    f"{r['best_hypothesis'] == out['best_hypothesis'] and np.array_equal(r['inlier'], out['inlier'].cpu().numpy().astype(bool))}")

    from loner_amd.common.frame import Frame
    from loner_amd.common.sensors import LidarScan
    from loner_amd.common.settings import default_tracking_settings
    from loner_amd.common.signals import Signal
    from loner_amd.tracking.tracker import Tracker
    from tests import track_restatement as TR
    tracker = Tracker(default_tracking_settings(), Signal(), Signal(), Signal(), device="cuda")
    dirs, dist, ts = TR.distorted_scan(0, 64, 1024)
    frame = tracker.frame_cloud(Frame(None, LidarScan(dirs, dist, ts)).to("cuda")).points
    cloud("tracker frame (64 x 1024 scan, UNIFORM 5000)", frame, 0.3, 5, cpu_eps=(2, 5), cpu_planes=(100, 1000))
    if not args.skip_large:
        room = PointCloud(IR.box_scene(0.05), "cuda").voxel_down_sample(0.05).points
        cloud("room at 0.05 m", room, 0.05, 10, cpu_eps=(2,), cpu_planes=(100,))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
