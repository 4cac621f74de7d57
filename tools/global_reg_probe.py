"""Global registration (profiles/global_reg.txt): what FPFH, the feature search and RANSAC cost on one MI355X, beside the same steps
on a 16-thread cKDTree and numpy (the restatement of tests/global_reg_restatement.py), on
  1. the tracker's default frame: two consecutive motion-distorted 64 x 1024 scans thinned to about 5 000 points (UNIFORM);
  2. an alignment pair of the synthetic room at 0.05 m (the box scene, one copy moved and jittered).
Each device step is timed by events around the whole wrapper call (its host read included) after two warm-up calls; the median and
the spread of 5 repeats are printed.  RANSAC runs 65 536 hypotheses with the edge checker off (e = 0) and on (e = 0.9).  The feature
search of the room pair is reported as the measured rate of a 100 000 x 100 000 sample of its features.  Nothing is gated: no
throughput was promised for these fp64 kernels.

    python tools/global_reg_probe.py [--out FILE] [--skip-large] [--closed-loop FOLDER --estimated TUM]

--closed-loop: a folder of examples/simulate_sequence.py and the estimated_trajectory.txt of examples/run_sequence.py run on it
WITHOUT --gt (the estimate lives in its own first-frame coordinates).  The scans are merged along either trajectory
(gt_map.build_lidar_map) and the two maps are scored with compare_point_clouds, first as the evaluation does today and then with
global_alignment=True; no trajectory is used to align them.
"""
import argparse
import glob
import os
import statistics
import sys
import tempfile
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--closed-loop", default=None)
    ap.add_argument("--estimated", default=None)
    args = ap.parse_args()
    from loner_amd import ops
    from loner_amd.analysis import registration as REG
    from loner_amd.analysis.lidar_map import PointCloud, compare_point_clouds
    from tests import global_reg_restatement as GR
    from tests import icp_restatement as IR
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(t):
        return f"{t[0]:.3f} ms (repeats {t[1]:.3f} .. {t[2]:.3f})"

    def pair(name, src, tgt, voxel, baseline, sample=None):
        """src, tgt: fp64 [n,3] on the device"""
        radius, d = 5.0 * voxel, 1.5 * voxel
        say(f"\n{name}: {len(src)} source and {len(tgt)} target points; FPFH radius {radius} m, max_nn 32; RANSAC distance {d} m")
        gs, gt = ops.NNGrid(src), ops.NNGrid(tgt)
        ns, nt = gs.normals(30), gt.normals(30)
        for n, p in ((ns, src), (nt, tgt)):
            REG.orient_normals(n, p, location=p.mean(0))
        say(f"  target grid {fmt(timed(lambda: ops.NNGrid(tgt)))}, normals (knn 30) {fmt(timed(lambda: gt.normals(30)))}, orientation "
            f"{fmt(timed(lambda: REG.orient_normals(nt, tgt, location=(0.0, 0.0, 100.0))))}")
        REG.orient_normals(nt, tgt, location=tgt.mean(0))
        stats = {}
        ft = REG.fpfh(gt, nt, radius, 32, stats=stats)
        fs = REG.fpfh(gs, ns, radius, 32)
        t = timed(lambda: REG.fpfh(gt, nt, radius, 32))
        say(f"  FPFH of the target: {fmt(t)}, {len(tgt) / t[0] / 1e3:.3f} M points/s; {stats}")
        if sample is None:
            t = timed(lambda: REG.feature_nearest(ft, fs))
            say(f"  feature search {len(fs)} x {len(ft)} x 33: {fmt(t)}, {len(fs) * len(ft) / t[0] / 1e6:.2f} G pairs/s "
                f"({3 * 33 * len(fs) * len(ft) / t[0] / 1e9:.2f} fp64 TFLOP/s at 3 operations per dimension)")
            corr = REG.correspondences_from_features(fs, ft)
        else:
            qs, qt = fs[:sample].contiguous(), ft[:sample].contiguous()
            t = timed(lambda: REG.feature_nearest(qt, qs), repeats=3)
            say(f"  feature search on a {len(qs)} x {len(qt)} x 33 sample: {fmt(t)}, {len(qs) * len(qt) / t[0] / 1e6:.2f} G pairs/s "
                f"({3 * 33 * len(qs) * len(qt) / t[0] / 1e9:.2f} fp64 TFLOP/s); the whole {len(fs)} x {len(ft)} search at that rate: "
                f"{len(fs) * len(ft) / (len(qs) * len(qt)) * t[0] / 1e3:.2f} s")
            index, _ = REG.feature_nearest(qt, qs)
            corr = torch.stack([torch.arange(len(qs), device=index.device, dtype=torch.int32), index], dim=1).contiguous()
        for e in (0.0, 0.9):
            out = REG.ransac_correspondence(src, tgt, corr, d, e, 65536, 0, strict=False)
            t = timed(lambda: REG.ransac_correspondence(src, tgt, corr, d, e, 65536, 0, strict=False))
            say(f"  RANSAC, {len(corr)} correspondences, 65536 hypotheses, e = {e}: {fmt(t)}; {out['survivors']} survivors "
                f"({out['survivors'] * len(corr) / t[0] / 1e6:.2f} G scored pairs/s), {out['n_inliers']} inliers, rejected "
                f"{out['rejected_repeated']} / {out['rejected_edge']} / {out['rejected_frame']} (repeated / edge / frame)")
        if baseline:
            P, Q = src.cpu().numpy(), tgt.cpu().numpy()
            nq = nt.cpu().numpy()
            edges = GR.bin_edges()
            t_f, fq = host_ms(lambda: GR.fpfh(Q, nq, radius, 32, edges)[0])
            fp = fs.cpu().numpy()
            from scipy.spatial import cKDTree
            t_s, _ = host_ms(lambda: cKDTree(fq).query(fp, k=1, workers=16))
            c = corr.cpu().numpy()
            t_r, r = host_ms(lambda: GR.ransac(P, Q, c, 4096, 0, d, 0.9))
            say(f"  CPU (16-thread cKDTree + numpy): FPFH of the target {t_f:.0f} ms (same bits: {np.array_equal(fq, ft.cpu().numpy())}), "
                f"feature search by a 33-d cKDTree {t_s:.0f} ms, RANSAC with 4096 hypotheses at e = 0.9 {t_r:.0f} ms "
                f"({r['survivors']} survivors: {t_r / max(r['survivors'], 1):.2f} ms per scored hypothesis)")

    if not args.closed_loop:
        from loner_amd.common.frame import Frame
        from loner_amd.common.sensors import LidarScan
        from loner_amd.common.settings import default_tracking_settings
        from loner_amd.common.signals import Signal
        from loner_amd.tracking.tracker import Tracker
        from tests import track_restatement as TR
        tracker = Tracker(default_tracking_settings(), Signal(), Signal(), Signal(), device="cuda")
        clouds = []
        for k in range(2):
            dirs, dist, ts = TR.distorted_scan(k, 64, 1024)
            clouds.append(tracker.frame_cloud(Frame(None, LidarScan(dirs, dist, ts)).to("cuda")).points)
        pair("tracker frame (64 x 1024 scan, UNIFORM 5000)", clouds[1], clouds[0], 0.3, baseline=True)
        if not args.skip_large:
            rng = np.random.default_rng(0)
            T = IR.rigid(140, [3.0, -2.0, 1.5])
            raw = IR.box_scene(0.05)
            gt = PointCloud(raw, "cuda").voxel_down_sample(0.05)
            est = PointCloud(raw @ T[:3, :3].T + T[:3, 3] + rng.normal(size=raw.shape) * 0.002, "cuda").voxel_down_sample(0.05)
            pair("alignment pair (room at 0.05 m)", est.points, gt.points, 0.05, baseline=False, sample=100000)
    else:
        from loner_amd.analysis.gt_map import build_lidar_map
        files = sorted(glob.glob(os.path.join(args.closed_loop, "*.npy")))
        stamps = np.loadtxt(os.path.join(args.closed_loop, "stamps.txt"), dtype=np.float64, ndmin=1)
        scans = []
        for path, stamp in zip(files, stamps):
            rows = np.load(path).astype(np.float64)
            scans.append((rows[:, :3], rows[:, 3] + stamp))
        est = build_lidar_map(scans, args.estimated, 0.05, device="cuda")
        gt = build_lidar_map(scans, os.path.join(args.closed_loop, "gt_tum.txt"), 0.05, device="cuda")
        say(f"\n# the closed loop: {len(files)} simulated scans, the map merged along the estimated trajectory (its own first-frame "
            f"coordinates, {len(est)} points) against the map merged along the ground truth ({len(gt)} points), no trajectory used to align them")
        out = os.path.join(os.path.dirname(os.path.abspath(args.out)) if args.out else tempfile.gettempdir(), "global_reg_loop")
        for how in (False, True):
            info = {}
            try:
                s = compare_point_clouds(est, gt, out, 0.1, refine_alignment=True, alignment=info, global_alignment=how)
                say(f"global_alignment={how}: " + ", ".join(f"{k} {s[k]:.4f}" for k in ("accuracy", "completion", "chamfer_distance", "precision",
                                                                                         "recall", "f-score"))
                    + (f"; global fitness {info['global']['fitness']:.4f}" if how else "") + f"; ICP fitness {info['fitness']:.4f}")
            except (RuntimeError, ValueError) as err:
                say(f"global_alignment={how}: {type(err).__name__}: {err}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.closed_loop else "w") as f:
            f.write("\n".join(lines[1:] if args.closed_loop else lines) + "\n")


if __name__ == "__main__":
    main()
