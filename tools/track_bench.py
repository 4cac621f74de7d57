"""Per-frame cost of the LiDAR tracker on one MI355X (profiles/tracker.txt).

Motion-distorted scans of the analytic scene (tests/track_restatement.py: 3 m/s, 20 deg/s; the returns above 12 degrees of
elevation are dropped over a 135 degree sector, so that there is sky to find) are tracked frame to frame.  For the
default configuration (UNIFORM, 5 000 points) and for VOXEL 0.1 m, on 64 x 1024 and 128 x 2048 scans, it reports
  * the whole Tracker.track_frame + compute_sky_rays call per frame: a host clock around work that ends in a device synchronise (a
    tracked frame contains host reads by construction: the window indices, one per registration, the pose), median over the frames
    after two warm-up frames;
  * the split of a frame, each piece timed the same way on the same inputs: cloud (window + lnr_frame_cloud, and the voxel
    down-sampling where configured), normals of the new target, every ICP stage with the rounds it ran, compensation, sky rays;
  * for scale, the restated pipeline on the host with scipy's cKDTree (workers=16), as profiles/icp.txt does: tree build, knn 30, and
    one round (nearest query + 6x6 system) times the rounds the device ran.
Gate (exit status 1 when missed): a tracked frame of the default configuration costs less than the frame period
1 / frame_decimation_rate_hz = 200 ms.  Everything else is recorded, not gated.

    python tools/track_bench.py [--out FILE] [--frames 8] [--skip-kdtree]
"""
import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 2


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--skip-kdtree", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench.py measures on the MI355X: no device found")
    from loner_amd.analysis.lidar_map import registration_icp
    from loner_amd.common.frame import Frame
    from loner_amd.common.sensors import LidarScan
    from loner_amd.common.settings import default_tracking_settings
    from loner_amd.common.signals import Signal
    from loner_amd.tracking.tracker import NORMALS_KNN, Tracker
    from tests import icp_restatement as IR
    from tests import track_restatement as TR
    lines = [f"# tools/track_bench.py on one MI355X: host clock around a device synchronise, median of {args.frames} frames after {WARMUP} "
             f"warm-up frames (host: scipy cKDTree, workers=16)", f"device: {torch.cuda.get_device_name(0)}"]

    def log(s):
        print(s, flush=True)
        lines.append(s)

    period_ms = None
    gate_ok = True
    for beams, azimuths in ((64, 1024), (128, 2048)):
        # the closed scene returns on every ray: open a patch of sky, so that the sky-ray leg compacts and emits directions
        scans = [TR.open_sky(*TR.distorted_scan(k, beams, azimuths)) for k in range(WARMUP + args.frames + 1)]
        for downsample in ("UNIFORM", "VOXEL"):
            settings = default_tracking_settings()
            settings["tracker"]["icp"]["downsample"]["type"] = downsample
            settings["tracker"]["compute_sky_rays"] = True
            period_ms = 1e3 / settings["tracker"]["frame_synthesis"]["frame_decimation_rate_hz"]
            schedule = settings.tracker.icp.schedule

            def frame_of(k):
                d, r, t = scans[k]
                return Frame(None, LidarScan(d.clone(), r.clone(), t.clone())).to("cuda")

            # ---- the whole call
            tracker = Tracker(settings, Signal(), Signal(), Signal(), device="cuda")
            whole = []
            for k in range(len(scans)):
                frame = frame_of(k)
                _, ms = clock(lambda: (tracker.track_frame(frame), tracker.compute_sky_rays(frame)))
                whole.append(ms)
            whole = whole[1 + WARMUP:]                   # the first frame is not tracked
            # ---- the split, on the same inputs
            split = {}
            rounds = []
            sizes = []
            probe = Tracker(settings, Signal(), Signal(), Signal(), device="cuda")
            prev = probe.frame_cloud(frame_of(0)).estimate_normals(NORMALS_KNN)
            for k in range(1, len(scans)):
                frame = frame_of(k)
                cloud, t_cloud = clock(lambda: probe.frame_cloud(frame))
                init, t_stage, n_rounds = np.eye(4), [], []
                for stage in schedule:
                    reg, ms = clock(lambda: registration_icp(cloud, prev, stage.threshold, init, stage.relative_fitness, stage.relative_rmse,
                                                             stage.max_iterations))
                    init = reg.transformation.copy()
                    t_stage.append(ms)
                    n_rounds.append(reg.iterations)
                _, t_normals = clock(lambda: cloud.estimate_normals(NORMALS_KNN))
                from loner_amd.common.pose import Pose
                host_pose = Pose(torch.from_numpy(init).float(), requires_tensor=True)       # as Tracker.track_frame holds it
                pose = copy.deepcopy(host_pose).to("cuda")
                mid = frame.get_middle_time()
                _, t_comp = clock(lambda: frame.lidar_points.motion_compensate((Pose(), host_pose), (mid - 0.1, mid), host_pose, True))
                frame._lidar_pose = pose
                _, t_sky = clock(lambda: probe.compute_sky_rays(frame))
                if k > WARMUP:
                    for name, ms in (("cloud", t_cloud), ("normals", t_normals), ("compensation", t_comp), ("sky rays", t_sky)):
                        split.setdefault(name, []).append(ms)
                    for j, ms in enumerate(t_stage):
                        split.setdefault(f"icp {schedule[j].threshold} m", []).append(ms)
                    rounds.append(n_rounds)
                    sizes.append((len(cloud), len(prev), frame.lidar_points.sky_rays.shape[1]))
                prev = cloud
            med = statistics.median
            log(f"\n{beams} x {azimuths} ({len(scans[0][1])} returns), {downsample}: cloud {sizes[-1][0]} points onto {sizes[-1][1]}, "
                f"{sizes[-1][2]} sky rays")
            log(f"  tracked frame (track_frame + compute_sky_rays): median {med(whole):.2f} ms, min {min(whole):.2f}, max {max(whole):.2f}"
                f"  [frame period {period_ms:.0f} ms]")
            log("  split: " + "; ".join(f"{name} {med(v):.2f} ms" for name, v in split.items())
                + f"; rounds per stage {[round(float(np.mean(r)), 1) for r in zip(*rounds)]}")
            if downsample == "UNIFORM" and not med(whole) < period_ms:
                gate_ok = False
            if not args.skip_kdtree:
                from scipy.spatial import cKDTree
                d, r, t = scans[-1]
                src = TR.frame_cloud(d, r, t, 0.9, 5000 if downsample == "UNIFORM" else None)[3]
                d, r, t = scans[-2]
                tgt = TR.frame_cloud(d, r, t, 0.9, 5000 if downsample == "UNIFORM" else None)[3]
                if downsample == "VOXEL":
                    from tests import cloud_restatement as CR
                    src, tgt = CR.voxel_down_sample(src, 0.1), CR.voxel_down_sample(tgt, 0.1)
                t0 = time.perf_counter()
                tree = cKDTree(tgt)
                t1 = time.perf_counter()
                idx = tree.query(tgt, k=30, workers=16)[1]
                nrm = IR.normal_rule(IR.covariance(tgt, idx))[0]
                t2 = time.perf_counter()
                dd, ii = tree.query(src, distance_upper_bound=1.5, workers=16)
                ok = np.isfinite(dd)
                IR.system(src[ok], tgt, nrm, ii[ok])
                t3 = time.perf_counter()
                total_rounds = float(np.mean([sum(r) for r in rounds]))
                host = 1e3 * ((t2 - t0) + (t3 - t2) * total_rounds)
                log(f"  host cKDTree (16 threads): build {1e3 * (t1 - t0):.1f} ms, knn 30 + normals {1e3 * (t2 - t1):.1f} ms, one round "
                    f"(query + system) {1e3 * (t3 - t2):.1f} ms -> {host:.0f} ms for the {total_rounds:.1f} rounds of a frame")
    log(f"\ngate: default configuration below the frame period of {period_ms:.0f} ms: {'met' if gate_ok else 'MISSED'}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if gate_ok else 1


if __name__ == "__main__":
    sys.exit(main())
