"""Measures scan ingestion and the SLAM loop's per-frame wall time on the GPU; writes profiles/slam_loop.txt.

    python tools/slam_loop_profile.py [--out profiles/slam_loop.txt] [--repeats 60]

1. build_scan_from_points on a 128 x 2048 scan (row-major beam order, local times, two FOV segments) from host arrays, against the
   torch CPU restatement (tests/scan_restatement.py, 16 threads) followed by the upload of its result.  The two alternate inside one
   loop after a warm-up; every sample is a host clock around work that ends in a device synchronise.  Median, 10th and 90th
   percentile, min and max are reported.  A third row times the device path alone, from device-resident inputs.
2. The twelve-frame run of tests/test_gpu_slam.py (32 x 512 scans, four keyframes: 60 + 3 x 20 mapping iterations), every frame split
   into ingest, log, track and map, each closed by a device synchronise."""
import argparse
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import scan_restatement as SR            # noqa: E402
from tests import test_gpu_slam as TS               # noqa: E402

SEGMENTS = [[0.0, 235.0], [305.0, 360.0]]


def big_scan(beams=128, columns=2048):
    gen = torch.Generator().manual_seed(1)
    az = (torch.arange(columns, dtype=torch.float64) / columns * 2 * np.pi).repeat(beams)
    el = torch.deg2rad(torch.linspace(-22.5, 22.5, beams, dtype=torch.float64)).repeat_interleave(columns)
    r = 0.2 + 40.0 * torch.rand(beams * columns, generator=gen, dtype=torch.float64)
    xyz = torch.stack([r * torch.cos(el) * torch.cos(az), r * torch.cos(el) * torch.sin(az), r * torch.sin(el)], 1).float().contiguous()
    local = (torch.arange(columns, dtype=torch.float64) / columns * 0.1).repeat(beams).float()
    return xyz, local


def clocked(fn):
    torch.cuda.synchronize()
    start = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3, out


def row(name, samples):
    s = np.sort(np.asarray(samples))
    pick = lambda q: s[min(len(s) - 1, int(round(q * (len(s) - 1))))]
    return f"{name:<58s} median {np.median(s):8.3f}   p10 {pick(0.1):8.3f}   p90 {pick(0.9):8.3f}   min {s[0]:8.3f}   max {s[-1]:8.3f}   (n = {len(s)})"


def ingestion(lines, repeats):
    from loner_amd.common.sensors import build_scan_from_points
    torch.set_num_threads(16)
    xyz, local = big_scan()
    fov = SimpleNamespace(enabled=True, range=SEGMENTS)
    stamp = 1234.5

    def device_path():
        return build_scan_from_points(xyz, local, stamp, fov=fov, device="cuda")

    def host_path():
        out = SR.scan_from_points(xyz, local, stamp, SEGMENTS)
        return [out[k].cuda() for k in ("directions", "distances", "timestamps", "order")]

    xyz_d, local_d = xyz.cuda(), local.cuda()

    def resident_path():
        return build_scan_from_points(xyz_d, local_d, stamp, fov=fov)

    for _ in range(10):
        device_path(), host_path(), resident_path()
    dev, host, res = [], [], []
    for _ in range(repeats):
        dev.append(clocked(device_path)[0])
        host.append(clocked(host_path)[0])
        res.append(clocked(resident_path)[0])
    scan, order = device_path()
    want = SR.scan_from_points(xyz, local, stamp, SEGMENTS)
    same = torch.equal(order.cpu(), want["order"]) and torch.equal(scan.timestamps.cpu(), want["timestamps"])
    lines += [f"1. scan ingestion, 128 x 2048 = {len(xyz)} points, local times, FOV {SEGMENTS}: {len(order)} points kept; order and times "
              f"equal the restatement's: {same}", "   wall time per scan in ms, host clock closed by a device synchronise, the three alternating in one loop",
              "   " + row("build_scan_from_points, host arrays in (upload + device)", dev),
              "   " + row("restatement on 16 host threads + upload of its result", host),
              "   " + row("build_scan_from_points, device arrays in", res), ""]


def loop(lines, root):
    from loner_amd.common.pose import Pose
    from loner_amd.common.sensors import build_scan_from_points
    from loner_amd.loner import Loner
    raw = TS.raw_scans()
    truth = torch.stack([r[3] for r in raw])
    table = []
    for attempt in ("warm-up run", "timed run"):
        torch.manual_seed(0)
        loner = Loner(TS.slam_settings(root))
        loner.initialize(None, truth, None, [1, 50], None, root, experiment_name=attempt.replace(" ", "_"))
        loner.start()
        table = []
        for k, (xyz, local, stamp, _) in enumerate(raw):
            t_ingest, (scan, _) = clocked(lambda: build_scan_from_points(xyz, local, stamp, device="cuda"))
            t_log, _ = clocked(loner._logger.update)
            loner._lidar_signal.emit((scan, Pose(truth[k].clone())))
            t_track, _ = clocked(loner._tracker.update)
            t_map, _ = clocked(loner._mapper.update)
            table.append((t_ingest, t_track, t_map, t_log))
        t_stop, _ = clocked(loner.stop)
    lines += ["2. the twelve-frame run (32 x 512 scans, keyframes at frames 0, 3, 6, 9: 60 + 3 x 20 mapping iterations of 256 rays x 64 samples),",
              "   second run in the process; wall time per frame in ms, every part closed by a device synchronise",
              "   frame    ingest     track       map       log"]
    for k, r in enumerate(table):
        lines.append(f"   {k:5d}  {r[0]:8.3f}  {r[1]:8.3f}  {r[2]:8.3f}  {r[3]:8.3f}" + ("   keyframe" if k in TS.KEYFRAME_FRAMES else ""))
    t = np.array(table)
    lines.append("   median " + "  ".join(f"{np.median(t[:, c]):8.3f}" for c in range(4)))
    lines.append("   total  " + "  ".join(f"{t[:, c].sum():8.3f}" for c in range(4)) + f"   stop() {t_stop:.3f}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slam_loop.txt"))
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--scratch", default=None, help="where the runs' log directories go (default: a temporary directory)")
    args = ap.parse_args()
    lines = [f"tools/slam_loop_profile.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    ingestion(lines, args.repeats)
    loop(lines, args.scratch or tempfile.mkdtemp(prefix="slam_loop_"))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
