"""Mesh sampling, outlier filter and trajectory transform costs at the reference's sizes (profiles/cloud_tools.txt), device events
after a warm-up, each beside its numpy / scipy restatement on 16 threads:
  1. 50 M samples (mesh_to_pcd.py's count) of the synthetic box's surface as the mesher's marching cubes gives it at 0.1 m, the
     down-sample to 0.05 m that follows, and a plain fill of the same 1.2 GB as the write-bound yardstick;
  2. remove_statistical_outlier(20, 1.5) on the box cloud of profiles/icp.txt (0.03 m, down-sampled, every third point): the grid
     build, the neighbour means, the threshold and the compaction;
  3. the trajectory transform of one 128 x 2048 scan against a 100 Hz trajectory of 2000 poses.

    python tools/probe_cloud_tools.py [--out FILE] [--skip-host] [--points N]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def box_mesh(step, dev):
    """marching cubes over the box's inside-distance (positive inside), sampled at `step`: the closed surface of the synthetic box"""
    from loner_amd import ops
    from loner_amd.utils import synthetic as SY
    lo, hi = np.array(SY.BOX_MIN) - 2 * step, np.array(SY.BOX_MAX) + 2 * step
    axes = [torch.arange(lo[a], hi[a] + 0.5 * step, step, device=dev, dtype=torch.float32) for a in range(3)]
    X, Y, Z = torch.meshgrid(*axes, indexing="ij")
    inside = torch.stack([X - SY.BOX_MIN[0], SY.BOX_MAX[0] - X, Y - SY.BOX_MIN[1], SY.BOX_MAX[1] - Y, Z - SY.BOX_MIN[2],
                          SY.BOX_MAX[2] - Z]).amin(0) + 0.37 * step          # the surface off the lattice planes
    verts, faces = ops.marching_cubes(inside.contiguous(), 0.0, (step, step, step), tuple(float(x) for x in lo))
    return verts.to(torch.float64), faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--points", type=int, default=50_000_000)
    args = ap.parse_args()
    from loner_amd import ops
    from loner_amd.analysis.gt_map import load_trajectory
    from loner_amd.analysis.lidar_map import PointCloud
    from tests import cloud_restatement as CR
    from tests import cloud_tools_restatement as TR
    from tests import icp_restatement as IR
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def log(s):
        print(s, flush=True)
        lines.append(s)

    # ---- 1. sampling
    n = args.points
    verts, faces = box_mesh(0.1, dev)
    info = {}
    ops.mesh_sample_points(verts, faces, 0, 0, info=info)
    log(f"\nsampling: box mesh at 0.1 m, {verts.shape[0]} vertices, {faces.shape[0]} triangles, area {info['area']:.2f} m^2; {n} points")
    ops.profile_enable(True)
    ops.profile_read()
    pts = ops.mesh_sample_points(verts, faces, n, 0)
    torch.cuda.synchronize()
    prof = ops.profile_read()
    ops.profile_enable(False)
    t_sample = timed(lambda: ops.mesh_sample_points(verts, faces, n, 0), 3)
    t_small = timed(lambda: ops.mesh_sample_points(verts, faces, 256, 0), 3)
    fill = torch.empty(n, 3, device=dev, dtype=torch.float64)
    t_fill = timed(lambda: fill.fill_(1.0), 5)
    del fill
    gb = 24e-9 * n
    log(f"  lnr_mesh_sample_points {t_sample:.2f} ms incl. the allocation and the info read-back ({gb / t_sample * 1e3:.0f} GB/s of output); "
        f"on the device alone {prof.get('mesh_sample_points', {}).get('total_ms', float('nan')):.2f} ms")
    log(f"  the same call for 256 points (areas, cdf tree, bounds: everything but the points) {t_small:.3f} ms")
    log(f"  plain fill of the same {gb:.2f} GB (torch fill_) {t_fill:.2f} ms ({gb / t_fill * 1e3:.0f} GB/s)")
    t_down = timed(lambda: ops.voxel_down_sample(pts, 0.05), 2)
    down = ops.voxel_down_sample(pts, 0.05)
    log(f"  voxel_down_sample(0.05) of them {t_down:.1f} ms -> {down.shape[0]} points")
    del down
    if not args.skip_host:
        v_np, f_np = verts.cpu().numpy(), faces.cpu().numpy()
        m = n // 10
        t0 = time.perf_counter()
        TR.mesh_sample(v_np, f_np, m, 0)
        t1 = time.perf_counter()
        log(f"  host numpy restatement, {m} points (a tenth): {1e3 * (t1 - t0):.0f} ms -> {1e4 * (t1 - t0):.0f} ms for all, one thread "
            f"(numpy's element-wise kernels do not thread)")
    del pts

    # ---- 2. outlier filter
    raw = IR.box_scene(0.03)
    cloud = PointCloud(raw, dev).voxel_down_sample(0.03).uniform_down_sample(3)
    p = cloud.points
    log(f"\noutlier filter: box 0.03 m, {len(raw)} raw, {len(p)} points")
    t_grid = timed(lambda: ops.NNGrid(p), 5)
    g = ops.NNGrid(p)
    stats = {}
    avg = g.knn_mean_distance(20, stats=stats)
    t_avg = timed(lambda: g.knn_mean_distance(20), 5)
    t_thr = timed(lambda: g.outlier_threshold(avg, 1.5), 10)
    t_all = timed(lambda: cloud.remove_statistical_outlier(20, 1.5), 3)
    kept, _ = cloud.remove_statistical_outlier(20, 1.5)
    res = g.outlier_threshold(avg, 1.5).cpu().numpy()
    log(f"  grid build {t_grid:.3f} ms; neighbour means (k 20) {t_avg:.3f} ms  {stats}; threshold {t_thr:.3f} ms; "
        f"remove_statistical_outlier in all {t_all:.3f} ms")
    log(f"  mean {res[0]:.6g} std {res[1]:.6g} threshold {res[2]:.6g}; kept {len(kept)} of {len(p)}")
    if not args.skip_host:
        from scipy.spatial import cKDTree
        p_np = p.cpu().numpy()
        t0 = time.perf_counter()
        tree = cKDTree(p_np)
        t1 = time.perf_counter()
        d, _ = tree.query(p_np, k=20, workers=16)
        a = d.mean(1)
        thr = a.mean() + 1.5 * a.std(ddof=1)
        keep = p_np[a < thr]
        t2 = time.perf_counter()
        log(f"  host cKDTree (16 threads): build {1e3 * (t1 - t0):.1f} ms, knn 20 + statistics + selection {1e3 * (t2 - t1):.1f} ms "
            f"(kept {len(keep)})")

    # ---- 3. trajectory transform
    from scipy.spatial.transform import Rotation
    K = 2000
    T = 1.7e9 + 0.01 * np.arange(K)
    rng = np.random.default_rng(0)
    P = np.cumsum(rng.normal(size=(K, 3)) * 0.01, axis=0) + [5.0, 3.0, 1.0]
    rot = Rotation.from_rotvec(np.cumsum(rng.normal(size=(K, 3)) * 0.002, axis=0))
    rows = np.concatenate([T[:, None], P, rot.as_quat()], axis=1)
    traj = load_trajectory(rows, dev)
    m = 128 * 2048
    d = rng.normal(size=(m, 3))
    scan = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.2, 60.0, size=(m, 1))
    stamps = np.sort(rng.uniform(T[500], T[510], size=m))
    sd, td = torch.from_numpy(scan).to(dev), torch.from_numpy(stamps).to(dev)
    t_tr = timed(lambda: ops.trajectory_transform(sd, td, traj, 0.5), 20)
    out, tinfo = ops.trajectory_transform(sd, td, traj, 0.5)
    tinfo = tinfo.cpu().numpy()
    log(f"\ntrajectory transform: {m} points (128 x 2048), {K} poses: {t_tr:.3f} ms (count, scan, emit; no host read); "
        f"kept {tinfo[1]}, below range {tinfo[2]}, outside {tinfo[3]}")
    if not args.skip_host:
        t0 = time.perf_counter()
        want = TR.trajectory_transform(scan, stamps, rows, 0.5)
        t1 = time.perf_counter()
        err = np.abs(out.cpu().numpy()[:tinfo[1]] - want["points"])
        ratio = (err / TR.transform_bound(scan[want["index"]], want["trans"])[:, None]).max() * TR.TRANSFORM_BOUND_ULPS
        log(f"  host scipy Slerp + interp1d + einsum: {1e3 * (t1 - t0):.1f} ms, one thread (neither threads); max |device - scipy| "
            f"{err.max():.3e} m = {ratio:.1f} u (|p| + |trans|)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
