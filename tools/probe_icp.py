"""Normals and point-to-plane ICP costs at the reference's alignment size (profiles/icp.txt), device events after a warm-up:
  1. the grid build and the kNN normals (knn 30) of the target;
  2. one correspondence pass alone (lnr_icp_correspondences), and lnr_icp_point_to_plane with 0, 1 and 10 rounds (criteria 0, so
     that no round stops early): a round costs (t10 - t0) / 10;
  3. the restated pipeline on the host for scale: scipy's cKDTree with workers=16 (normals: one knn query; a round: one nearest query
     plus the 6x6 system in numpy).
Clouds: the box scene sampled at 0.03 m, down-sampled and uniformly sub-sampled as evaluate_lidar_map.py does (1-2 M points), with a
mis-aligned noisy copy as the source; and a scan-like cloud (one rendered-looking 64 x 2048 beam pattern per pose over 12 poses).
Run under rocprofv3 --kernel-trace --stats for the split of a round into search, fold, solve and transform.

    python tools/probe_icp.py [--out FILE] [--skip-kdtree]
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


def scan_cloud(n_poses=12, rows=64, cols=2048):
    """points where beams from poses along a line hit the box scene's walls (ray casting against the box, no sphere)"""
    from loner_amd.utils import synthetic as SY
    lo, hi = np.array(SY.BOX_MIN), np.array(SY.BOX_MAX)
    el = np.deg2rad(np.linspace(-22.5, 22.5, rows))
    az = np.linspace(0, 2 * np.pi, cols, endpoint=False)
    E, A = np.meshgrid(el, az, indexing="ij")
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    out = []
    for k in range(n_poses):
        o = np.array([-15.0 + 30.0 * k / max(n_poses - 1, 1), 0.5 * np.sin(k), 1.5])
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf))
        out.append(o + d * t.min(1, keepdims=True))
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-kdtree", action="store_true")
    args = ap.parse_args()
    from loner_amd import ops
    from loner_amd.analysis.lidar_map import PointCloud, alignment_skip
    from tests import icp_restatement as IR
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def log(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    T = IR.rigid(0.2, [0.03, 0.0, -0.01])
    for name, raw in (("box 0.03 m", IR.box_scene(0.03)), ("scan-like", scan_cloud())):
        gt = PointCloud(raw, "cuda").voxel_down_sample(0.03)
        est_np = raw @ T[:3, :3].T + T[:3, 3] + rng.normal(size=raw.shape) * 0.002
        est = PointCloud(est_np, "cuda").voxel_down_sample(0.03)
        tgt = gt.uniform_down_sample(alignment_skip(len(gt))).points
        src = est.uniform_down_sample(alignment_skip(len(est))).points
        log(f"\n{name}: {len(raw)} raw, {len(gt)} / {len(est)} down-sampled, alignment target {len(tgt)}, source {len(src)}")
        t_grid = timed(lambda: ops.NNGrid(tgt), 10)
        g = ops.NNGrid(tgt, 0.125)
        stats = {}
        t_norm = timed(lambda: g.normals(30), 5)
        normals = g.normals(30, stats=stats)
        log(f"  grid build (default edge) {t_grid:.3f} ms; kNN normals (k 30) {t_norm:.3f} ms  {stats}")
        t_corr = timed(lambda: g.correspondences(src, 0.125), 10)
        t_icp = {k: timed(lambda: ops.icp_point_to_plane(g, normals, src, 0.125, relative_fitness=0.0, relative_rmse=0.0,
                                                         max_iteration=k), 5) for k in (0, 1, 10)}
        out = ops.icp_point_to_plane(g, normals, src, 0.125, relative_fitness=0.0, relative_rmse=0.0, max_iteration=10)
        log(f"  correspondence pass alone {t_corr:.3f} ms; icp 0 / 1 / 10 rounds {t_icp[0]:.3f} / {t_icp[1]:.3f} / {t_icp[10]:.3f} ms"
            f" -> {(t_icp[10] - t_icp[0]) / 10:.3f} ms per round; fitness {out['fitness']:.4f} rmse {out['inlier_rmse']:.4g}")
        if not args.skip_kdtree:
            from scipy.spatial import cKDTree
            t_np, s_np = tgt.cpu().numpy(), src.cpu().numpy()
            n_np = normals.cpu().numpy()
            t0 = time.perf_counter()
            tree = cKDTree(t_np)
            t1 = time.perf_counter()
            tree.query(t_np, k=30, workers=16)
            t2 = time.perf_counter()
            d, i = tree.query(s_np, distance_upper_bound=0.125, workers=16)
            ok = np.isfinite(d)
            IR.system(s_np[ok], t_np, n_np, i[ok])
            t3 = time.perf_counter()
            log(f"  host cKDTree (16 threads): build {1e3 * (t1 - t0):.1f} ms, knn 30 {1e3 * (t2 - t1):.1f} ms, "
                f"one round (query + system) {1e3 * (t3 - t2):.1f} ms")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
